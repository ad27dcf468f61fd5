"""Shared bodies of the spectral-diffusion tests (drivers: test_diffusion_emu.py on the emulator build, test_diffusion_gpu.py on the device): the
learned-time diffusion operator  xs = Phi^T (m x),  ys = exp(-lambda t^T) xs,  xd = Phi ys  and its backward as ONE isolated op against the fp64
evaluation of the same fp32 inputs, on every kernel route of its dispatch, on inputs that are hard on purpose (masses over six decades,
lambda_max = 4 pi K, times from the clamp floor 1e-8 to 1, channels scaled by 2^20 and 2^-20, a zero channel) and on benign ones, plus the
contracts beyond accuracy: where a non-finite value may go, underflow of exp(-lambda t), determinism, the exact workspace.

Criterion: the condition-scaled error  s = max |got - ref| / S,  S the reference expression evaluated on absolute values (``scales``); where
S = 0 the result must be exactly 0.  Two assertions, in this order: (a) s <= gamma_n = n u / (1 - n u), u = 2^-24, n counted from the operations
(``counts``; torch's own fp32 evaluation must pass it first); (b) s <= 4 max(s_torch32, 2 u), the margin of ``linear_cases`` for an fp32 sum in
another order.  ``rel_max`` / ``rel_l2`` are not used: d_time is one cancelling sum per channel, so they would measure its conditioning.

``routes`` restates the dispatch (csrc/dn_api.hip diffuse_route / to_basis_partials / from_basis / diffuse_fwd / diffuse_bwd, dn_tngemm.hip
tn_finish / dn_launch_tngemm, dn_pointwise.hip dn_launch_spec_fwd / dn_spec_bwd_fused_ok, dn_rowgemm.hip rg_finish / rg_dispatch_width,
dn_rowgemm_persist.hip pt_eligible / pt_launch, dn_diffuse.hip dn_diffuse_plan_host, dn_backproject_wide_ok) and ``check_case_table`` holds the
case table against it with no library loaded."""
import collections
import math

import torch

import helpers
from linear_cases import U, gamma, offset_copy

# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ------------------------------------------------------------------------------------------------------------------------------
Route = collections.namedtuple("Route", "proj_fwd proj_bwd spec_fwd spec_bwd bp_fwd bp_bwd")
FIELD_VALUES = {
    "proj_fwd": ("tngemm_x3", "tngemm_f32"), "proj_bwd": ("tngemm_x3", "tngemm_f32"), "spec_fwd": (4, 1), "spec_bwd": ("fused", "unfused"),
    "bp_fwd": ("wide", "direct", "pt_lockstep3", "pt_ws4_8", "pt_ws9", "rg32", "rg64", "rg128", "rg_unaligned"),
    "bp_bwd": ("direct", "pt_lockstep3", "pt_ws4_8", "pt_ws9", "rg32", "rg64", "rg128", "rg_unaligned"),
}
# the integer bounds of the dispatch by the name routes() knows them under.  plan_meshes: the plan is refused for n_mesh > n_cus + plan_meshes.
BOUNDS = {"direct_K": 128, "direct_C": 128, "wide_K": 256, "wide_C": 256, "plan_meshes": 0, "pt_n": 128, "pt_min": 3, "pt_max": 32,
          "ws_min": 4, "ws9": 9, "w32": 32, "w64": 64}
STEP = {"pt_n": 4, "w32": 4, "w64": 4, "direct_K": 32, "wide_K": 32, "direct_C": 4, "wide_C": 4}     # next to a `% 4` / `% 32` test
MODS = ("tn_k4", "tn_c4", "kc4", "bwd_c4", "rg_k32", "rg_c4")                                         # the divisibility tests
ALL = frozenset("xdt")      # operands a case may hand over 4 bytes off a 16-byte boundary: x, d_xd, time


def plan_ok(sizes, n_cus, bounds=BOUNDS):
    """dn_diffuse_plan_host refuses an empty mesh and more meshes than workgroups (its `sum > n_wg` loop cannot fail otherwise: every count it
    lowers is above 1 while the meshes are no more than the workgroups)."""
    return len(sizes) > 0 and all(v > 0 for v in sizes) and len(sizes) <= n_cus + bounds["plan_meshes"] and len(sizes) <= 4096


def _row_gemm(K, C, has_r0, store, bounds, off):
    """dn_launch_rowgemm for the back-projection (one segment of width K, B = the spectrum [K, C] per mesh): STORE or MASS_ADD."""
    aligned = (K % 32 == 0 or "rg_k32" in off) and (C % 4 == 0 or "rg_c4" in off)
    nsl = K // 32
    if aligned and C >= bounds["pt_n"] and C % 4 == 0 and bounds["pt_min"] <= nsl <= bounds["pt_max"] and (store or has_r0):
        return "pt_ws9" if nsl >= bounds["ws9"] else "pt_ws4_8" if nsl >= bounds["ws_min"] else "pt_lockstep3"
    if not aligned:
        return "rg_unaligned"
    return "rg32" if C <= bounds["w32"] else "rg64" if C <= bounds["w64"] else "rg128"


def routes(sizes, K, C, aligned=ALL, n_cus=256, diffuse_opt=2, has_add=False, bounds=BOUNDS, off=(), workspace=True):
    """The kernels one forward + backward call takes.  ``aligned``: which of x ("x"), d_xd ("d"), time ("t") sit on a 16-byte boundary (the
    library's own buffers always do).  ``bounds`` / ``off`` (divisibility tests switched off) exist for the table test.  ``workspace`` False:
    dn_from_basis_f32, which has none and therefore never takes the wide ring kernel."""
    tn = lambda al: "tngemm_x3" if (K % 4 == 0 or "tn_k4" in off) and (C % 4 == 0 or "tn_c4" in off) and al else "tngemm_f32"
    spec_fwd = 4 if (K * C) % 4 == 0 or "kc4" in off else 1
    spec_bwd = "fused" if (C % 4 == 0 or "bwd_c4" in off) and "t" in aligned else "unfused"
    direct = diffuse_opt != 0 and K == bounds["direct_K"] and C == bounds["direct_C"] and plan_ok(sizes, n_cus, bounds)
    wide = diffuse_opt != 0 and K == bounds["wide_K"] and C == bounds["wide_C"] and workspace      # (tile bound of the ring: beyond any test size)
    bp_fwd = "wide" if wide else "direct" if direct else _row_gemm(K, C, False, True, bounds, off)
    bp_bwd = "direct" if direct else _row_gemm(K, C, has_add, False, bounds, off)
    return Route(tn("x" in aligned), tn("d" in aligned), spec_fwd, spec_bwd, bp_fwd, bp_bwd)


# ------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "K C sizes diffuse mis add chunk_rows")
RAGGED = (1, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 200)
ONE = (700,)
PAIR, W2, W3, CH = (65, 129), (150, 37), (150, 37, 9), (1100, 40, 9)
MANY, FULL = ("n_cus+1", 3), ("n_cus", 3)          # that many meshes of three rows


def _c(K, C, sizes, diffuse=2, mis="", add=False, chunk_rows=None):
    return Case(K, C, sizes, diffuse, mis, add, chunk_rows)


CASES = (
    # direct back-projection: small and ragged meshes (one workgroup, under one MFMA unit, off the 16-row unit), one mesh over many workgroups;
    # two batches of three meshes so that the emulator's three workgroups see tiny meshes too
    [_c(128, 128, RAGGED), _c(128, 128, ONE), _c(128, 128, (5, 17, 129)), _c(128, 128, (1, 16, 63))]
    # the same on the row GEMM: forward 4-slice wave-specialised, backward (no add operand) the 128 tile
    + [_c(128, 128, RAGGED, 0), _c(128, 128, ONE, 0)]
    # MASS_ADD with an add operand: direct, and the persistent kernels in all three forms (pt_eligible wants r0)
    + [_c(128, 128, PAIR, 0, add=True), _c(128, 128, PAIR, 2, add=True)]
    + [_c(K, C, PAIR, add=True) for K, C in ((96, 128), (96, 132), (288, 128), (288, 132), (160, 192))]
    # more meshes than workgroups: the plan is refused and the row GEMM runs under diffuse = 2; as many as workgroups: one row tile each
    + [_c(128, 128, MANY), _c(128, 128, FULL)]
    # wide ring kernel (forward), backward on the 128 tile; under diffuse = 0 the forward has 8 slices
    + [_c(256, 256, (300, 257, 17)), _c(256, 256, (40, 130)), _c(256, 256, (300, 257, 17), 0)]
    # width classes, aligned: N <= 32; N <= 64; 128 tile; 3-slice lock-step; >= 9 slices; 2 x 2 split-V tiles + a partial column tile; a
    # persistent product with a partial column tile; then the widths next to each bound, and 32 / 33 slices
    + [_c(K, C, W2) for K, C in ((32, 32), (64, 64), (64, 128), (96, 128), (288, 128), (160, 192), (128, 132),
                                 (64, 32), (32, 36), (32, 68), (96, 124), (1024, 128), (1056, 128))]
    # exact-f32 and scalar forms: K % 32 != 0; C % 4 != 0 (exact tngemm, unfused spectral backward); spec_fwd<1>; K C % 4 = 0 with C % 4 != 0;
    # K % 4 != 0 with C % 4 = 0; K % 32 = 0 with C % 4 != 0
    + [_c(K, C, W3) for K, C in ((20, 32), (24, 40), (30, 33), (4, 3), (7, 5), (1, 1), (6, 8), (32, 33))]
    # operands 4 bytes off, in turn and together
    + [_c(K, C, PAIR, mis=m) for K, C in ((128, 128), (24, 40)) for m in ("x", "d", "t", "xdt")]
    # 35 chunks: more than the 32 chunk lanes of spec_bwd_fused and than the unrolled loop of seg_reduce_body; the others have 2 and 1
    + [_c(24, 40, CH, chunk_rows=32), _c(128, 128, CH, chunk_rows=32)]
)
# cases that dominate the emulator tier run on the device only: the three-mesh K = C = 256 batch (the two-mesh one stays) and 32 / 33 slices
EMU_SLOW_CASES = (_c(256, 256, (300, 257, 17)), _c(256, 256, (300, 257, 17), 0), _c(1024, 128, W2), _c(1056, 128, W2))
BASIS_CASES = [_c(128, 128, RAGGED), _c(30, 33, W3), _c(160, 192, W2)]


def case_id(c):
    sz = "x".join(map(str, c.sizes))
    return "K%d-C%d-%s-d%d%s%s%s" % (c.K, c.C, sz, c.diffuse, c.mis and "-mis_" + c.mis, "-add" if c.add else "", "-ch%d" % c.chunk_rows if c.chunk_rows else "")


def sizes_of(c, n_cus):
    if isinstance(c.sizes[0], str):
        return (c.sizes[1],) * (n_cus + (1 if c.sizes[0] == "n_cus+1" else 0))
    return tuple(c.sizes)


def case_route(c, n_cus, **moved):
    return routes(sizes_of(c, n_cus), c.K, c.C, ALL - set(c.mis), n_cus, c.diffuse, c.add, **moved)


def check_case_table(n_cus=256):
    """Every value of every field is reached at least twice; moving any bound by one step, switching off any divisibility test or
    realigning a misaligned operand changes the route of some case."""
    got = [case_route(c, n_cus) for c in CASES]
    assert len({case_id(c) for c in CASES}) == len(CASES)
    for field, values in FIELD_VALUES.items():
        for v in values:
            n = sum(getattr(r, field) == v for r in got)
            assert n >= 2, "%s = %s is reached by %d case(s)" % (field, v, n)
    noticed = lambda **moved: [c for c, r in zip(CASES, got) if case_route(c, n_cus, **moved) != r]
    for name, v in BOUNDS.items():
        for step in (-STEP.get(name, 1), STEP.get(name, 1)):
            assert noticed(bounds=dict(BOUNDS, **{name: v + step})), "no case notices %s = %d moved to %d" % (name, v, v + step)
    for m in MODS:
        assert noticed(off=(m,)), "no case notices the divisibility test %s" % m
    for op, fields in (("x", ("proj_fwd",)), ("d", ("proj_bwd",)), ("t", ("spec_bwd",))):
        hit = [c for c, r in zip(CASES, got) if op in c.mis and routes(sizes_of(c, n_cus), c.K, c.C, ALL, n_cus, c.diffuse, c.add) != r]
        assert len(hit) >= 2, "fall-through of a misaligned %s" % op
        for c in hit:
            r, r0 = case_route(c, n_cus), routes(sizes_of(c, n_cus), c.K, c.C, ALL - set(c.mis) | {op}, n_cus, c.diffuse, c.add)
            assert all(getattr(r, f) != getattr(r0, f) for f in fields)
    # dn_from_basis_f32 has no workspace: never wide
    assert routes((300,), 256, 256, workspace=False).bp_fwd == "pt_ws4_8" and routes((300,), 256, 256).bp_fwd == "wide"
    # the smallness targets: under 2000 rows, but for the many-mesh batches and the 35-chunk mesh
    for c in CASES:
        assert isinstance(c.sizes[0], str) or c.sizes == CH or sum(c.sizes) < 2000, c
    assert -(-CH[0] // 32) == 35 and -(-CH[1] // 32) == 2 and -(-CH[2] // 32) == 1
    # what each row of the table is there for
    r = lambda *a, **k: routes(*a, n_cus=n_cus, **k)
    assert r(RAGGED, 128, 128) == Route("tngemm_x3", "tngemm_x3", 4, "fused", *(("direct",) * 2 if n_cus >= len(RAGGED) else ("pt_ws4_8", "rg128")))
    assert r((5, 17, 129), 128, 128)[4:] == ("direct", "direct")
    assert r(RAGGED, 128, 128, diffuse_opt=0)[4:] == ("pt_ws4_8", "rg128") and r(PAIR, 128, 128, diffuse_opt=0, has_add=True).bp_bwd == "pt_ws4_8"
    assert r((3,) * (n_cus + 1), 128, 128)[4:] == ("pt_ws4_8", "rg128") and r((3,) * n_cus, 128, 128).bp_fwd == "direct"
    assert r((300, 257, 17), 256, 256)[4:] == ("wide", "rg128")
    assert [r(W2, K, C).bp_fwd for K, C in ((32, 32), (64, 64), (64, 128), (96, 128), (288, 128), (160, 192), (128, 132))] == \
        ["rg32", "rg64", "rg128", "pt_lockstep3", "pt_ws9", "pt_ws4_8", "pt_ws4_8"]
    assert r(W3, 24, 40) == Route("tngemm_x3", "tngemm_x3", 4, "fused", "rg_unaligned", "rg_unaligned")
    assert r(W3, 30, 33) == Route("tngemm_f32", "tngemm_f32", 1, "unfused", "rg_unaligned", "rg_unaligned")
    assert r(W3, 4, 3)[:4] == ("tngemm_f32", "tngemm_f32", 4, "unfused")


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def make_operators(sizes, K, seed, hard=True):
    """Per mesh: masses 10^(-6 U) (benign: within a factor 3), summing to 4 pi; Phi = Q / sqrt(m), Q with orthonormal columns (random Gaussian
    where V < K), so that Phi^T M Phi = I; lambda_0 = 0 and the rest sorted uniform up to 4 pi K (benign: 0.55 K)."""
    out = []
    for i, v in enumerate(sizes):
        g = torch.Generator().manual_seed(7919 * seed + i)
        u = torch.rand(v, generator=g, dtype=torch.float64)
        m = 10.0 ** (-6.0 * u) if hard else 1.0 + 2.0 * u
        m = m * (4.0 * math.pi / m.sum())
        q = torch.randn(v, K, generator=g, dtype=torch.float64)
        q = torch.linalg.qr(q)[0] if v >= K else q / v ** 0.5
        lam = torch.sort(torch.rand(K, generator=g, dtype=torch.float64))[0]
        lam[0] = 0.0
        if K > 1:
            lam = lam * ((4.0 * math.pi * K if hard else 0.55 * K) / lam[-1])
        out.append({"mass": m.float(), "evals": lam.float(), "evecs": (q / m.sqrt()[:, None]).float()})
    return out


def special_channels(C):
    """(zero channel of x, channel scaled by 2^20, channel scaled by 2^-20); None where the width has no room next to t_0 and t_1."""
    return (C - 1 if C >= 3 else None, C - 2 if C >= 5 else None, C - 3 if C >= 5 else None)


def make_features(rows, C, seed, hard=True):
    g = torch.Generator().manual_seed(104729 * seed + C)
    x, d = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    add = torch.randn(rows, C, generator=g)
    if not hard:
        return x, 0.01 + 0.3 * torch.rand(C, generator=g), d, add
    t = 10.0 ** (-8.0 * torch.rand(C, generator=g))          # log-uniform in [1e-8, 1]
    t[0] = 1e-8
    if C > 1:
        t[1] = 1.0
    zero, big, small = special_channels(C)
    if big is not None:
        x[:, big] *= 2.0 ** 20
        d[:, big] *= 2.0 ** 20
        x[:, small] *= 2.0 ** -20
        d[:, small] *= 2.0 ** -20
    if zero is not None:
        x[:, zero] = 0.0
    return x, t, d, add


def _offsets(sizes):
    offs = [0]
    for v in sizes:
        offs.append(offs[-1] + v)
    return offs


def evaluate(meshes, x, time, d_xd, add, dtype):
    """The formulas in torch at ``dtype``, gradients by autograd: {xs [n_mesh, K, C], xd, d_x (+ add), d_time}."""
    offs = _offsets([m["mass"].shape[0] for m in meshes])
    xr, tr = x.to(dtype).clone().requires_grad_(True), time.to(dtype).clone().requires_grad_(True)
    xs, xd = [], []
    for i, m in enumerate(meshes):
        phi, mass, lam = m["evecs"].to(dtype), m["mass"].to(dtype), m["evals"].to(dtype)
        s = phi.T @ (mass[:, None] * xr[offs[i]:offs[i + 1]])
        xs.append(s)
        xd.append(phi @ (torch.exp(-lam[:, None] * tr[None, :]) * s))
    xd = torch.cat(xd, 0)
    (xd * d_xd.to(dtype)).sum().backward()
    d_x = xr.grad if add is None else add.to(dtype) + xr.grad
    return {"xs": torch.stack(xs, 0).detach(), "xd": xd.detach(), "d_x": d_x, "d_time": tr.grad}


def scales(meshes, x, time, d_xd, add):
    """The reference expressions on absolute values, in fp64."""
    offs = _offsets([m["mass"].shape[0] for m in meshes])
    xa, da, t = x.double().abs(), d_xd.double().abs(), time.double()
    S = {"xs": [], "xd": [], "d_x": [], "d_time": torch.zeros(time.shape[0], dtype=torch.float64)}
    for i, m in enumerate(meshes):
        phi, mass, lam = m["evecs"].double().abs(), m["mass"].double(), m["evals"].double()
        coef = torch.exp(-lam[:, None] * t[None, :])
        sxs = phi.T @ (mass[:, None] * xa[offs[i]:offs[i + 1]])
        sd = phi.T @ da[offs[i]:offs[i + 1]]
        S["xs"].append(sxs)
        S["xd"].append(phi @ (coef * sxs))
        S["d_x"].append(mass[:, None] * (phi @ (coef * sd)))
        S["d_time"] += (lam[:, None] * coef * sd * sxs).sum(0)
    S["xs"], S["xd"], S["d_x"] = torch.stack(S["xs"], 0), torch.cat(S["xd"], 0), torch.cat(S["d_x"], 0)
    if add is not None:
        S["d_x"] = S["d_x"] + add.double().abs()
    return S


E3 = 4       # a 3-term split-bf16 product, per term and relative to |a||b|: the two operands' 24-bit pieces (2 u) and the dropped mid*lo, lo*mid (2 u)
EXP = 4      # exp(-lambda t) ys: the rounded product lambda t moves the result by lambda t e^(-lambda t) u <= 0.37 u relative to S (1), expf (2), the product (1)
NAMES = ("xs", "xd", "d_x", "d_time")


def counts(sizes, chunk_rows, K, has_add=False):
    """n of gamma_n per quantity.  Projection: the rows of the largest mesh, its chunk partials, the 8 lane sums."""
    per = chunk_rows if isinstance(chunk_rows, (list, tuple)) else [chunk_rows] * len(sizes)
    proj = max(sizes) + max(-(-v // c) for v, c in zip(sizes, per)) + 8
    n_xs = proj + 1 + E3                                    # + the mass product
    n_dys = proj + E3
    return {"xs": n_xs, "xd": n_xs + EXP + K + E3, "d_x": n_dys + EXP + K + E3 + 1 + (1 if has_add else 0),
            "d_time": n_dys + n_xs + EXP + 1 + K + len(sizes) + 8}      # + the lambda product, K terms per mesh in groups of 8, the meshes


def scaled_err(got, ref, scale, what=""):
    """max |got - ref| / S; where S = 0 the result must be exactly 0."""
    got, zero = got.detach().cpu().double(), scale == 0
    assert bool((got[zero] == 0).all()), "%s: non-zero where the reference expression on absolute values is 0" % what
    if bool(zero.all()):
        return 0.0
    return float(((got - ref).abs()[~zero] / scale[~zero]).max())


_INPUTS = {}


def inputs(sizes, K, C, hard, add):
    """Operators, features, the fp64 reference, S and torch's fp32 evaluation, computed once per shape and left unchanged."""
    key = (tuple(sizes), K, C, hard, add)
    if key not in _INPUTS:
        seed = 1000 * K + C + sum(sizes) % 997
        meshes = make_operators(sizes, K, seed, hard)
        x, t, d, a = make_features(sum(sizes), C, seed, hard)
        a = a if add else None
        ref, S = evaluate(meshes, x, t, d, a, torch.float64), scales(meshes, x, t, d, a)
        t32 = evaluate(meshes, x, t, d, a, torch.float32)
        s32 = {n: scaled_err(t32[n], ref[n], S[n], "torch fp32 " + n) for n in NAMES}
        _INPUTS[key] = (meshes, x, t, d, a, ref, S, s32)
    return _INPUTS[key]


# ------------------------------------------------------------------------------------------------------------------------------
# calls
# ------------------------------------------------------------------------------------------------------------------------------
def n_cus_of():
    from diffusion_net import _hip
    return int(_hip.lib().dn_diffusion_plan_wgs())


def pack(meshes, dev, chunk_rows=None):
    from diffusion_net.batch import MeshBatch
    return MeshBatch.from_operators([m["mass"] for m in meshes], [m["evals"] for m in meshes], [m["evecs"] for m in meshes], None, None,
                                    device=dev, chunk_rows=chunk_rows)


def _ws_for(mb, C, ws):
    from diffusion_net import _hip, ops
    return ops._ws(mb, _hip.lib().dn_diffusion_workspace_bytes(mb.ref(), C)) if ws is None else ws


def raw_fwd(mb, x, time, ws=None):
    """dn_diffusion_fwd_f32 on the operands as they are (no copy: a misaligned view stays misaligned) -> xs, xd."""
    from diffusion_net import _hip
    C = x.shape[1]
    assert x.is_contiguous() and time.is_contiguous()
    xs = torch.empty(mb.n_mesh, mb.k_eig, C, dtype=torch.float32, device=x.device)
    xd = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    w, n = _ws_for(mb, C, ws)
    _hip.check(_hip.lib().dn_diffusion_fwd_f32(mb.ref(), x.data_ptr(), time.data_ptr(), C, xs.data_ptr(), xd.data_ptr(), w.data_ptr(), n,
                                               _hip.stream_of(x)), "dn_diffusion_fwd_f32")
    return xs, xd


def raw_bwd(mb, d_xd, xs, time, add=None, ws=None):
    """dn_diffusion_bwd_f32 -> d_x (= add + ...), d_time."""
    from diffusion_net import _hip
    C = d_xd.shape[1]
    assert d_xd.is_contiguous() and xs.is_contiguous() and time.is_contiguous()
    d_x = torch.empty(d_xd.shape, dtype=torch.float32, device=d_xd.device)
    d_t = torch.empty(C, dtype=torch.float32, device=d_xd.device)
    w, n = _ws_for(mb, C, ws)
    _hip.check(_hip.lib().dn_diffusion_bwd_f32(mb.ref(), d_xd.data_ptr(), xs.data_ptr(), time.data_ptr(), C, None if add is None else add.data_ptr(),
                                               d_x.data_ptr(), d_t.data_ptr(), w.data_ptr(), n, _hip.stream_of(d_xd)), "dn_diffusion_bwd_f32")
    return d_x, d_t


def call_op(dev, mb, x, time, d_xd, add=None, mis=""):
    """One forward and one backward.  Aligned operands without an add go through ``ops.DiffusionFn`` and autograd (the saved xs is the node's);
    the others through the C entry points."""
    place = lambda t, m: offset_copy(t, dev) if m in mis else t.to(dev)
    if not mis and add is None:
        from diffusion_net import ops
        xi, ti = x.clone().to(dev).requires_grad_(True), time.clone().to(dev).requires_grad_(True)
        xd = ops.DiffusionFn.apply(xi, ti, mb)
        xs = xd.grad_fn.saved_tensors[0]
        xd.backward(d_xd.to(dev))
        return {"xs": xs.detach(), "xd": xd.detach(), "d_x": xi.grad, "d_time": ti.grad}
    xi, ti, di = place(x, "x"), place(time, "t"), place(d_xd, "d")
    xs, xd = raw_fwd(mb, xi, ti)
    d_x, d_t = raw_bwd(mb, di, xs, ti, None if add is None else add.to(dev))
    return {"xs": xs, "xd": xd, "d_x": d_x, "d_time": d_t}


def judge(got, ref, S, s32, n, label):
    """Prints every figure, then (a) and (b) for each quantity present in ``got``.  -> ({name: s / u}, failures)"""
    rec, failures = {}, []
    for name in NAMES:
        if name not in got:
            continue
        assert gamma(n[name]) >= s32[name], "torch's fp32 evaluation misses gamma_%d on %s (%.3g u): the count is wrong" % (n[name], name, s32[name] / U)
        s = scaled_err(got[name], ref[name], S[name], label + " " + name)
        rec[name] = s / U
        print("diffusion %s %s: s = %.2f u, torch fp32 %.2f u, gamma_n %.1f u" % (label, name, s / U, s32[name] / U, gamma(n[name]) / U))
        if not s <= gamma(n[name]):
            failures.append("(a) %s: s = %.3g u above gamma_%d" % (name, s / U, n[name]))
        elif not s <= 4 * max(s32[name], 2 * U):
            failures.append("(b) %s: s = %.3g u above 4 x max(torch fp32 %.3g u, 2 u)" % (name, s / U, s32[name] / U))
    return rec, failures


def with_option(name, value, fn):
    from diffusion_net import _hip
    saved = _hip.get_option(name)
    try:
        _hip.set_option(name, value)
        return fn()
    finally:
        _hip.set_option(name, saved)


def run_case(dev, c):
    n_cus = n_cus_of()
    sizes = sizes_of(c, n_cus)
    route = case_route(c, n_cus)
    rec, failures = {}, []
    for hard in (True, False):
        meshes, x, t, d, a, ref, S, s32 = inputs(sizes, c.K, c.C, hard, c.add)
        mb = pack(meshes, dev, c.chunk_rows)
        if c.K == 128:      # the plan is made or refused as restated
            assert (mb.df_plan is not None and mb._struct.df_n_groups == 1) == plan_ok(sizes, n_cus), "plan %s" % (mb.df_plan is not None)
        n = counts(sizes, mb.chunk_rows, c.K, c.add)
        got = with_option("diffuse", c.diffuse, lambda: call_op(dev, mb, x, t, d, a, c.mis))
        tag = "hard" if hard else "benign"
        r, f = judge(got, ref, S, s32, n, "%s %s" % (case_id(c), tag))
        failures += ["%s %s" % (tag, m) for m in f]
        for name in NAMES:
            rec["s_%s%s" % (name, "" if hard else "_benign")] = r[name]
            rec["s_torch32_%s%s" % (name, "" if hard else "_benign")] = s32[name] / U
        if hard:
            rec["n"] = [n[name] for name in NAMES]
        if route.bp_fwd in ("direct", "wide"):
            # the route must have run: not bitwise the row GEMM's result, and as close to it as two results that each meet (b) are
            xd0 = with_option("diffuse", 0, lambda: raw_fwd(mb, x.to(dev), t.to(dev))[1])
            assert not torch.equal(xd0, got["xd"]), "%s and row-GEMM back-projection are bitwise equal: the %s kernel did not run" % (route.bp_fwd,) * 2
            gap = scaled_err(got["xd"], xd0.cpu().double(), S["xd"], "xd")
            if not gap <= 8 * max(s32["xd"], 2 * U):
                failures.append("%s xd: %.3g u from the row GEMM's" % (tag, gap / U))
    helpers.record_margin("diffusion_ops", dev, id=case_id(c), K=c.K, C=c.C, sizes=list(sizes) if len(sizes) <= 16 else [len(sizes), sizes[0]],
                          route=list(route), unit="2^-24", **rec)
    assert not failures, failures


def run_basis(dev, c):
    """ToBasisFn and FromBasisFn alone, forward and backward, hard inputs.  (FromBasisFn has no workspace: at K = C = 256 it would not be wide.)"""
    from diffusion_net import ops
    sizes = sizes_of(c, n_cus_of())
    meshes, x, t, d, _, _, _, _ = inputs(sizes, c.K, c.C, True, False)
    mb = pack(meshes, dev, c.chunk_rows)
    offs = _offsets(sizes)
    g = torch.Generator().manual_seed(5)
    spec, d_spec = torch.randn(len(sizes), c.K, c.C, generator=g), torch.randn(len(sizes), c.K, c.C, generator=g)

    def ev(dtype, absolute):
        f = (lambda v: v.to(dtype).abs()) if absolute else (lambda v: v.to(dtype))
        phis, ms = [f(m["evecs"]) for m in meshes], [m["mass"].to(dtype) for m in meshes]
        rows = lambda v, i: f(v)[offs[i]:offs[i + 1]]
        return {"to_fwd": torch.stack([p.T @ (m[:, None] * rows(x, i)) for i, (p, m) in enumerate(zip(phis, ms))], 0),
                "to_bwd": torch.cat([m[:, None] * (p @ f(d_spec)[i]) for i, (p, m) in enumerate(zip(phis, ms))], 0),
                "from_fwd": torch.cat([p @ f(spec)[i] for i, p in enumerate(phis)], 0),
                "from_bwd": torch.stack([p.T @ rows(d, i) for i, p in enumerate(phis)], 0)}

    ref, S, t32 = ev(torch.float64, False), ev(torch.float64, True), ev(torch.float32, False)
    xi, si = x.clone().to(dev).requires_grad_(True), spec.clone().to(dev).requires_grad_(True)
    to = ops.ToBasisFn.apply(xi, mb)
    to.backward(d_spec.to(dev))
    fr = ops.FromBasisFn.apply(si, mb)
    fr.backward(d.to(dev))
    got = {"to_fwd": to.detach(), "to_bwd": xi.grad, "from_fwd": fr.detach(), "from_bwd": si.grad}
    cn = counts(sizes, mb.chunk_rows, c.K)
    n = {"to_fwd": cn["xs"], "to_bwd": c.K + E3 + 1, "from_fwd": c.K + E3, "from_bwd": cn["xs"] - 1}
    failures = []
    for name in got:
        s32 = scaled_err(t32[name], ref[name], S[name], name)
        assert gamma(n[name]) >= s32
        s = scaled_err(got[name], ref[name], S[name], name)
        print("basis %s %s: s = %.2f u, torch fp32 %.2f u, gamma_n %.1f u" % (case_id(c), name, s / U, s32 / U, gamma(n[name]) / U))
        if not (s <= gamma(n[name]) and s <= 4 * max(s32, 2 * U)):
            failures.append("%s: s = %.3g u, torch fp32 %.3g u, gamma_%d" % (name, s / U, s32 / U, n[name]))
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------------
# contracts beyond accuracy.  Each at (128, 128) on the direct route and at (24, 40).
# ------------------------------------------------------------------------------------------------------------------------------
CONTRACT_WIDTHS = [(128, 128), (24, 40)]
POISON_ROWS = {"first_in_chunk": 32, "last_in_chunk": 63, "last_in_mesh": 64}      # mesh 0 of PAIR in 32-row chunks: 32, 32, 1 rows
POISON_C = 5


def _raw_both(dev, mb, x, t, d):
    xs, xd = raw_fwd(mb, x.to(dev), t.to(dev))
    d_x, d_t = raw_bwd(mb, d.to(dev), xs, t.to(dev))
    return {"xs": xs.cpu(), "xd": xd.cpu(), "d_x": d_x.cpu(), "d_time": d_t.cpu()}


def _same(a, b):
    """bitwise, NaN payloads included"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_nonfinite(dev, K, C, where, value):
    """A NaN / +inf in one element x[r, c] of mesh 0 stays in channel c of mesh 0; a NaN in time[c] stays in channel c.  The poisoned row is
    first in its chunk, last in its chunk or last in its mesh: the aligned split-V loads clamp a chunk's tail rows to its first row and
    multiply by 0."""
    meshes, x, t, d, _, _, _, _ = inputs(PAIR, K, C, True, False)
    mb = pack(meshes, dev, 32)
    assert routes(PAIR, K, C, n_cus=n_cus_of()).bp_fwd == ("direct" if K == 128 else "rg_unaligned")
    clean = _raw_both(dev, mb, x, t, d)
    others = [ch for ch in range(C) if ch != POISON_C]
    v0 = PAIR[0]
    if where == "time":
        tp = t.clone()
        tp[POISON_C] = value
        got = _raw_both(dev, mb, x, tp, d)
        assert _same(got["xs"], clean["xs"])
        for name in ("xd", "d_x"):
            assert _same(got[name][:, others], clean[name][:, others]), name
            assert bool(torch.isnan(got[name][:, POISON_C]).all()), name
    else:
        xp = x.clone()
        xp[POISON_ROWS[where], POISON_C] = value
        got = _raw_both(dev, mb, xp, t, d)
        assert _same(got["xs"][1], clean["xs"][1]) and _same(got["xd"][v0:], clean["xd"][v0:]), "mesh 1 is touched"
        assert _same(got["xs"][0][:, others], clean["xs"][0][:, others]) and _same(got["xd"][:v0, others], clean["xd"][:v0, others]), "another channel of mesh 0"
        assert _same(got["d_x"][v0:], clean["d_x"][v0:]), "d_x of mesh 1"
        assert not bool(torch.isfinite(got["xs"][0][:, POISON_C]).all()), "the poison left no trace"
    assert _same(got["d_time"][others], clean["d_time"][others]), "d_time of another channel"
    assert not bool(torch.isfinite(got["d_time"][POISON_C]))


def spectrum_of(mb, C, ws):
    """The scaled spectrum ys the forward left in its workspace: the second region of diffuse_layout (csrc/dn_api.hip), each region rounded up
    to 256 bytes, the first one starting at the next 256-byte boundary."""
    kc = mb.k_eig * C
    start = (-ws.data_ptr()) % 256 + (mb._struct.n_chunks * kc * 4 + 255) // 256 * 256
    return ws[start:start + mb.n_mesh * kc * 4].view(torch.float32).view(mb.n_mesh, mb.k_eig, C).cpu()


def run_underflow(dev, K, C):
    """t = 1 in every channel (features randn): every ys[k, c] with lambda_k > 104 is 0 or denormal (e^-104 is below half the smallest
    denormal), nothing is NaN and xd, d_x, d_time meet (a) and (b).  t = 1e-8, the clamp floor: ys is xs e^(-lambda t) to within
    (lambda t + 2) u |xs| -- the rounded argument, expf and the product -- and so equals xs to that plus lambda t |xs|."""
    from diffusion_net import _hip
    sizes = PAIR
    meshes = inputs(sizes, K, C, True, False)[0]
    mb = pack(meshes, dev)
    x, _, d, _ = make_features(sum(sizes), C, 31, hard=False)
    lam = torch.stack([m["evals"] for m in meshes], 0).double()
    nbytes = int(_hip.lib().dn_diffusion_workspace_bytes(mb.ref(), C))
    for tv in (1.0, 1e-8):
        t = torch.full((C,), tv)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        xs, xd = raw_fwd(mb, x.to(dev), t.to(dev), (ws, nbytes))
        ys = spectrum_of(mb, C, ws).double()
        d_x, d_t = raw_bwd(mb, d.to(dev), xs, t.to(dev))
        got = {"xs": xs, "xd": xd, "d_x": d_x, "d_time": d_t}
        assert all(bool(torch.isfinite(v).all()) for v in got.values()) and bool(torch.isfinite(ys).all())
        if tv == 1.0:
            deep = (lam > 104.0)[:, :, None].expand_as(ys)
            assert int(deep.sum()) > 0 or K < 16
            assert bool((ys[deep].abs() < 2.0 ** -126).all()), "a coefficient e^(-lambda), lambda > 104, that is neither 0 nor denormal"
        else:
            tf = float(torch.tensor(tv, dtype=torch.float32))
            bound = (lam[:, :, None] * tf + 2.0) * U * xs.cpu().double().abs()
            exact = xs.cpu().double() * torch.exp(-lam[:, :, None] * tf)
            print("t = 1e-8: worst |ys - xs e^(-lambda t)| / ((lambda t + 2) u |xs|) = %.3f" % float(((ys - exact).abs() / bound.clamp_min(1e-300)).max()))
            assert bool(((ys - exact).abs() <= bound).all()), "ys is off xs e^(-lambda t) by more than (lambda t + 2) u |xs| at t = 1e-8"
        ref, S = evaluate(meshes, x, t, d, None, torch.float64), scales(meshes, x, t, d, None)
        t32 = evaluate(meshes, x, t, d, None, torch.float32)
        s32 = {n: scaled_err(t32[n], ref[n], S[n], n) for n in NAMES}
        _, failures = judge(got, ref, S, s32, counts(sizes, mb.chunk_rows, K), "underflow K%d C%d t=%g" % (K, C, tv))
        assert not failures, failures


def run_determinism(dev, K, C):
    """Two calls are bitwise equal in all four results; a third too, after a call of another shape has used the workspace."""
    meshes, x, t, d, _, _, _, _ = inputs(PAIR, K, C, True, False)
    mb = pack(meshes, dev, 32)
    a, b = _raw_both(dev, mb, x, t, d), _raw_both(dev, mb, x, t, d)
    om, ox, ot, od = inputs(W3, 30, 33, True, False)[:4]
    _raw_both(dev, pack(om, dev), ox, ot, od)
    c = _raw_both(dev, mb, x, t, d)
    for name in NAMES:
        assert _same(a[name], b[name]) and _same(a[name], c[name]), name


WORKSPACE_CASES = [_c(24, 40, CH, chunk_rows=32), _c(128, 128, CH, chunk_rows=32), _c(256, 256, (300, 257, 17))]


def run_exact_workspace(dev, c):
    """A raw forward and a raw backward inside exactly ``dn_diffusion_workspace_bytes`` bytes, 16 bytes past a 256-byte boundary; the guard
    floats on both sides keep their fill and the results are right."""
    from diffusion_net import _hip
    meshes, x, t, d, _, ref, S, s32 = inputs(c.sizes, c.K, c.C, True, False)
    mb = pack(meshes, dev, c.chunk_rows)
    need = int(_hip.lib().dn_diffusion_workspace_bytes(mb.ref(), c.C))
    assert need % 4 == 0
    guard = 1 << 16
    buf = torch.full((need // 4 + 2 * guard + 64,), -7.0, dtype=torch.float32, device=dev)
    lo = guard + ((16 - buf[guard:].data_ptr()) % 256) // 4
    ws = buf[lo:lo + need // 4]
    assert ws.data_ptr() % 256 == 16
    xs, xd = raw_fwd(mb, x.to(dev), t.to(dev), (ws, need))
    d_x, d_t = raw_bwd(mb, d.to(dev), xs, t.to(dev), None, (ws, need))
    assert bool((buf[:lo] == -7.0).all()) and bool((buf[lo + need // 4:] == -7.0).all()), "a store outside the workspace"
    _, failures = judge({"xs": xs, "xd": xd, "d_x": d_x, "d_time": d_t}, ref, S, s32, counts(c.sizes, mb.chunk_rows, c.K), "workspace " + case_id(c))
    assert not failures, failures

"""Shared bodies of the irregular-sparsity tests (drivers: test_sparse_emu.py on the emulator build, test_sparse_gpu.py on the device): every
kernel that walks the CSR pattern of gradX / gradY -- ``spmm_kernel`` in each instantiation the launcher can choose, the gathers of the chained
forward, ``sg_grad_kernel``, the packing and the norm word -- on an operator whose rows are NOT all the same length.

The operator (``make_irregular``): mass / evals / evecs of ``synthetic.make_mesh_operators``, gradX / gradY on one shared pattern with row lengths
from LENS (the multiples of DN_SP_CHUNK = 8 and DN_CH_GCHUNK = 4, plus and minus one), empty first rows, a long row alone among the empty rows of
its wave, a whole empty block, a long last row, a hub column, a column nobody references, explicit zeros.

Criterion of the isolated gathers: the condition-scaled error  s = max |got - ref| / (|G| |x|)  against the dense fp64 product built from the COO
entries, element by element.  A chain of n fmaf terms in any order obeys s <= gamma_n = n u / (1 - n u), u = 2^-24; the tests allow gamma_(n + 2),
n the number of fmaf terms of the longest row (two per entry in the two-operand backward, one more for ``add``).  Where |G||x| = 0 -- an empty
row -- the result must be exactly the reference."""
import contextlib

import numpy as np
import torch

import helpers
import parity_cases
from linear_cases import U, gamma, offset_copy
from parity_cases import FWD_TOL, GRAD_TOL, pack

LENS = (0, 1, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 33, 40)
SIZES = (150, 131)            # no multiple of 16; 281 rows: 9 row blocks of 32 (C = 32), 141 of 2 (C = 128) -- no multiple of 8
SIZES_WIDE = (260, 257)       # K = 256 needs 256 rows per mesh
HUB, UNUSED = 5, 7            # per mesh: the column every odd non-empty row references, the column no row references
LONE = (16, 32, 21, 40)       # mesh 0: rows [16, 32) are empty but row 21, which holds 40 entries -- alone in its 8-row wave (C = 32), beside an
                              # empty row in its 2-row wave (C = 128), alone in a 16-row half of the chained kernel
EMPTY_RUN = (64, 104)         # mesh 0: 40 empty rows, the 32-row block [64, 96) among them
LAST_LEN = 33                 # the batch's last row


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the operator
# ------------------------------------------------------------------------------------------------------------------------------
def row_lengths(V, seed, first, last):
    rng = np.random.RandomState(seed)
    lens = rng.permutation(np.resize(np.array(LENS), V))
    if first:
        lens[:2] = 0
        lens[LONE[0]:LONE[1]] = 0
        lens[LONE[2]] = LONE[3]
        lens[EMPTY_RUN[0]:EMPTY_RUN[1]] = 0
    if last:
        lens[V - 1] = LAST_LEN
    return lens


def irregular_operator(V, seed, first=False, last=False):
    """-> (gradX, gradY) sparse COO [V, V], coalesced, one pattern."""
    rng = np.random.RandomState(seed + 7919)
    lens = row_lengths(V, seed, first, last)
    others = np.array([c for c in range(V) if c not in (HUB, UNUSED)])
    rows, cols = [], []
    for r, n in enumerate(lens):
        if n == 0:
            continue
        if r % 2:
            c = np.concatenate([[HUB], rng.choice(others, n - 1, replace=False)])
        else:
            c = rng.choice(others, n, replace=False)
        rows.append(np.full(n, r, dtype=np.int64))
        cols.append(np.sort(c).astype(np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    nnz = rows.shape[0]
    vx, vy = (0.1 * V ** 0.5 * rng.randn(nnz) for _ in range(2))
    k = np.arange(nnz)
    vx[k % 11 == 3] = 0.0          # explicit zeros: in one operator, in the other, in both
    vy[k % 13 == 5] = 0.0
    vx[k % 17 == 9] = 0.0
    vy[k % 17 == 9] = 0.0
    idx = torch.from_numpy(np.stack([rows, cols], 0))
    mk = lambda v: torch.sparse_coo_tensor(idx, torch.from_numpy(v).to(torch.float32), (V, V)).coalesce()
    return mk(vx), mk(vy)


_plain_make_ragged = parity_cases.make_ragged


def make_irregular(sizes, K, C_in, seed=0):
    """``parity_cases.make_ragged`` with the gradient operators replaced."""
    return _make_irregular(_plain_make_ragged, sizes, K, C_in, seed)


def _make_irregular(plain, sizes, K, C_in, seed):
    meshes, feats = plain(sizes, K, C_in, seed)
    for i, m in enumerate(meshes):
        m["gradX"], m["gradY"] = irregular_operator(int(m["mass"].shape[0]), seed + 100 + i, first=i == 0, last=i == len(meshes) - 1)
    return meshes, feats


def global_coo(meshes):
    """(rows, cols, vx, vy) of the whole batch, numpy, coalesced order -- what ``MeshBatch.from_operators`` hands to ``coo_to_csr``."""
    off, out = 0, []
    for m in meshes:
        i, a, b = m["gradX"].indices().numpy(), m["gradX"].values().numpy(), m["gradY"].values().numpy()
        assert np.array_equal(i, m["gradY"].indices().numpy())
        out.append((i[0] + off, i[1] + off, a, b))
        off += int(m["mass"].shape[0])
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


def check_operator(sizes=SIZES):
    """The generator places what the tests rely on (no library)."""
    meshes, _ = make_irregular(sizes, 8, 3, seed=1)
    rows, cols, vx, vy = global_coo(meshes)
    vt = sum(sizes)
    lens, tlens = np.bincount(rows, minlength=vt), np.bincount(cols, minlength=vt)
    assert set(lens.tolist()) == set(LENS), sorted(set(LENS) ^ set(lens.tolist()))
    assert lens[0] == 0 and lens[1] == 0 and lens[vt - 1] == LAST_LEN
    lone = lens[LONE[0]:LONE[1]]
    assert lone[LONE[2] - LONE[0]] == LONE[3] and lone.sum() == LONE[3] and LONE[0] % 16 == 0 and LONE[1] - LONE[0] == 16
    assert not lens[EMPTY_RUN[0]:EMPTY_RUN[1]].any() and EMPTY_RUN[0] % 32 == 0 and EMPTY_RUN[1] - EMPTY_RUN[0] >= 32
    off = 0
    for v in sizes:
        assert v % 16 != 0
        assert tlens[off + UNUSED] == 0
        off += v
    assert tlens[off - sizes[-1] + HUB] >= 0.4 * sizes[-1], "the hub of the last mesh"      # a transposed row of about V / 2 entries
    assert tlens.max() > 40 and (tlens == 0).any()
    for C in (32, 128):
        rpb = 256 // spmm_route(C, True)[1]
        assert -(-vt // rpb) % 8 != 0
    assert (vx == 0).sum() > 10 and (vy == 0).sum() > 10 and ((vx == 0) & (vy == 0)).sum() > 5
    assert np.all(np.diff(rows) >= 0) and np.all((np.diff(cols) > 0) | (np.diff(rows) > 0)), "coalesced order"


def dense64(meshes):
    """Block-diagonal dense fp64 (gradX, gradY, pattern) of the batch, from the COO entries."""
    rows, cols, vx, vy = global_coo(meshes)
    vt = sum(int(m["mass"].shape[0]) for m in meshes)
    r, c = torch.from_numpy(rows), torch.from_numpy(cols)
    out = []
    for v in (vx, vy, np.ones_like(vx)):
        d = torch.zeros(vt, vt, dtype=torch.float64)
        d.index_put_((r, c), torch.from_numpy(v).double(), accumulate=True)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the isolated gathers, every instantiation of spmm_kernel
# ------------------------------------------------------------------------------------------------------------------------------
SP_CHUNK = 8


def spmm_route(C, aligned):
    """dn_launch_spmm / spmm_kernel restated -> (vec, tpr, coop, passes): float4 lanes; lanes per row; pattern entries fetched once per row and
    shared by shuffles (device build only); trips of the column loop."""
    vec = C % 4 == 0 and aligned
    tpr = 1
    while tpr < ((C + 3) // 4 if vec else C):
        tpr *= 2
    tpr = min(tpr, 256)
    span = tpr * (4 if vec else 1)
    return vec, tpr, SP_CHUNK <= tpr <= 64 and C % span == 0, -(-C // span)


def instantiation(C, aligned):
    vec, tpr, coop, passes = spmm_route(C, aligned)
    if passes > 1:
        return "passes"
    if not vec:
        return "scalar_coop" if coop else "scalar"
    if tpr < SP_CHUNK:
        return "vec_narrow"
    if tpr > 64:
        return "vec_wide"
    return "vec_coop_%d" % tpr if coop else "vec_ragged"


# (C, misaligned): misaligned operands sit 4 bytes past a 16-byte boundary, which turns the float4 form off
CASES = [(1, False), (5, False), (8, True), (32, True), (8, False), (16, False), (32, False), (64, False), (128, False), (256, False),
         (40, False), (512, False), (1028, False)]
INSTANTIATIONS = ("scalar", "scalar_coop", "vec_narrow", "vec_coop_8", "vec_coop_16", "vec_coop_32", "vec_coop_64", "vec_ragged", "vec_wide", "passes")
EMU_SKIPS_COOP = "DN_SP_COOP is compiled out of the emulator build: there these cases run the every-lane-loads form"


def check_case_table():
    """Every instantiation has a case, so removing a sole representative fails here; the widths the launcher's tests turn on are present."""
    got = [instantiation(C, not mis) for C, mis in CASES]
    for name in INSTANTIATIONS:
        assert name in got, "no case reaches the %s instantiation" % name
    assert set(got) <= set(INSTANTIATIONS), set(got) - set(INSTANTIATIONS)
    assert spmm_route(1, True) == (False, 1, False, 1) and spmm_route(5, True) == (False, 8, False, 1)
    assert spmm_route(8, False) == (False, 8, True, 1) and spmm_route(32, False) == (False, 32, True, 1)
    assert spmm_route(8, True)[:3] == (True, 2, False) and spmm_route(16, True)[:3] == (True, 4, False)
    assert [spmm_route(C, True)[1:3] for C in (32, 64, 128, 256)] == [(8, True), (16, True), (32, True), (64, True)]
    assert spmm_route(40, True) == (True, 16, False, 1) and spmm_route(512, True) == (True, 128, False, 1)
    assert spmm_route(1028, True) == (True, 256, False, 2)


_CACHE = {}


def irregular_batch(dev, sizes=SIZES, K=8, seed=1):
    """(meshes, packed batch, (gradX, gradY, pattern) dense fp64) -- built once per device and shape, never modified."""
    key = (str(dev), tuple(sizes), K, seed)
    if key not in _CACHE:
        meshes, _ = make_irregular(sizes, K, 3, seed)
        _CACHE[key] = (meshes, pack(meshes, dev, chunk_rows=64), dense64(meshes))
    return _CACHE[key]


def scaled(got, ref, scale):
    """max |got - ref| / scale; where scale = 0 (an empty row: nothing is summed) any difference counts as infinite."""
    err = (got.detach().cpu().double() - ref).abs()
    s = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(s.max())


def place(t, dev, mis):
    return offset_copy(t, dev) if mis else t.to(dev).contiguous()


def run_case(dev, C, mis):
    from diffusion_net import _hip, ops
    meshes, mb, (GX, GY, P) = irregular_batch(dev)
    vt = mb.v_total
    g = torch.Generator().manual_seed(7000 + C)
    x, w1, w2, add = (torch.randn(vt, C, generator=g) for _ in range(4))
    x6, w16, w26, a6 = x.double(), w1.double(), w2.double(), add.double()
    n_f, n_b = int(P.sum(1).max()), int(P.sum(0).max())          # entries of the longest row, of the longest transposed row
    L, st = _hip.lib(), _hip.stream_of(mb.mass)
    res, fails = {}, []

    def judge(name, got, ref, scale, n):
        s = scaled(got, ref, scale)
        res["s_" + name], res["gamma_" + name] = s / U, gamma(n + 2) / U
        print("sparse C=%d%s %s: s = %.2f u, gamma_%d = %.1f u" % (C, " misaligned" if mis else "", name, s / U, n + 2, gamma(n + 2) / U))
        if not s <= gamma(n + 2):
            fails.append("%s: s = %.4g u above gamma_%d = %.4g u" % (name, s / U, n + 2, gamma(n + 2) / U))

    # ops.GradApplyFn, forward and backward (the backward's operands are autograd's: aligned)
    xa = place(x, dev, mis).detach().requires_grad_(True)
    gx, gy = ops.GradApplyFn.apply(xa, mb)
    (gx * w1.to(dev) + gy * w2.to(dev)).sum().backward()
    judge("gx", gx, GX @ x6, GX.abs() @ x6.abs(), n_f)
    judge("gy", gy, GY @ x6, GY.abs() @ x6.abs(), n_f)
    ref_b, scale_b = GX.T @ w16 + GY.T @ w26, GX.T.abs() @ w16.abs() + GY.T.abs() @ w26.abs()
    judge("d_x", xa.grad, ref_b, scale_b, 2 * n_b)
    # dn_grad_apply_bwd_f32 with ``add``: into a separate output, then in place (add == d_x, the call of dn_block_bwd_f32)
    dgx, dgy = place(w1, dev, mis), place(w2, dev, mis)
    out = place(torch.full((vt, C), float("nan")), dev, mis)
    addd = place(add, dev, mis)
    _hip.check(L.dn_grad_apply_bwd_f32(mb.ref(), dgx.data_ptr(), dgy.data_ptr(), addd.data_ptr(), C, out.data_ptr(), st), "dn_grad_apply_bwd_f32")
    judge("d_x_add", out, ref_b + a6, scale_b + a6.abs(), 2 * n_b + 1)
    assert torch.equal(addd.cpu(), add), "the backward wrote to its ``add`` operand"
    _hip.check(L.dn_grad_apply_bwd_f32(mb.ref(), dgx.data_ptr(), dgy.data_ptr(), addd.data_ptr(), C, addd.data_ptr(), st), "dn_grad_apply_bwd_f32")
    if not torch.equal(addd.cpu(), out.cpu()):
        fails.append("d_x_add in place differs from the separate output")
    # dn_csr_mean_f32 on the irregular rowptr and on the transposed one (the hub row), div != 1
    xs = place(x, dev, mis)
    for name, rp, col, M, n in (("mean", mb.g_rowptr, mb.g_col, P, n_f), ("mean_t", mb.gt_rowptr, mb.gt_col, P.T, n_b)):
        o = place(torch.full((vt, C), float("nan")), dev, mis)
        _hip.check(L.dn_csr_mean_f32(rp.data_ptr(), col.data_ptr(), vt, xs.data_ptr(), C, 3.0, o.data_ptr(), st), "dn_csr_mean_f32")
        judge(name, o, (M @ x6) / 3.0, (M @ x6.abs()) / 3.0, n)
    helpers.record_margin("sparse_irregular", dev, C=C, misaligned=bool(mis), instantiation=instantiation(C, not mis),
                          route=list(spmm_route(C, not mis)), longest_row=n_f, longest_transposed_row=n_b, unit="2^-24", **res)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------
# 3. packing, the norm word, determinism
# ------------------------------------------------------------------------------------------------------------------------------
def run_packing(dev):
    """``coo_to_csr`` on the generator's pattern against scipy, bit for bit: the CSR, and the CSR of the transpose with ascending row ids inside
    every transposed row -- the hub's holds about V / 2 of them (the insertion sort of pack_finish_kernel), the unused column's none."""
    import scipy.sparse as sp
    from diffusion_net.batch import coo_to_csr
    meshes, _, _ = irregular_batch(dev)
    rows, cols, vx, vy = global_coo(meshes)
    vt = sum(SIZES)
    t = lambda a: torch.from_numpy(a).to(dev)
    rowptr, col, _, _, t_rowptr, t_col, t_vx, t_vy = coo_to_csr(t(rows), 1, t(cols), t(vx), t(vy), vt, vt)
    csr = sp.csr_matrix((np.ones_like(vx), (rows, cols)), shape=(vt, vt))
    csr.sort_indices()
    assert np.array_equal(rowptr.cpu().numpy(), csr.indptr) and np.array_equal(col.cpu().numpy(), csr.indices)
    order = np.lexsort((rows, cols))                        # transposed rows, ascending row ids inside each (explicit zeros stay entries)
    assert np.array_equal(t_rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=vt))]))
    assert np.array_equal(t_col.cpu().numpy(), rows[order])
    assert np.array_equal(t_vx.cpu().numpy(), vx[order]) and np.array_equal(t_vy.cpu().numpy(), vy[order])
    tl = np.diff(t_rowptr.cpu().numpy())
    assert tl[SIZES[0] + HUB] >= 0.4 * SIZES[1] and tl[UNUSED] == 0 and tl[SIZES[0] + UNUSED] == 0


def run_norm_word(dev):
    """``mb.amax[2]`` = max row sum of |gradX|, |gradY| -- a sum of n non-negative terms: within gamma_n of fp64, relatively."""
    _, mb, (GX, GY, P) = irregular_batch(dev)
    n = int(P.sum(1).max())
    ref = float(torch.maximum(GX.abs().sum(1).max(), GY.abs().sum(1).max()))
    got = float(mb.amax[2].cpu())
    # (which operator holds the maximum, and that the other one alone would miss it)
    only_x, only_y = float(GX.abs().sum(1).max()), float(GY.abs().sum(1).max())
    print("norm word %.9g, fp64 %.9g (|gradX| alone %.9g, |gradY| alone %.9g), gamma_%d = %.3g" % (got, ref, only_x, only_y, n, gamma(n)))
    helpers.record_margin("sparse_norm_word", dev, rel_err=abs(got - ref) / ref, gamma_n=gamma(n), n=n)
    assert abs(got - ref) <= gamma(n) * ref, (got, ref)
    return only_x, only_y


def run_determinism(dev):
    """Packing twice: the same words and patterns, bit for bit.  Forward + backward twice on fresh outputs: the same."""
    from diffusion_net import ops
    meshes, mb, _ = irregular_batch(dev)
    mb2 = pack(meshes, dev, chunk_rows=64)
    for name in ("g_rowptr", "g_col", "g_vx", "g_vy", "gt_rowptr", "gt_col", "gt_vx", "gt_vy", "amax"):
        assert torch.equal(getattr(mb, name).cpu(), getattr(mb2, name).cpu()), name
    for C in (32, 128):
        x = torch.randn(mb.v_total, C, generator=torch.Generator().manual_seed(C))
        runs = []
        for _ in range(2):
            xa = x.to(dev).requires_grad_(True)
            gx, gy = ops.GradApplyFn.apply(xa, mb)
            (gx - 2.0 * gy).sum().backward()
            runs.append((gx.detach().cpu(), gy.detach().cpu(), xa.grad.cpu()))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), C


# ------------------------------------------------------------------------------------------------------------------------------
# 4. block routes
# ------------------------------------------------------------------------------------------------------------------------------
# gather form of the chained forward -> (C, K, sizes, option chain_hh)
FORMS = {"c128_hh1_row_contiguous": (128, 128, SIZES, 1), "c128_hh2_operand_layout": (128, 128, SIZES, 2), "c64": (64, 128, SIZES, 0),
         "c256_rolling": (256, 256, SIZES_WIDE, 0)}


@contextlib.contextmanager
def options(**values):
    from diffusion_net import _hip
    saved = {k: _hip.get_option(k) for k in values}
    try:
        for k, v in values.items():
            _hip.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _hip.set_option(k, v)


@contextlib.contextmanager
def irregular_meshes():
    """The shared bodies of parity_cases.py build their batch with ``parity_cases.make_ragged``: inside this block that name is
    ``make_irregular`` (same signature), so the bodies -- assertions, tolerances and all -- run unchanged on the irregular operator."""
    plain = parity_cases.make_ragged
    parity_cases.make_ragged = lambda sizes, K, C_in, seed=0: _make_irregular(plain, sizes, K, C_in, seed)
    try:
        yield
    finally:
        parity_cases.make_ragged = plain


def run_chain_form(dev, form):
    """``parity_cases.run_chain_vs_unfused``, its own tolerances, on the irregular operator with the gather form selected."""
    C, K, sizes, hh = FORMS[form]
    with options(spectral_grad=0, chain_hh=hh), irregular_meshes():
        return parity_cases.run_chain_vs_unfused(dev, sizes=sizes, K=K, C=C, N_block=1)


def run_spectral_form(dev):
    """``parity_cases.run_spectral_grad`` on the irregular operator: its ``saved_rel_max`` comparison of xd / gx / gy between the spectral and the
    gather form is the check on ``sg_grad_kernel`` (rows that are not 7 long)."""
    with irregular_meshes():
        return parity_cases.run_spectral_grad(dev, sizes=SIZES, C=128, N_block=1)


def _block_forward(dev, mb, feats, C, seed=5, train=True):
    """One-block DiffusionNet, no dropout -> (out, saved activations of the block by name | None)."""
    import diffusion_net
    from diffusion_net import ops, synthetic
    torch.manual_seed(seed)
    model = diffusion_net.layers.DiffusionNet(3, 5, C_width=C, N_block=1, outputs_at="vertices", dropout=False)
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=seed))
    model.to(dev).train(train)
    x = torch.cat(feats, 0).to(dev).requires_grad_(train)
    ops.debug_saved = []
    try:
        with torch.set_grad_enabled(train):
            out = model.forward_packed(x, mb, None)
        saved = ops.debug_saved[0] if train else None
    finally:
        ops.debug_saved = None
    return out.detach(), saved


def run_saved_gather_bitwise(dev, form):
    """dn_chain.hip promises of its gathers "entry order, fmaf: bit for bit spmm_kernel's sums": the gx / gy the chained training forward saves
    equal ``ops.GradApplyFn`` on the xd it saved, under ``torch.equal``, in each gather form -- and the chained kernel is what ran."""
    from diffusion_net import ops
    C, K, sizes, hh = FORMS[form]
    meshes, feats = make_irregular(sizes, K, 3, seed=5)
    mb = pack(meshes, dev, chunk_rows=64)
    with options(spectral_grad=0, chain_hh=hh, chain=1):
        out, sv = _block_forward(dev, mb, feats, C)
        with options(chain=0):
            out_u, _ = _block_forward(dev, mb, feats, C)
    assert not torch.equal(out, out_u), "chained and unfused forward are bitwise equal: the chained kernel did not run"
    gx, gy = ops.GradApplyFn.apply(sv["xd"].detach(), mb)
    bad = {k: int((a != b).sum()) for k, a, b in (("gx", sv["gx"], gx), ("gy", sv["gy"], gy)) if not torch.equal(a, b)}
    assert not bad, ("saved gx / gy of the chained forward differ from spmm_kernel's (elements)", form, bad)


def run_cloud_backward(dev):
    """The operators of a 300-point cloud (31 entries per row; the transpose of a kNN graph is irregular, with hubs and empty rows) through
    forward + backward at C = 32 in train mode without dropout, against the oracle."""
    import diffusion_net
    import scipy.sparse as sp
    import cloud_cases
    from diffusion_net import synthetic
    from oracle import diffusionnet_oracle as orc
    N, K, C = 300, 16, 32
    pts = cloud_cases.sample(N, 3)
    v64 = torch.from_numpy(pts.astype(np.float64))
    nbr = diffusion_net.geometry.find_knn(v64, v64, 8, omit_diagonal=True, method="cpu_kd").indices.numpy()
    A = sp.coo_matrix((np.ones(N * 8), (np.repeat(np.arange(N), 8), nbr.reshape(-1))), shape=(N, N)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64)
    Lap, mass = (sp.diags(np.asarray(A.sum(axis=1)).reshape(-1)) - A).tocsr(), np.full(N, 4 * np.pi / N)
    verts = torch.from_numpy(pts).to(dev)
    _, massvec, Lt, evals, evecs, gX, gY = diffusion_net.geometry.compute_operators(verts, torch.zeros(0, 3, dtype=torch.long, device=dev), K,
                                                                                  laplacian=(Lap, mass))
    assert gX._nnz() == N * 31
    tl = np.bincount(gX.cpu().indices()[1].numpy(), minlength=N)
    assert tl.min() < tl.max(), "the transposed operator of the cloud has rows of one length"
    torch.manual_seed(4)
    model = diffusion_net.layers.DiffusionNet(3, 6, C_width=C, N_block=2, outputs_at="vertices", dropout=False)
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=4))
    params = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(dev).train(True)
    x = verts.clone().requires_grad_(True)
    out = model(x, massvec, L=Lt, evals=evals, evecs=evecs, gradX=gX, gradY=gY)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (out * w.to(dev)).sum().backward()
    c = lambda t: t.detach().cpu()
    ref, rg = orc.net_forward_backward(params, dict(x_in=c(verts), mass=c(massvec), evals=c(evals), evecs=c(evecs), gradX=c(gX), gradY=c(gY)),
                                       outputs_at="vertices", loss_weights=w)
    got = {"x_in": x.grad.cpu(), **{k: p.grad.cpu() for k, p in model.named_parameters()}}
    e_f = helpers.rel_max(c(out), ref.reshape(out.shape))
    e_g = {k: helpers.rel_l2(v, rg[k].reshape(v.shape)) for k, v in got.items()}
    wk = max(e_g, key=e_g.get)
    helpers.record_margin("cloud_forward_backward", dev, n=N, k_eig=K, C=C, transposed_row_lengths=[int(tl.min()), int(tl.max())], fwd_rel_max=e_f,
                          worst_gradient_rel_l2=e_g[wk], worst_gradient=wk, fwd_tol=FWD_TOL, grad_tol=GRAD_TOL)
    assert e_f < FWD_TOL, e_f
    bad = {k: v for k, v in e_g.items() if not v < GRAD_TOL}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------
# 5. a non-finite value stays inside its mesh
# ------------------------------------------------------------------------------------------------------------------------------
ISOLATION_ROUTES = {"unfused": dict(chain=0, spectral_grad=0), "gather_hh1": dict(chain=1, chain_hh=1, spectral_grad=0),
                    "gather_hh2": dict(chain=1, chain_hh=2, spectral_grad=0), "spectral": dict(chain=1, chain_hh=1, spectral_grad=2)}


def run_nan_isolation(dev, route, planted):
    """C = K = 128, meshes of 150 and 131 rows: a NaN in one input feature of mesh ``planted`` leaves every row of the other mesh finite and
    bitwise what a run without the NaN gives -- the training forward (saved xd / gx / gy too) and the inference forward.  Both gather forms of
    the chained kernel pad the rows of a wave to its longest row, and a padding entry carries weight 0: 0 x NaN must not be formed from another
    mesh's rows.  The planted mesh's features are 2^-6 of the other's: every batch-wide magnitude word of the split-fp16 engine is then set by the
    clean mesh in both runs, so that bitwise equality is what isolation means."""
    meshes, feats = make_irregular(SIZES, 128, 3, seed=5)
    mb = pack(meshes, dev, chunk_rows=64)
    feats = [f * (2.0 ** -6 if i == planted else 1.0) for i, f in enumerate(feats)]
    dirty = [f.clone() for f in feats]
    dirty[planted][3, 1] = float("nan")
    lo = sum(SIZES[:1 - planted])
    keep = slice(lo, lo + SIZES[1 - planted])           # the rows of the clean mesh
    with options(**ISOLATION_ROUTES[route]):
        for train in (True, False):
            (o0, s0), (o1, s1) = _block_forward(dev, mb, feats, 128, train=train), _block_forward(dev, mb, dirty, 128, train=train)
            named = {k: (s0[k], s1[k]) for k in ("xd", "gx", "gy")} if train else {}
            named["out"] = (o0, o1)
            for k, (a, b) in named.items():
                a, b = a.detach().cpu()[keep], b.detach().cpu()[keep]
                assert bool(torch.isfinite(b).all()), "%s: %s of the clean mesh holds %d non-finite values (%s forward)" % (
                    route, k, int((~torch.isfinite(b)).sum()), "training" if train else "inference")
                assert torch.equal(a, b), "%s: %s of the clean mesh changed with the NaN in the other mesh (%s forward)" % (
                    route, k, "training" if train else "inference")
            dirty_rows = o1.cpu()[slice(0, SIZES[0]) if planted == 0 else slice(SIZES[0], sum(SIZES))]
            assert not bool(torch.isfinite(dirty_rows).all()), "the planted NaN did not reach the output of its own mesh"

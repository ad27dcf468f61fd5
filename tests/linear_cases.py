"""Shared bodies of the nn.Linear and heat-kernel-signature tests (drivers: test_linear_emu.py on the emulator build, test_linear_gpu.py on the
device): every route of ``dn_linear_fwd_amax_f32`` / ``dn_linear_bwd_amax_f32`` as an isolated op against the fp64 evaluation of the same inputs,
the magnitude words both entry points leave behind, misaligned operands, the backward inside exactly the workspace it asks for on a batch of
many small chunks, and ``hks_kernel`` off its tile sizes.

Criterion: the condition-scaled error  s = max_ij |got - ref|_ij / S_ij,  S being the reference expression evaluated on absolute values
(|x| |W|^T + |b| for the forward).  Any summation order of an fp32 product-sum of n terms obeys s <= gamma_n = n u / (1 - n u), u = 2^-24, so that
bound is a priori; the pure-fp32 VALU kernels must also stay within 4 x torch's own fp32 CPU evaluation (floored at 2 u), the margin a different
summation order accounts for.  ``rel_max`` on the result would measure the conditioning of the inputs instead (one cancelling column sum at
C_out = 1)."""
import torch

import helpers
from parity_cases import FWD_TOL, GRAD_TOL, make_ragged, pack

U = 2.0 ** -24
D, T, B = (200, 77), (33, 40), (1500, 600)      # the default batch; fewer rows than one block pass of thin_tn; past the 512-workgroup cap at N = 1024

# (sizes, C_in, C_out, misalign): misalign names the operands handed over 4 bytes past a 16-byte boundary ("x", "d" = d_out)
CASES = [
    # thin input: smallk_rows forward (<4>, <8>, <16>; K < KMAX and K == KMAX), thin_tn m-major / smalln_tn weight gradients
    (D, 1, 128, ""), (D, 2, 130, ""), (D, 3, 260, ""), (D, 3, 28, ""), (D, 3, 31, ""), (D, 3, 32, ""), (D, 3, 33, ""), (D, 3, 36, ""),
    (D, 4, 132, ""), (D, 5, 260, ""), (D, 8, 128, ""), (D, 9, 130, ""), (D, 16, 128, ""),
    # both sides thin: smalln_tn and its bias product at C_out around 4, smallk_rows on both passes
    (D, 16, 1, ""), (D, 16, 2, ""), (D, 8, 3, ""), (D, 16, 4, ""), (D, 16, 5, ""), (D, 17, 7, ""),
    # C_in 17..33 against the m-major bounds: ragged n0 groups of thin_tn, the row GEMM forward
    (D, 17, 128, ""), (D, 30, 128, ""), (D, 31, 260, ""), (D, 32, 36, ""), (D, 33, 36, ""), (D, 32, 32, ""),
    # thin output: thin_tn n-major against its bounds, smallk_rows for d_x
    (D, 32, 7, ""), (D, 28, 7, ""), (D, 33, 3, ""), (D, 34, 5, ""), (D, 36, 32, ""), (D, 36, 33, ""), (D, 36, 31, ""),
    (D, 128, 1, ""), (D, 130, 2, ""), (D, 132, 9, ""), (D, 260, 15, ""), (D, 128, 16, ""), (D, 128, 17, ""), (D, 260, 4, ""), (D, 132, 8, ""),
    # either side of the 1024 limit of smallk_rows (1028: the next width thin_tn takes)
    (D, 1028, 3, ""), (D, 1025, 3, ""), (D, 3, 1028, ""), (D, 3, 1025, ""),
    (T, 3, 128, ""),
    (B, 3, 1024, ""), (B, 16, 1024, ""), (B, 1024, 3, ""), (B, 1024, 16, ""),
    # misaligned x: no vector input load in smallk_rows; no n-major thin_tn
    (D, 4, 128, "x"), (D, 8, 36, "x"), (D, 16, 130, "x"), (D, 32, 3, "x"), (D, 128, 7, "x"),
    # misaligned d_out: no m-major thin_tn (smalln_tn up to C_in = 16, split-V above); no vector input load in the d_x smallk_rows
    (D, 3, 32, "d"), (D, 16, 128, "d"), (D, 17, 32, "d"), (D, 32, 36, "d"), (D, 16, 16, "xd"),
]
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 30, 31, 32, 33, 34, 36, 128, 130, 132, 260, 1024, 1028)

# the integer bounds of the dispatch (csrc/dn_api.hip, nn.Linear section), by the name routes() knows them under
BOUNDS = {"fwd_cin": 16, "fwd_cout": 1024, "m_cin": 32, "m_cout": 32, "n_cout": 32, "n_cin": 32, "smalln_cin": 16, "dx_cout": 16, "dx_cin": 1024}
# m_cout and n_cin stand next to a `% 4 == 0` test: the nearest width below 32 that only the bound keeps out is 28
STEP = {"m_cout": 4, "n_cin": 4}


def routes(C_in, C_out, x_aligned=True, d_out_aligned=True, bounds=BOUNDS, mod4=True):
    """(forward, dW/db, d_x) route names for one call.  ``bounds`` / ``mod4`` / the alignment flags exist for the table test, which moves one
    condition at a time and asks whether some case notices.  (The workspace test of the m-major branch is always true: its partials are
    sized by the same chunk count.  The forward's relu / mask never come from ``ops.linear_fwd``.)"""
    b = bounds
    fwd = "smallk_rows" if C_in <= b["fwd_cin"] and C_out <= b["fwd_cout"] else "row_gemm"
    if C_in <= b["m_cin"] and C_out >= b["m_cout"] and (C_out % 4 == 0 or not mod4) and d_out_aligned:
        dw = "thin_tn_m"
    elif C_out <= b["n_cout"] and C_in >= b["n_cin"] and (C_in % 4 == 0 or not mod4) and x_aligned:
        dw = "thin_tn_n"
    elif C_in <= b["smalln_cin"]:
        dw = "smalln_tn"
    else:
        dw = "split_v"
    dx = "smallk_rows" if C_out <= b["dx_cout"] and C_in <= b["dx_cin"] else "bwd_input"
    return fwd, dw, dx


ROUTE_NAMES = {"fwd": ("smallk_rows", "row_gemm"), "dw": ("thin_tn_m", "thin_tn_n", "smalln_tn", "split_v"), "dx": ("smallk_rows", "bwd_input")}


def passes(case):
    """The passes a case runs: both, but at the 2100-row size only the one whose smallk_rows launch has the width 1024 on its output side."""
    return ("fwd", "bwd") if case[0] != B else ("fwd",) if case[2] == 1024 else ("bwd",)


def case_routes(case, **moved):
    """routes() of a case, with None for a pass the case does not run."""
    _, ci, co, mis = case
    fwd, dw, dx = routes(ci, co, "x" not in mis, "d" not in mis, **moved)
    return (fwd if "fwd" in passes(case) else None,) + ((dw, dx) if "bwd" in passes(case) else (None, None))


def check_case_table():
    """Every route is reached three times; every comparison of the dispatch has a case on each side that it alone decides."""
    got = [case_routes(c) for c in CASES]
    for pos, key in enumerate(("fwd", "dw", "dx")):
        for name in ROUTE_NAMES[key]:
            n = sum(r[pos] == name for r in got)
            assert n >= 3, "%s route %s is reached by %d case(s)" % (key, name, n)
    noticed = lambda **moved: [c for c, r in zip(CASES, got) if case_routes(c, **moved) != r]
    for name, v in BOUNDS.items():
        for step in (-STEP.get(name, 1), STEP.get(name, 1)):
            hit = noticed(bounds=dict(BOUNDS, **{name: v + step}))
            assert hit, "no case notices %s = %d moved to %d" % (name, v, v + step)
    for pos, route in ((1, "thin_tn_n"), (2, "thin_tn_m")):     # a width off the multiple of 4 that only `% 4` keeps out, and a multiple of 4 next to it that gets in
        hit = [c for c in noticed(mod4=False) if c[pos] % 4]
        assert hit, "no case notices the %% 4 test of %s" % route
        near = {w for c in hit for w in (c[pos] - c[pos] % 4, c[pos] - c[pos] % 4 + 4)}
        assert any(c[pos] in near and r[1] == route for c, r in zip(CASES, got)), route
    for mis in ("x", "d"):
        hit = [c for c, r in zip(CASES, got) if mis in c[3] and routes(c[1], c[2]) != r]
        assert len(hit) >= 2, "fall-through of a misaligned %s" % mis
    seen = {w for c in CASES for w in c[1:3]}
    assert seen >= set(WIDTHS), sorted(set(WIDTHS) - seen)
    assert all(min(c[1], c[2]) <= 36 for c in CASES)


def gamma(n):
    return n * U / (1.0 - n * U)


def scaled_err(got, ref, scale):
    return float(((got.detach().cpu().double() - ref).abs() / scale).max())


def offset_copy(t, dev):
    """``t`` on ``dev``, contiguous, its first element 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


_BATCHES = {}


def batch(dev, sizes):
    key = (str(dev), tuple(sizes))
    if key not in _BATCHES:
        _BATCHES[key] = pack(make_ragged(sizes, 8, 3, seed=1)[0], dev, with_grad=False)
    return _BATCHES[key]


def make_inputs(rows, C_in, C_out, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C_in, generator=g)
    W = torch.randn(C_out, C_in, generator=g) / C_in ** 0.5
    b = torch.randn(C_out, generator=g)
    d_out = torch.randn(rows, C_out, generator=g)
    return x, W, b, d_out


def references(x, W, b, d_out):
    """name -> (fp64 result, the same expression on absolute values, torch's fp32 CPU evaluation, addends + 1)."""
    x6, W6, b6, d6 = (t.double() for t in (x, W, b, d_out))
    rows, (C_out, C_in) = x.shape[0], W.shape
    return {
        "out": (x6 @ W6.T + b6, x6.abs() @ W6.abs().T + b6.abs(), x @ W.T + b, C_in + 1),
        "d_x": (d6 @ W6, d6.abs() @ W6.abs(), d_out @ W, C_out),
        "dW": (d6.T @ x6, d6.abs().T @ x6.abs(), d_out.T @ x, rows),
        "db": (d6.sum(0), d6.abs().sum(0), d_out.sum(0), rows),
    }


def place(t, dev, misaligned):
    return offset_copy(t, dev) if misaligned else t.to(dev)


def call_linear(dev, mb, x, W, b, d_out, mis="", run=("fwd", "bwd")):
    """One forward and / or one backward call -> ({name: result}, {name: word | None}).  Aligned operands take the forward through ``LinearFn``
    (the word travels as the output's tag); the backward is always the plain launch function, whose word is its second result."""
    from diffusion_net import ops
    xd, dd = place(x, dev, "x" in mis), place(d_out, dev, "d" in mis)
    Wd, bd = W.to(dev), b.to(dev)
    got, words = {}, {}
    if "fwd" in run:
        if mis:
            got["out"], words["out"] = ops.linear_fwd(mb, xd, Wd, bd)
        else:
            got["out"] = ops.LinearFn.apply(xd, Wd, bd, mb)
            tag = getattr(got["out"], "_dn_amax", None)
            words["out"] = None if tag is None else tag[0]
    if "bwd" in run:
        got["dW"], got["db"] = torch.empty_like(Wd), torch.empty_like(bd)
        got["d_x"], words["d_x"] = ops.linear_bwd(mb, dd, xd, Wd, got["dW"], got["db"])
    return got, words


def check_words(got, words, C_in, C_out):
    """The words are maxima: no rounding, no order -- bit-exact on either route, and absent where ``ops`` allocates none."""
    for name, word in words.items():
        if (C_in <= 16 and C_out >= 128) if name == "out" else (C_out <= 16 and C_in >= 128):
            assert word is not None, "no magnitude word for " + name
            assert torch.equal(word.cpu(), got[name].detach().abs().max().reshape(1).cpu()), (name, float(word), float(got[name].abs().max()))
        else:
            assert word is None, "unexpected magnitude word for " + name


def run_case(dev, sizes, C_in, C_out, mis):
    rows = sum(sizes)
    x, W, b, d_out = make_inputs(rows, C_in, C_out, 1000 * C_in + C_out)
    got, words = call_linear(dev, batch(dev, sizes), x, W, b, d_out, mis, passes((sizes, C_in, C_out, mis)))
    fwd, dw, dx = routes(C_in, C_out, "x" not in mis, "d" not in mis)
    # pure fp32 FMAs: smallk_rows, thin_tn (dW and its column sums), smalln_tn (dW only: its db is a split-V product)
    valu = {"out": fwd == "smallk_rows", "d_x": dx == "smallk_rows", "dW": dw != "split_v", "db": dw in ("thin_tn_m", "thin_tn_n")}
    rec, failures = {}, []
    for name, (ref, scale, t32, n) in references(x, W, b, d_out).items():
        if name not in got:
            continue
        s, s32 = scaled_err(got[name], ref, scale), scaled_err(t32, ref, scale)
        rec["s_" + name], rec["s_torch32_" + name] = s / U, s32 / U
        print("linear %s %dx%d%s %s: s = %.2f u, torch fp32 %.2f u, gamma_n %.1f u" % (sizes, C_in, C_out, mis and " mis=" + mis, name, s / U, s32 / U, gamma(n) / U))
        if not s <= gamma(n):
            failures.append("%s: s = %.3g u above gamma_%d" % (name, s / U, n))
        if valu[name]:
            if not s <= 4 * max(s32, 2 * U):
                failures.append("%s: s = %.3g u above 4 x max(torch fp32 %.3g u, 2 u)" % (name, s / U, s32 / U))
        elif name == "out":
            if not helpers.rel_max(got[name].detach().cpu(), ref) < FWD_TOL:
                failures.append("out: rel_max %.3g" % helpers.rel_max(got[name].detach().cpu(), ref))
        elif not helpers.rel_l2(got[name].detach().cpu(), ref) < GRAD_TOL:
            failures.append("%s: rel_l2 %.3g" % (name, helpers.rel_l2(got[name].detach().cpu(), ref)))
    helpers.record_margin("linear_routes", dev, sizes=list(sizes), C_in=C_in, C_out=C_out, misalign=mis, routes=[fwd, dw, dx], unit="2^-24", **rec)
    assert not failures, failures
    check_words(got, words, C_in, C_out)


# ------------------------------------------------------------------------------------------------------------------------------
# magnitude words: where the maximum sits, and at which scale
# ------------------------------------------------------------------------------------------------------------------------------
WORD_WIDTHS = [(D, 3, 130), (T, 3, 1028)]     # forward as given, backward transposed: the kernel's own epilogue; measure_amax
WORD_PLACES = ["negative", "last_row", "ragged_column"]
WORD_SCALES = [0, -20, 20]


def run_word(dev, passname, sizes, thin, wide, where, log2_scale):
    """Plants the largest magnitude of the result at a chosen element -- negative, in the last row, or in the last column (at width 130 the
    second of a two-column group) -- and reads it back from the word, with the streamed operand scaled by a power of two."""
    rows = sum(sizes)
    C_in, C_out = (thin, wide) if passname == "fwd" else (wide, thin)
    x, W, b, d_out = make_inputs(rows, C_in, C_out, 77)
    r = rows - 1 if where == "last_row" else 25       # (at width 130 a workgroup covers 7 rows a pass: row 25 is held by its third wave)
    n = wide - 1 if where == "ragged_column" else 57
    sign = -1.0 if where == "negative" else 1.0
    if passname == "fwd":        # out[r, n] = x[r] . W[n] + b[n]: W[n] eight times as long as any other row of W, x[r] along it and ten long
        W[n] *= 8.0 * W.norm(dim=1).max() / W[n].norm()
        x[r] = sign * 10.0 * W[n] / W[n].norm()
    else:                        # d_x[r, n] = d_out[r] . W[:, n]: the same with the columns of W
        W[:, n] *= 8.0 * W.norm(dim=0).max() / W[:, n].norm()
        d_out[r] = sign * 10.0 * W[:, n] / W[:, n].norm()
    scale = 2.0 ** log2_scale
    x, b, d_out = x * scale, b * scale, d_out * scale
    name = "out" if passname == "fwd" else "d_x"
    ref, sabs, _, nterms = references(x, W, b, d_out)[name]
    top = int(ref.abs().argmax())
    assert (top // wide, top % wide) == (r, n) and float(ref[r, n]) * sign > 0, "the test's own planting went wrong"
    assert float(ref.abs().flatten().topk(2).values[1]) < 0.9 * abs(float(ref[r, n]))
    got, words = call_linear(dev, batch(dev, sizes), x, W, b, d_out, run=(passname,))
    check_words(got, words, C_in, C_out)
    assert torch.equal(words[name].cpu(), got[name][r, n].detach().abs().reshape(1).cpu())
    assert scaled_err(got[name], ref, sabs) <= gamma(nterms)


def run_unaligned_out(dev):
    """The C entry point with ``out`` 4 bytes past a 16-byte boundary (N % 4 == 0, so the alignment alone turns the vector store off): right
    result, right word, and the floats on either side of the output keep their fill."""
    from diffusion_net import _hip
    rows, C_in, C_out = sum(D), 3, 128
    x, W, b, _ = make_inputs(rows, C_in, C_out, 5)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    pad = 64
    buf = torch.full((rows * C_out + 2 * pad + 1,), -7.0, dtype=torch.float32, device=dev)
    out = buf[pad + 1:pad + 1 + rows * C_out]
    assert out.data_ptr() % 16 == 4
    word = torch.zeros(1, dtype=torch.float32, device=dev)
    _hip.check(_hip.lib().dn_linear_fwd_amax_f32(batch(dev, D).ref(), xd.data_ptr(), C_in, Wd.data_ptr(), bd.data_ptr(), C_out, 0, None,
                                                 out.data_ptr(), word.data_ptr(), _hip.stream_of(xd)), "dn_linear_fwd_amax_f32")
    ref, sabs, t32, n = references(x, W, b, torch.zeros(rows, C_out))["out"]
    s, s32 = scaled_err(out.view(rows, C_out), ref, sabs), scaled_err(t32, ref, sabs)
    assert s <= gamma(n) and s <= 4 * max(s32, 2 * U), (s / U, s32 / U)
    assert torch.equal(word.cpu(), out.abs().max().reshape(1).cpu())
    assert bool((buf[:pad + 1] == -7.0).all()) and bool((buf[pad + 1 + rows * C_out:] == -7.0).all()), "a store outside the output"


def run_exact_workspace_many_chunks(dev):
    """The backward through the C entry point on a batch of 132 sixteen-row chunks, C_in = 1, C_out = 31 (smalln_tn; its bias gradient from the
    4-column split-V product), with exactly the bytes ``dn_linear_workspace_bytes`` asks for: per-chunk partials grow with the chunk count while
    the smalln_tn region does not, so this is where a product wider than 4 columns would leave the workspace.  The floats on either side of
    it keep their fill, and the results are right."""
    from diffusion_net import _hip
    from diffusion_net.batch import MeshBatch
    rows, C_in, C_out = sum(B), 1, 31
    assert routes(C_in, C_out) == ("smallk_rows", "smalln_tn", "bwd_input")
    mb = MeshBatch.rows_only(rows, dev, chunk_rows=16)
    x, W, b, d_out = make_inputs(rows, C_in, C_out, 9)
    xd, Wd, dd = x.to(dev), W.to(dev), d_out.to(dev)
    L = _hip.lib()
    need = int(L.dn_linear_workspace_bytes(mb.ref(), C_in, C_out))
    assert need % 4 == 0
    guard = 1 << 18
    buf = torch.full((need // 4 + 2 * guard,), -7.0, dtype=torch.float32, device=dev)
    ws = buf[guard:guard + need // 4]
    assert ws.data_ptr() % 16 == 0
    got = {"d_x": torch.empty_like(xd), "dW": torch.empty_like(Wd), "db": torch.empty(C_out, dtype=torch.float32, device=dev)}
    _hip.check(L.dn_linear_bwd_amax_f32(mb.ref(), dd.data_ptr(), xd.data_ptr(), Wd.data_ptr(), C_in, C_out, got["d_x"].data_ptr(),
                                        got["dW"].data_ptr(), got["db"].data_ptr(), None, ws.data_ptr(), need, _hip.stream_of(xd)),
               "dn_linear_bwd_amax_f32")
    assert bool((buf[:guard] == -7.0).all()) and bool((buf[guard + need // 4:] == -7.0).all()), "a store outside the workspace"
    refs = references(x, W, b, d_out)
    for name in got:
        ref, scale, _, n = refs[name]
        assert scaled_err(got[name], ref, scale) <= gamma(n), name


# ------------------------------------------------------------------------------------------------------------------------------
# heat kernel signature: K off the 32-wide chunk, S past one 16-scale block and off the 4-scale group, V off the 64-row block, B > 1
# ------------------------------------------------------------------------------------------------------------------------------
HKS_CASES = [(1, 63, 31, 5, False), (1, 65, 33, 17, False), (2, 130, 20, 16, True), (3, 257, 128, 33, True), (2, 64, 160, 4, False)]


def run_hks(dev, Bn, V, K, S, per_batch):
    """All terms are positive, so the element-wise relative error against fp64 is the measure; torch's fp32 evaluation of the same formula
    sets the bar, with the margin and floor of the linear VALU kernels."""
    from diffusion_net import ops
    g = torch.Generator().manual_seed(100 * V + S)
    evals = torch.cumsum(0.05 + 0.5 * torch.rand(Bn, K, generator=g), dim=1)         # increasing, positive
    evecs = torch.randn(Bn, V, K, generator=g) / V ** 0.5
    scales = torch.logspace(-2, 0.0, steps=S)
    if per_batch:
        scales = scales[None] * (1.0 + 0.5 * torch.arange(Bn, dtype=torch.float32))[:, None]
    formula = lambda ev, ph, sc: torch.einsum("bks,bvk->bvs", torch.exp(-ev[:, :, None] * (sc if sc.dim() == 2 else sc[None])[:, None, :]), ph * ph)
    ref = formula(evals.double(), evecs.double(), scales.double())
    e32 = float(((formula(evals, evecs, scales).double() - ref).abs() / ref).max())
    if Bn == 1:
        got = ops.hks(evals[0].to(dev), evecs[0].to(dev), scales.to(dev))[None]
    else:
        got = ops.hks(evals.to(dev), evecs.to(dev), scales.to(dev))
    assert tuple(got.shape) == (Bn, V, S)
    e = float(((got.cpu().double() - ref).abs() / ref).max())
    print("hks B=%d V=%d K=%d S=%d: rel err %.3e, torch fp32 %.3e" % (Bn, V, K, S, e, e32))
    helpers.record_margin("hks_shapes", dev, B=Bn, V=V, K=K, S=S, per_batch_scales=bool(per_batch), rel_err=e, rel_err_torch32=e32)
    assert e <= 4 * max(e32, 2 * U), (e, e32)

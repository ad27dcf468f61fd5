"""Shared bodies of the tests of the fused head (dn_head.hip), the mass-weighted mean (``mass_mean_*_kernel``) and the content checksum
(``checksum_multi_kernel``) as isolated ops.  Drivers: test_head_emu.py on the emulator build, test_head_gpu.py on the device.

The head.  A row of C classes is handled by G = 2^k <= 64 lanes (G >= C up to 64), lane l owning the classes l, l + G, ...: cpl = ceil(C / G) of
them, in the instantiation for 1, 2, 4, 8, 16 or 32 classes per lane.  CASES crosses the widths on either side of every boundary of G and of the
instantiation with the gather (none / edges / faces), log_softmax on and off, smoothing 0 / 0.1, which gradients arrive (loss, log-probabilities,
both) and two logit scales; ``check_case_table`` proves the coverage with no library.  The gather pattern (``build_pattern``) is built on purpose:
a hub vertex in every output, two vertices nobody references (vertex 0 among them: empty transposed rows, the wave pads to its longest group), a
vertex twice in one output, the last vertex in the last output only; ``check_pattern`` asserts each feature.

Criteria.  The reference is torch's evaluation of the same formula in fp64 on the fp32 inputs, eps = 2^-23 (one ulp at 1).  The constants count
operations; none is fitted to a kernel's output, and before a bound judges the kernel torch's own fp32 CPU evaluation has to pass it.

  log-probabilities, output row i, n_per gathered rows, M_i = max_c mean_j |x[col_j, c]| (over the classes whose mean is finite; a masked class
  contributes exp(-inf) = 0 exactly), lse_i the fp64 log-sum-exp:
      |lp - ref| <= B_i = eps ((n_per + 3) M_i + |lse_i| + cpl / 2 + 8)
    the gather mean is n_per - 1 additions and one product with the rounded 1 / n_per: (n_per + 1) / 2 eps M_i; z - max is one rounding of at most
    2 M_i: eps M_i; lse = max + log(se) and z - lse are one rounding each of at most M_i + |lse_i|: together below eps (M_i + |lse_i|); the
    argument error of expf passes into log(se) once more: eps M_i.  The sum se of cpl terms per lane and log2 G shuffle steps carries
    (cpl - 1 + 6) / 2 eps relative, which log turns into an absolute error; expf and logf one ulp each (log se <= log 2048 < 8).  With
    log_softmax off and no gather the head copies its input: there the log-probabilities must be bitwise the input.
  loss, term_i the smoothed cross entropy of row i, over the rows that count:
      |loss - ref| <= mean_i B_i + eps (n_iter + 20) mean_i |term_i|
    B_i weighted by the smoothed target, whose weights sum to one; all log-probabilities are <= 0, so the sum over the classes of one row
    (cpl + 6 additions, two products) and the sum over rows (n_iter additions of one thread, n_iter = ceil(n_out / (blocks rows_per_block)) the
    trips of the grid-stride loop; then 6 shuffle steps, 2 additions across waves, the 8 + 8 of the finish kernel and the division, half an eps
    each) do not cancel: their relative errors add to below (n_iter + 20) eps.
  d_x[v, c], dlp = incoming d_logp + the loss term, p the fp64 softmax, deg_v the entries of the transposed row:
      S_vc = (1 / n_per) sum_{i in v} (|dlp_ic| + p_ic sum_c |dlp_ic|)
      |got - ref| <= eps (deg_v + cpl / 2 + 8) S_vc + (1 / n_per) sum_{i in v} ((B_i + eps |lp_ic|) p_ic + 2^-126) |sum_c dlp_ic|
    deg_v additions into the accumulator, the class sum of cpl + 6 additions, expf, the products with the loss scale and 1 / n_per; the second
    term is what the forward's error in lp (B_i, and its rounding to fp32) does to p = exp(lp), and 2^-126 the absolute error of a p below the
    normal range of fp32, denormal or flushed to zero (at logits x 1e4 the fp64 p reaches 1e-236; torch's fp32 evaluation misses the bound
    without this term, which is how it got here).  A vertex nobody references has S = 0 and no such term: exactly 0.0.

Non-finite and extreme inputs: torch (log_softmax + F.nll_loss, or the label-smoothing formula) on the CPU is the contract -- see each body.

Mass mean: n rows of a mesh go to RL = 256 / CL row lanes (CL = 32 channel lanes for C <= 32, else 64), four partial sums each: ceil(n / (4 RL)) fmaf
per partial, 2 + RL additions, the division and the same chain in the mass sum -> gamma_k sum m |x| / sum m with k = ceil(n / (4 RL)) + RL + 6 and
gamma_k = k u / (1 - k u), u = 2^-24; the backward is three roundings on the rounded mass sum: 4 eps |d_out| m / sum m.

Checksum: ``checksum_model`` is dn_pack.hip's hash in Python integers; the kernel has to equal it exactly at every length and pointer offset."""
import collections
import math

import numpy as np
import torch

import helpers
from linear_cases import gamma
from parity_cases import make_ragged, pack

EPS = 2.0 ** -23
TINY = 2.0 ** -126           # the smallest normal float: what a flushed or denormal p = exp(lp) is off by
HEAD_BLOCKS = 2048            # DN_HEAD_BLOCKS (csrc/dn_api.hip): the forward's grid, past which one block strides over several row groups
BWD_BLOCKS = 8192             # the cap of dn_launch_head_bwd
CPLS = (1, 2, 4, 8, 16, 32)
GROUPS = (1, 2, 4, 8, 16, 32, 64)
BOUNDARY_C = (1, 2, 3, 7, 8, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
WIDTHS = tuple(sorted(BOUNDARY_C + (9, 16, 17, 32)))      # 9 .. 32: the only widths with G = 16 and G = 32
N_SRC, N_OUT = 37, 53         # primes: no multiple of the rows of a wave or of a block at any G -- dead rows run along in every wave
HUB, UNUSED = 5, (0, 11)
GATHERS = {"none": 1, "edges": 2, "faces": 3}
GRADS = ("loss", "logp", "both")
SCALES = (2.0, 1.0e4)         # randn x 2; randn x 1e4, where the softmax saturates
G_LOSS = 1.7                  # the gradient arriving at the loss

Case = collections.namedtuple("Case", "C gather lsm smoothing grads scale n_src n_out")


def head_group(C):
    g = 1
    while g < C and g < 64:
        g <<= 1
    return g


def head_route(C):
    """dn_launch_head_fwd / _bwd restated -> (G, classes per lane, instantiation, rows per block)."""
    G = head_group(C)
    cpl = -(-C // G)
    return G, cpl, next(c for c in CPLS if cpl <= c), 4 * (64 // G)


def _table():
    cases = []
    for i, C in enumerate(WIDTHS):                      # every width with every gather; smoothing, gradients and scale rotate
        for j, gather in enumerate(GATHERS):
            n_src = N_OUT if gather == "none" else N_SRC
            cases.append(Case(C, gather, True, (0.0, 0.1)[(i + j) % 2], GRADS[(i + 2 * j) % 3], SCALES[int(j == i % 3)], n_src, N_OUT))
    for i, C in enumerate((1, 2, 8, 17, 64, 65, 129, 257, 513, 2048)):      # given log-probabilities (F.nll_loss, the smoothed loss): loss only
        cases.append(Case(C, "none", False, (0.0, 0.1)[i % 2], "loss", SCALES[(i // 2) % 2], N_OUT, N_OUT))
    for C in (1, 64):                                   # one row; one row more than a block holds
        rpb = head_route(C)[3]
        cases += [Case(C, "none", True, 0.1, "both", 2.0, 1, 1), Case(C, "none", True, 0.0, "both", 2.0, rpb + 1, rpb + 1)]
    return cases


# the grid-stride loop of the forward with log_softmax on, with and without a gather; the block cap of the backward at two classes per lane
STRIDE_CASES = [Case(65, "none", True, 0.1, "loss", 2.0, 9000, 9000), Case(64, "faces", True, 0.0, "both", 2.0, 3000, 8300),
                Case(65, "faces", True, 0.0, "both", 2.0, 33000, 100)]
GPU_ONLY_CASES = [Case(8, "none", True, 0.0, "loss", 2.0, 66000, 66000)]          # the stride of a small group: 32 rows a block
CASES = _table()


def case_id(c):
    return "C%d-%s-%s-s%g-%s-x%g-%dto%d" % (c.C, c.gather, "lsm" if c.lsm else "given", c.smoothing, c.grads, c.scale, c.n_src, c.n_out)


def check_case_table():
    """CASES reaches every instantiation forward and backward, every group width, both sides of every boundary, and every option with every
    other; the stride cases are past the grids they are named for."""
    routes = [head_route(c.C) for c in CASES]
    assert {r[0] for r in routes} == set(GROUPS), sorted({r[0] for r in routes})
    assert {c.C for c in CASES} >= set(BOUNDARY_C)
    for lo, hi in ((1, 2), (2, 3), (7, 8), (8, 9), (16, 17), (32, 33), (64, 65), (128, 129), (256, 257), (512, 513), (1024, 1025), (2047, 2048)):
        assert lo in WIDTHS and hi in WIDTHS
        assert lo + 1 == hi and (head_route(lo)[:3] != head_route(hi)[:3] or hi == 2048 or (lo, hi) == (7, 8)), (lo, hi)
    assert head_route(2048)[1:3] == (32, 32) and head_route(2047)[1] == 32 and head_route(1025)[1] == 17 and head_route(7)[0] == head_route(8)[0] == 8
    assert all(c.grads in GRADS and c.gather in GATHERS and c.scale in SCALES and (c.lsm or c.gather == "none") for c in CASES)
    for inst in CPLS:                                   # every case runs forward and backward
        mine = [c for c, r in zip(CASES, routes) if r[2] == inst]
        seen = lambda f: {f(c) for c in mine}
        assert seen(lambda c: c.gather) == set(GATHERS), (inst, "gather")
        assert seen(lambda c: c.smoothing) == {0.0, 0.1} and seen(lambda c: c.grads) == set(GRADS) and seen(lambda c: c.scale) == set(SCALES), inst
        assert seen(lambda c: c.lsm) == {True, False}, (inst, "log_softmax off")
        assert seen(lambda c: (c.lsm, c.smoothing)) >= {(True, 0.0), (True, 0.1)}
    for C in WIDTHS:
        assert {c.gather for c in CASES if c.C == C and c.lsm} == set(GATHERS), C
    pairs = lambda f: {f(c) for c in CASES if c.lsm}
    assert len(pairs(lambda c: (c.gather, c.smoothing, c.grads))) == 18 and len(pairs(lambda c: (c.gather, c.scale))) == 6
    assert {c.smoothing for c in CASES if not c.lsm} == {0.0, 0.1}
    for C in (1, 64):                                   # rows-per-wave edges at G = 1 and G = 64
        G, _, _, rpb = head_route(C)
        assert G == C and {c.n_out for c in CASES if c.C == C} >= {1, rpb + 1}
    for v in (N_SRC, N_OUT):
        assert all(v % (64 // G) and v % (4 * (64 // G)) for G in GROUPS if G < 64) and v % 4
    fwd_plain, fwd_faces, bwd_cap = STRIDE_CASES
    for c in (fwd_plain, fwd_faces) + tuple(GPU_ONLY_CASES):
        assert c.lsm and c.n_out > HEAD_BLOCKS * head_route(c.C)[3], c
    assert fwd_plain.gather == "none" and fwd_plain.smoothing > 0 and fwd_faces.gather == "faces"
    assert bwd_cap.n_src > BWD_BLOCKS * head_route(bwd_cap.C)[3] and head_route(bwd_cap.C)[1] > 1 and bwd_cap.grads == "both"
    assert head_route(GPU_ONLY_CASES[0].C)[0] < 64
    assert len({case_id(c) for c in CASES + STRIDE_CASES + GPU_ONLY_CASES}) == len(CASES + STRIDE_CASES + GPU_ONLY_CASES)


# ------------------------------------------------------------------------------------------------------------------------------
# the gather pattern
# ------------------------------------------------------------------------------------------------------------------------------
DOUBLED = 3                   # the output that names one vertex twice


def build_pattern(n_src, n_out, n_per, seed=0):
    """[n_out, n_per] int64: HUB in every output (its place rotates), UNUSED in none, the last vertex in the last output only, output DOUBLED
    with one vertex twice (the hub, on an edge), everything else drawn from the remaining vertices."""
    rng = np.random.RandomState(seed + 31 * n_per)
    others = np.array([v for v in range(n_src - 1) if v != HUB and v not in UNUSED])

    def stream():                                       # permutation after permutation: every other vertex is referenced once the draws suffice
        while True:
            for v in rng.permutation(others):
                yield int(v)
    draw = stream()
    idx = np.empty((n_out, n_per), dtype=np.int64)
    for i in range(n_out):
        row = []
        while len(row) < n_per - 1:
            v = next(draw)
            if v not in row:
                row.append(v)
        if i == min(DOUBLED, n_out - 1):
            row = [HUB] if n_per == 2 else [row[0]] * 2
        if i == n_out - 1:
            row[-1] = n_src - 1
        row.insert(i % n_per, HUB)
        idx[i] = row
    return torch.from_numpy(idx)


def check_pattern():
    for n_per in (2, 3):
        idx = build_pattern(N_SRC, N_OUT, n_per)
        deg = torch.bincount(idx.reshape(-1), minlength=N_SRC)
        assert bool((idx == HUB).any(1).all()) and len({int(r.tolist().index(HUB)) for r in idx}) == n_per, "the hub, in every place"
        assert int(deg[HUB]) >= N_OUT and all(int(deg[v]) == 0 for v in UNUSED) and 0 in UNUSED
        assert int((deg == 0).sum()) == len(UNUSED), "only the two chosen vertices are unreferenced"
        doubled = [i for i, r in enumerate(idx.tolist()) if len(set(r)) < n_per]
        assert doubled == [DOUBLED], doubled
        assert int(deg[N_SRC - 1]) == 1 and N_SRC - 1 in idx[N_OUT - 1].tolist()
        assert int(idx.min()) >= 0 and int(idx.max()) == N_SRC - 1
        rows = 64 // 8                                  # in a wave of eight 8-lane groups the hub's count sits beside a zero and beside small ones
        assert int(deg[:rows].max()) == int(deg[HUB]) and int(deg[:rows].min()) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# inputs, the call, torch's evaluation
# ------------------------------------------------------------------------------------------------------------------------------
Spec = collections.namedtuple("Spec", "x idx labels lsm smoothing grads d_logp via")     # via: "head" (ops.HeadFn) | "nll" (utils.nll_loss)

_PATTERNS = {}


def make_spec(case):
    g = torch.Generator().manual_seed(7 * case.C + 1000 * GATHERS[case.gather] + case.n_out)
    x = torch.randn(case.n_src, case.C, generator=g) * case.scale
    if not case.lsm:
        x = torch.log_softmax(x.double(), -1).float()
    idx = None if case.gather == "none" else build_pattern(case.n_src, case.n_out, GATHERS[case.gather])
    labels = torch.randint(0, case.C, (case.n_out,), generator=g)
    labels[::7] = -100
    if case.n_out == 1:
        labels[0] = 0
    d_logp = torch.randn(case.n_out, case.C, generator=g)       # not constant: a constant would hide an error in the row sum
    return Spec(x, idx, labels, case.lsm, case.smoothing, case.grads, d_logp, "head")


def pattern(dev, idx, n_src):
    """The packed GatherPattern of ``idx`` on ``dev``: built once, never modified."""
    if idx is None:
        return None
    from diffusion_net.batch import GatherPattern
    key = (str(dev), n_src, tuple(idx.shape), int(idx.sum()))
    if key not in _PATTERNS:
        _PATTERNS[key] = GatherPattern(idx.to(dev), n_src)
    return _PATTERNS[key]


def call_head(dev, spec):
    """One forward and one backward on ``dev`` -> (logp, loss | None, d_x) on the host.  With only the loss wanted the graded call returns no
    log-probabilities (the backward then has no incoming d_logp): they come from a second, ungraded call."""
    from diffusion_net import ops, utils
    use_loss, use_lp = spec.grads in ("loss", "both"), spec.grads in ("logp", "both")
    xa = spec.x.clone().to(dev).requires_grad_(True)
    pat = pattern(dev, spec.idx, spec.x.shape[0])
    lab = spec.labels.to(dev)
    if spec.via == "nll":
        assert not spec.lsm and spec.smoothing == 0.0 and spec.grads == "loss" and pat is None
        lp, loss = None, utils.nll_loss(xa, lab)
    else:
        lp, loss = ops.HeadFn.apply(xa, pat, lab if use_loss else None, spec.lsm, spec.smoothing, use_lp)
    outs = ([loss] if use_loss else []) + ([lp] if use_lp else [])
    grads = ([torch.tensor(G_LOSS, device=dev)] if use_loss else []) + ([spec.d_logp.to(dev)] if use_lp else [])
    torch.autograd.backward(outs, grads)
    if lp is None:
        with torch.no_grad():
            lp = ops.HeadFn.apply(xa.detach(), pat, lab, spec.lsm, spec.smoothing, True)[0]
    c = lambda t: None if t is None else t.detach().cpu()
    return c(lp), c(loss), c(xa.grad)


def smoothing32(s):
    return float(torch.tensor(s, dtype=torch.float32))          # the kernel's argument is a float


def loss_terms(lp, labels, s):
    """-> (term [n_out], rows that count).  The smoothed cross entropy of every row, the other classes summed over c != t and not at all
    at smoothing 0 -- what F.nll_loss computes there, and the label-smoothing formula wherever that is finite."""
    C = lp.shape[1]
    keep = (labels >= 0) & (labels < C)
    t = labels.clamp(0, C - 1)[:, None]
    at = lp.gather(1, t)[:, 0]
    if s == 0.0:
        return -at, keep
    off = smoothing32(s) / (C - 1) if C > 1 else 0.0
    oth = lp.masked_fill(torch.zeros_like(lp, dtype=torch.bool).scatter_(1, t, True), 0.0).sum(1)
    return -((1.0 - smoothing32(s)) * at + off * oth), keep


def torch_head(spec, dtype):
    """torch's evaluation at ``dtype`` on the host, gradients by autograd -> (logp, loss | None, d_x)."""
    use_loss, use_lp = spec.grads in ("loss", "both"), spec.grads in ("logp", "both")
    x = spec.x.clone().to(dtype).requires_grad_(True)
    z = x if spec.idx is None else x[spec.idx].mean(1)
    lp = torch.log_softmax(z, -1) if spec.lsm else z
    loss = None
    outs, grads = [], []
    if use_loss:
        term, keep = loss_terms(lp, spec.labels, spec.smoothing)
        loss = term[keep].sum() / keep.sum()
        outs.append(loss); grads.append(torch.tensor(G_LOSS, dtype=dtype))
    if use_lp:
        outs.append(lp); grads.append(spec.d_logp.to(dtype))
    torch.autograd.backward(outs, grads)
    return lp.detach(), None if loss is None else loss.detach(), x.grad


def bounds(spec, blocks_cap=HEAD_BLOCKS):
    """fp64 -> (logp bound [n_out, 1], loss bound | None, d_x bound [n_src, C]) as derived in the module docstring."""
    use_loss, use_lp = spec.grads in ("loss", "both"), spec.grads in ("logp", "both")
    n_src, C = spec.x.shape
    _, cpl, _, rpb = head_route(C)
    x = spec.x.double()
    idx = spec.idx if spec.idx is not None else torch.arange(n_src)[:, None]
    n_out, n_per = idx.shape
    z = x[idx].mean(1)
    zabs = x.abs()[idx].mean(1)
    M = torch.where(torch.isfinite(zabs), zabs, torch.zeros_like(zabs)).max(1).values
    lp = torch.log_softmax(z, -1) if spec.lsm else z
    lse = torch.logsumexp(z, -1).abs() if spec.lsm else torch.zeros(n_out, dtype=torch.float64)
    B = EPS * ((n_per + 3) * M + lse + cpl / 2.0 + 8.0)
    b_loss = None
    dlp = spec.d_logp.double() if use_lp else torch.zeros(n_out, C, dtype=torch.float64)
    if use_loss:
        term, keep = loss_terms(lp, spec.labels, spec.smoothing)
        blocks = min(-(-n_out // rpb), blocks_cap)
        n_iter = -(-n_out // (blocks * rpb))
        b_loss = B[keep].mean() + EPS * (n_iter + 20) * term[keep].abs().mean()
        s = smoothing32(spec.smoothing)
        target = torch.full((n_out, C), s / (C - 1) if C > 1 else 0.0, dtype=torch.float64)
        target.scatter_(1, spec.labels.clamp(0, C - 1)[:, None], 1.0 - s)
        dlp = dlp - (G_LOSS / float(keep.sum())) * target * keep[:, None]
    p = lp.exp() if spec.lsm else torch.zeros_like(lp)
    q = dlp.abs() + p * dlp.abs().sum(1, keepdim=True)
    lp_p = torch.where(p > 0, lp.abs() * p, torch.zeros_like(p))
    prop = (B[:, None] * p + EPS * lp_p + TINY) * dlp.sum(1, keepdim=True).abs()
    S, P = torch.zeros(n_src, C, dtype=torch.float64), torch.zeros(n_src, C, dtype=torch.float64)
    for j in range(n_per):
        S.index_add_(0, idx[:, j], q)
        P.index_add_(0, idx[:, j], prop)
    deg = torch.bincount(idx.reshape(-1), minlength=n_src).double()[:, None]
    return B[:, None], b_loss, (EPS * (deg + cpl / 2.0 + 8.0) * S + P) / n_per


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 any difference counts as infinite."""
    err = (torch.as_tensor(got).double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if not bool(torch.isnan(r).any()) else float("nan")


def judge(dev, spec, name, record=True):
    """The kernel and torch's fp32 evaluation against fp64, each as measured / bound -> ({quantity: ratio}, the kernel's results)."""
    ref_lp, ref_loss, ref_dx = torch_head(spec, torch.float64)
    t_lp, t_loss, t_dx = torch_head(spec, torch.float32)
    b_lp, b_loss, b_dx = bounds(spec)
    got_lp, got_loss, got_dx = call_head(dev, spec)
    exact_lp = not spec.lsm and spec.idx is None                 # the head copies its input
    if exact_lp:
        b_lp = torch.zeros_like(b_lp)
    res, t32 = {}, {}
    for key, got, t, ref, b in (("logp", got_lp, t_lp, ref_lp, b_lp), ("loss", got_loss, t_loss, ref_loss, b_loss), ("d_x", got_dx, t_dx, ref_dx, b_dx)):
        if ref is None:
            continue
        finite = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), finite) and torch.equal(torch.isfinite(t), finite), key + ": finite where fp64 is"
        z = lambda a: torch.where(finite, a.double(), torch.zeros_like(ref))      # (-inf log-probabilities of a masked class compare equal)
        same = bool((got[~finite].double() == ref[~finite]).all()) if bool((~finite).any()) else True
        assert same, key + ": another non-finite value than fp64"
        res[key], t32[key] = ratio(z(got), z(ref), b), ratio(z(t), z(ref), b)
    print("head %s: measured / bound %s; torch fp32 %s" % (name, {k: "%.3g" % v for k, v in res.items()}, {k: "%.3g" % v for k, v in t32.items()}))
    if record:
        helpers.record_margin("head_ops", dev, name=name, route=list(head_route(spec.x.shape[1])[:3]), unit="measured / bound",
                              **res, **{"torch32_" + k: v for k, v in t32.items()})
    wrong = {k: v for k, v in t32.items() if not v <= 1.0}
    assert not wrong, ("torch's own fp32 evaluation misses the bound: the bound is wrong", name, wrong)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (name, bad)
    if spec.idx is not None:
        unref = torch.bincount(spec.idx.reshape(-1), minlength=spec.x.shape[0]) == 0
        assert bool((got_dx[unref] == 0.0).all()), "a vertex nobody references has a gradient"
    return res, (got_lp, got_loss, got_dx)


def run_case(dev, case):
    return judge(dev, make_spec(case), case_id(case))


# ------------------------------------------------------------------------------------------------------------------------------
# non-finite and extreme inputs
# ------------------------------------------------------------------------------------------------------------------------------
NONFINITE_C = (5, 129)        # eight lanes a row, one class per lane; 64 lanes, three classes per lane
ROWS = 23
INF = float("inf")


def _plain(C, rows=ROWS, seed=0, gather="none"):
    g = torch.Generator().manual_seed(100 * C + seed)
    n_src = rows if gather == "none" else N_SRC
    n_out = rows if gather == "none" else N_OUT
    x = torch.randn(n_src, C, generator=g) * 2.0
    labels = torch.randint(0, C, (n_out,), generator=g)
    labels[::7] = -100
    idx = None if gather == "none" else build_pattern(n_src, n_out, GATHERS[gather])
    return x, idx, labels, torch.randn(n_out, C, generator=g)


def run_masked_class(dev, C, route):
    """The last class masked with -inf in every row (``route`` "head": logits, log_softmax on; "head_faces": the same through the face gather;
    "nll": the resulting log-probabilities through utils.nll_loss), no label on it, smoothing 0: loss and gradients are finite and inside the
    bounds of the ordinary cases."""
    x, idx, labels, d_logp = _plain(C, gather="faces" if route == "head_faces" else "none")
    x[:, C - 1] = -INF
    labels = torch.where(labels == C - 1, torch.zeros_like(labels), labels)
    if route == "nll":
        spec = Spec(torch.log_softmax(x.double(), -1).float(), None, labels, False, 0.0, "loss", d_logp, "nll")
    else:
        spec = Spec(x, idx, labels, True, 0.0, "both", d_logp, "head")
    _, (lp, loss, dx) = judge(dev, spec, "masked-class-C%d-%s" % (C, route))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all()), (float(loss), int((~torch.isfinite(dx)).sum()))
    assert bool((lp[:, C - 1] == -INF).all())
    if route == "head":                                 # p = 0 there: the incoming gradient passes through untouched
        assert torch.equal(dx[:, C - 1], d_logp[:, C - 1])


def run_nll_of_log_zero(dev):
    """log(0) among the probabilities, outside the target: F.nll_loss gives 0.458."""
    from diffusion_net import utils
    lp = torch.log(torch.tensor([[0.5, 0.5, 0.0], [0.2, 0.0, 0.8]]))
    lab = torch.tensor([0, 2])
    ref = float(torch.nn.functional.nll_loss(lp.double(), lab))
    a = lp.to(dev).requires_grad_(True)
    got = utils.nll_loss(a, lab.to(dev))
    got.backward()
    assert abs(float(got.detach()) - ref) <= 4 * EPS * ref, (float(got.detach()), ref)
    assert torch.equal(a.grad.cpu(), torch.tensor([[-0.5, 0.0, 0.0], [0.0, 0.0, -0.5]]))


def extreme_row(C):
    return torch.tensor([3e38, -3e38, 0.0, 1.0, 2.0] + [float(k % 3) for k in range(C - 5)])


def run_extreme_row(dev, C, target):
    """A row [3e38, -3e38, 0, 1, 2, ...] among ordinary rows: the loss is +inf exactly where torch's is and never NaN; log-probabilities and
    gradient are infinite / NaN exactly where torch's are."""
    x, _, labels, d_logp = _plain(C)
    x[2] = extreme_row(C)
    labels[2] = target
    spec = Spec(x, None, labels, True, 0.0, "both", d_logp, "head")
    lp, loss, dx = call_head(dev, spec)
    t_lp, t_loss, t_dx = torch_head(spec, torch.float32)
    ref = torch.nn.functional.nll_loss(torch.log_softmax(x, -1), labels)
    assert bool(torch.isinf(ref)) == bool(torch.isinf(t_loss)) == (target == 1)
    assert not bool(torch.isnan(loss)) and bool(torch.isinf(loss)) == bool(torch.isinf(ref)), (float(loss), float(ref))
    assert not bool(torch.isinf(loss)) or float(loss) > 0
    for name, a, b in (("logp", lp, t_lp), ("d_x", dx, t_dx)):
        assert torch.equal(torch.isinf(a), torch.isinf(b)) and torch.equal(torch.isnan(a), torch.isnan(b)), name
    assert bool(torch.isinf(lp[2, 1])) and int(torch.isinf(lp).sum()) == 1


def run_target_masked(dev, C, smoothing, lsm):
    """-inf in the target class of one row (a logit, or a given log-probability): the loss is +inf, with and without smoothing."""
    x, _, labels, d_logp = _plain(C)
    if not lsm:
        x = torch.log_softmax(x.double(), -1).float()
    labels[4] = 1
    x[4, 1] = -INF
    loss = call_head(dev, Spec(x, None, labels, lsm, smoothing, "loss", d_logp, "head"))[1]
    assert float(loss) == INF, float(loss)
    assert float(torch_head(Spec(x, None, labels, lsm, smoothing, "loss", d_logp, "head"), torch.float32)[1]) == INF


def run_poison(dev, C, value, gather):
    """+inf or NaN in one logit: the loss is NaN as torch's is, the rows that read the value are NaN, and every other row of the
    log-probabilities and of the gradient is bitwise what the same call gives without it."""
    x, idx, labels, d_logp = _plain(C, gather=gather)
    spec = Spec(x, idx, labels, True, 0.0, "both", d_logp, "head")
    if idx is None:
        at = 4
        rows_hit = torch.zeros(x.shape[0], dtype=torch.bool); rows_hit[at] = True
        src_hit = rows_hit
    else:
        at = int(idx[1, (1 % idx.shape[1] + 1) % idx.shape[1]])       # a vertex of output 1 (labelled) that is not the hub
        assert at != HUB and at not in UNUSED
        rows_hit = (idx == at).any(1)
        src_hit = torch.zeros(x.shape[0], dtype=torch.bool); src_hit[idx[rows_hit].reshape(-1)] = True
        assert 0 < int(rows_hit.sum()) < idx.shape[0] and bool(src_hit[HUB]) and not bool(src_hit.all())
    assert bool((labels[rows_hit] >= 0).any())
    dirty = x.clone()
    dirty[at, 1] = value
    lp0, loss0, dx0 = call_head(dev, spec)
    lp1, loss1, dx1 = call_head(dev, spec._replace(x=dirty))
    assert bool(torch.isfinite(loss0)) and bool(torch.isnan(loss1))
    assert bool(torch.isnan(torch_head(spec._replace(x=dirty), torch.float32)[1]))
    assert bool(torch.isnan(lp1[rows_hit]).all()), "the rows that read the value"
    assert torch.equal(lp1[~rows_hit], lp0[~rows_hit]), "log-probabilities of rows that do not read the value"
    assert torch.equal(dx1[~src_hit], dx0[~src_hit]), "gradient rows of vertices that share no output with the value"
    assert bool(torch.isnan(dx1[src_hit]).any(1).all()), "gradient rows of the vertices that do"


def run_nan_in_ignored_row(dev, C):
    """A NaN in a row labelled -100: the loss is finite and equal to the loss with that row's logits replaced by zeros."""
    x, _, labels, d_logp = _plain(C)
    assert int(labels[7]) == -100
    dirty, zeroed = x.clone(), x.clone()
    dirty[7, 2] = float("nan")
    zeroed[7] = 0.0
    spec = Spec(x, None, labels, True, 0.0, "loss", d_logp, "head")
    a, b = call_head(dev, spec._replace(x=dirty))[1], call_head(dev, spec._replace(x=zeroed))[1]
    assert bool(torch.isfinite(a)) and torch.equal(a, b), (float(a), float(b))


def run_all_ignored(dev, C):
    """Every row labelled -100: the loss is NaN (0 / 0) and the gradient exactly zero, as in torch."""
    x, _, labels, d_logp = _plain(C)
    spec = Spec(x, None, torch.full_like(labels, -100), True, 0.0, "loss", d_logp, "head")
    _, loss, dx = call_head(dev, spec)
    xt = x.clone().requires_grad_(True)
    ref = torch.nn.functional.nll_loss(torch.log_softmax(xt, -1), spec.labels)
    ref.backward()
    assert bool(torch.isnan(ref)) and bool((xt.grad == 0).all())
    assert bool(torch.isnan(loss)) and bool((dx == 0.0).all())


def run_single_class(dev, gather, smoothing):
    """C = 1: log-probabilities, loss and gradient are exactly 0."""
    x, idx, labels, d_logp = _plain(1, gather=gather)
    lp, loss, dx = call_head(dev, Spec(x, idx, labels, True, smoothing, "both", d_logp, "head"))
    assert bool((lp == 0.0).all()) and float(loss) == 0.0 and bool((dx == 0.0).all()), (float(lp.abs().max()), float(loss), float(dx.abs().max()))


def run_denormal(dev, C):
    """Logits x 1e-40, all denormal in fp32: the loss is log C within the loss bound (flushed to zero or not)."""
    x, _, labels, d_logp = _plain(C)
    spec = Spec(x * 1e-40, None, labels, True, 0.0, "both", d_logp, "head")
    assert 0 < float(spec.x.abs().max()) < 2.0 ** -126
    _, (_, loss, _) = judge(dev, spec, "denormal-C%d" % C)
    assert abs(float(loss) - math.log(C)) <= float(bounds(spec)[1]) + 1e-38, float(loss)


BAD_LABELS = ("C", -1, 2 ** 40)       # 2^40: its low 32 bits are 0, a class -- the label must not be truncated to int32


def run_bad_label(dev, C, bad, via):
    """A label that is neither a class nor -100: the loss is NaN."""
    x, _, labels, d_logp = _plain(C)
    labels[5] = C if bad == "C" else bad
    if via == "nll":
        spec = Spec(torch.log_softmax(x, -1), None, labels, False, 0.0, "loss", d_logp, "nll")
    else:
        spec = Spec(x, None, labels, True, 0.0, "loss", d_logp, "head")
    assert bool(torch.isnan(call_head(dev, spec)[1])), bad
    labels[5] = 0
    assert bool(torch.isfinite(call_head(dev, spec._replace(labels=labels))[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------------------------------------
DETERMINISM_CASES = {"faces": Case(65, "faces", True, 0.1, "both", 2.0, N_SRC, N_OUT), "stride": STRIDE_CASES[1], "stride_bwd_cap": STRIDE_CASES[2]}


def run_determinism(dev, which):
    """Two calls on the same inputs, and a third after a head call of another shape has used the workspace: loss, log-probabilities and
    gradient are bitwise equal."""
    spec = make_spec(DETERMINISM_CASES[which])
    first = call_head(dev, spec)
    second = call_head(dev, spec)
    other = call_head(dev, make_spec(Case(8, "none", True, 0.0, "both", 2.0, 300, 300)))
    third = call_head(dev, spec)
    assert bool(torch.isfinite(other[1]))
    for name, a, b, c in zip(("logp", "loss", "d_x"), first, second, third):
        assert torch.equal(a, b), name + ": second call"
        assert torch.equal(a, c), name + ": after an unrelated call"


# ------------------------------------------------------------------------------------------------------------------------------
# mass mean
# ------------------------------------------------------------------------------------------------------------------------------
MM_SIZES = (16, 17, 31, 32, 33, 63, 64, 65, 129, 700)       # around 4 RL = 16 and 32 rows, and many trips
MM_C = (1, 31, 32, 33, 64, 65, 130)
_MM = {}


def mass_batch(dev):
    if str(dev) not in _MM:
        meshes, _ = make_ragged(MM_SIZES, 8, 3, seed=4)
        g = torch.Generator().manual_seed(11)
        for m in meshes:
            v = int(m["mass"].shape[0])
            mass = 10.0 ** (6.0 * torch.rand(v, generator=g) - 3.0)           # six decades
            mass[0], mass[v - 1] = 1e-3, 1e3
            m["mass"] = mass.to(m["mass"].dtype)
        _MM[str(dev)] = (pack(meshes, dev, with_grad=False), torch.cat([m["mass"].float() for m in meshes]))
    return _MM[str(dev)]


def run_mass_mean(dev, C):
    from diffusion_net import ops
    mb, mass = mass_batch(dev)
    assert torch.equal(mb.mass.cpu(), mass)
    vt, nm = sum(MM_SIZES), len(MM_SIZES)
    g = torch.Generator().manual_seed(50 + C)
    x = torch.randn(vt, C, generator=g) + 100.0
    d_out = torch.randn(nm, C, generator=g)
    RL = 256 // (32 if C <= 32 else 64)

    def call(xin):
        xa = xin.clone().to(dev).requires_grad_(True)
        out = ops.MassMeanFn.apply(xa, mb)
        out.backward(d_out.to(dev))
        return out.detach().cpu(), xa.grad.cpu()
    out, dx = call(x)
    worst = {"fwd": 0.0, "bwd": 0.0, "torch32_fwd": 0.0, "torch32_bwd": 0.0}
    lo = 0
    for k, n in enumerate(MM_SIZES):
        m6, x6 = mass[lo:lo + n].double()[:, None], x[lo:lo + n].double()
        ref, scale = (m6 * x6).sum(0) / m6.sum(), (m6 * x6.abs()).sum(0) / m6.sum()
        b_f = gamma(-(-n // (4 * RL)) + RL + 6) * scale
        ref_b = d_out[k].double()[None] * m6 / m6.sum()
        b_b = 4 * EPS * ref_b.abs()
        m32, x32 = mass[lo:lo + n][:, None], x[lo:lo + n]
        t_f, t_b = (m32 * x32).sum(0) / m32.sum(), d_out[k][None] * (m32 / m32.sum())
        for key, got, r, b in (("fwd", out[k], ref, b_f), ("bwd", dx[lo:lo + n], ref_b, b_b), ("torch32_fwd", t_f, ref, b_f), ("torch32_bwd", t_b, ref_b, b_b)):
            worst[key] = max(worst[key], ratio(got, r, b))
        lo += n
    print("mass mean C=%d: measured / bound %s" % (C, {k: "%.3g" % v for k, v in worst.items()}))
    helpers.record_margin("mass_mean", dev, C=C, sizes=list(MM_SIZES), unit="measured / bound", **worst)
    assert worst["torch32_fwd"] <= 1.0 and worst["torch32_bwd"] <= 1.0, ("torch's own fp32 evaluation misses the bound: the bound is wrong", worst)
    assert worst["fwd"] <= 1.0 and worst["bwd"] <= 1.0, worst
    again = call(x)
    assert torch.equal(out, again[0]) and torch.equal(dx, again[1]), "run to run"
    dirty = x.clone()
    planted, row = 3, sum(MM_SIZES[:3]) + 5
    dirty[row, C // 2] = float("nan")
    out_d, _ = call(dirty)
    others = torch.arange(nm) != planted
    assert torch.equal(out_d[others], out[others]), "a NaN in one mesh changed another mesh's mean"
    assert bool(torch.isnan(out_d[planted, C // 2])) and int(torch.isnan(out_d).sum()) == 1


# ------------------------------------------------------------------------------------------------------------------------------
# checksum
# ------------------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
CK_LENGTHS = (1, 3, 4, 5, 255, 256, 257, 4099, 70001)
CK_OFFSETS = (0, 4, 8, 12)
_CK_MODEL = {}


def mix64(z):
    z ^= z >> 30; z = z * 0xbf58476d1ce4e5b9 & M64
    z ^= z >> 27; z = z * 0x94d049bb133111eb & M64
    return z ^ (z >> 31)


def checksum_model(words, salt):
    """dn_pack.hip's checksum of a list of unsigned 32-bit words, in Python integers -> (lane 0, lane 1)."""
    k0, k1 = mix64((salt + 0x9E3779B97F4A7C15) & M64), mix64(salt ^ 0xD1B54A32D192ED03)
    s0 = s1 = 0
    for i, w in enumerate(words):
        v = ((i << 32) & M64) ^ (i >> 32) ^ w
        s0 += mix64(v ^ k0)
        s1 += mix64(((v + k1) & M64) * 0xff51afd7ed558ccd & M64)
    return s0 & M64, s1 & M64


def ck_data(n):
    t = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=torch.Generator().manual_seed(n), dtype=torch.int64).to(torch.int32)
    if n > 2:
        t[1], t[n - 1] = 0, -1
    return t


def ck_expected(n, salt):
    if (n, salt) not in _CK_MODEL:
        _CK_MODEL[(n, salt)] = checksum_model(ck_data(n).numpy().view(np.uint32).tolist(), salt)
    return _CK_MODEL[(n, salt)]


def ck_view(dev, n, offset):
    """The words of ``ck_data(n)`` on ``dev``, their first byte ``offset`` bytes past a 16-byte boundary."""
    base = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    first = (-(base.data_ptr() % 16) // 4) % 4 + offset // 4
    v = base[first:first + n]
    v.copy_(ck_data(n))
    assert v.data_ptr() % 16 == offset and v.is_contiguous()
    return v


def _lanes(acc):
    return tuple(int(a) & M64 for a in acc.cpu().tolist())


def run_checksum_single(dev, n, offset):
    from diffusion_net import _hip
    v = ck_view(dev, n, offset)
    salt = 4 * n + 1
    acc = torch.zeros(2, dtype=torch.int64, device=dev)
    _hip.check(_hip.lib().dn_checksum128(v.data_ptr(), 4 * n, salt, acc.data_ptr(), _hip.stream_of(v)), "dn_checksum128")
    assert _lanes(acc) == ck_expected(n, salt), (n, offset)


def run_checksum_multi(dev, offset):
    """One 70001-word operand with operands shorter than one workgroup's share of it (their later workgroups leave at once) and an empty one,
    every operand ``offset`` bytes past a 16-byte boundary: the wrapping sum of the model's values."""
    import ctypes as C
    from diffusion_net import _hip
    lengths = (255, 70001, 1, 0, 257, 4099, 5)
    views = [ck_view(dev, n, offset) if n else None for n in lengths]
    salts = [4 * i + 3 for i in range(len(lengths))]
    nb = min(48, -(-max(lengths) // (256 * 16)))
    assert nb > 1 and all(n <= (nb - 1) * 256 for n in lengths if n != max(lengths)), "no operand with an idle workgroup"
    acc = torch.zeros(2, dtype=torch.int64, device=dev)
    k = len(lengths)
    _hip.check(_hip.lib().dn_checksum128_multi(k, (C.c_void_p * k)(*[v.data_ptr() if v is not None else None for v in views]),
                                               (C.c_size_t * k)(*[4 * n for n in lengths]), (C.c_uint64 * k)(*salts), acc.data_ptr(),
                                               _hip.stream_of(views[0])), "dn_checksum128_multi")
    want = [ck_expected(n, s) for n, s in zip(lengths, salts) if n]
    assert _lanes(acc) == (sum(w[0] for w in want) & M64, sum(w[1] for w in want) & M64), offset

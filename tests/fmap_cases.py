"""Shared bodies of the functional-map tests (drivers: test_fmap_emu.py on the emulator build of dn_fmap.hip, test_fmap_gpu.py on the device,
test_fmap_host.py for the torch routes of ``diffusion_net.fmaps``).

Two yardsticks, neither tuned to what the code gives:
  * the op in isolation (``ops.fmap_solve``, forward and backward under a random dC) against the formula evaluated in fp64 on the same fp32
    operands: max |got - ref| <= 2^-23 max |ref| -- the one rounding at the store, 2^-24, doubled; the fp64 solve's own error at the
    condition numbers asserted here (<= 1e6) is below 1e-9 and disappears under it.  (lam travels through the C ABI as a float: the
    operand the op sees, and so the one the formula gets, is 1e-3 rounded to fp32.)
  * ``fmaps.compute_correspondence`` / ``fmaps.functional_map`` against the reference's own fp64 output and gradients recorded in
    tests/golden/geom_fmap_ref.npz: max |got - C64| <= 4 max |C32_ref - C64|, the reference's own fp32 evaluation being the scale (the
    factor 4 of the linear tests' "within torch's own fp32 evaluation"); for the two feature gradients the fp32 evaluation is torch's fp32
    autograd of this package's torch route on the host.
Every body first asserts, in fp64 on the host, that max_i cond(G + lam D_i) <= 1e6: a condition on the inputs, not a measurement."""
import os

import numpy as np
import torch

import helpers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAM = 1e-3
LAM32 = float(np.float32(LAM))          # what a C float holds of it
COND_MAX = 1e6
OP_BOUND = 2.0 ** -23

# (K, F, P): the smallest shapes at which the kernels can still go wrong -- one row, fewer rows than a gram workgroup owns, an odd row count
# (the second wave of the last solve workgroup idles), F below K (singular G), F past a multiple of the 32-wide tiles, several pairs, K at
# the limit
CASES = [(1, 1, 1), (5, 3, 1), (30, 128, 1), (30, 16, 1), (30, 131, 3), (31, 40, 2), (64, 70, 1)]


def spectral_inputs(V, K, F, seed):
    """One pair of shapes as the fixture builds them: mass, a basis with Phi^T M Phi = I, eigenvalues sorted in [0, 100] with the first
    exactly 0 on both shapes and no two closer than a quarter grid step, features.  fp32 tensors."""
    rs = np.random.RandomState(seed)
    out = {}
    for s, shift in (("x", 0.0), ("y", 0.5)):
        mass = rs.uniform(0.5, 1.5, V) / V
        q, _ = np.linalg.qr(rs.randn(V, K))
        evals = 100.0 * (np.arange(K) + shift + 0.25 * rs.uniform(0.0, 1.0, K)) / K
        evals[0] = 0.0
        out["mass_" + s] = torch.from_numpy(mass.astype(np.float32))
        out["evecs_" + s] = torch.from_numpy((q / np.sqrt(mass)[:, None]).astype(np.float32))
        out["evals_" + s] = torch.from_numpy(evals.astype(np.float32))
        out["feat_" + s] = torch.from_numpy(rs.randn(V, F).astype(np.float32))
    return out


def op_inputs(K, F, P, seed=0):
    """A, B [P, K, F], evals_x, evals_y [P, K] fp32: the spectral coefficients of P seeded pairs of shapes."""
    A, B, ex, ey = [], [], [], []
    for p in range(P):
        t = spectral_inputs(K + 10, K, F, 1000 * seed + 10 * K + p)
        A.append((t["evecs_x"].double().t() @ (t["mass_x"].double()[:, None] * t["feat_x"].double())).float())
        B.append((t["evecs_y"].double().t() @ (t["mass_y"].double()[:, None] * t["feat_y"].double())).float())
        ex.append(t["evals_x"])
        ey.append(t["evals_y"])
    return torch.stack(A), torch.stack(B), torch.stack(ex), torch.stack(ey)


def systems64(A, B, evals_x, evals_y, lam):
    """The K systems of every pair in fp64: M [P, K, K, K] (M[p, i] = G + lam D_i) and H [P, K, K]."""
    A, B, evals_x, evals_y = A.double(), B.double(), evals_x.double(), evals_y.double()
    G, H = A @ A.transpose(-1, -2), B @ A.transpose(-1, -2)
    D = (evals_x[:, None, :] - evals_y[:, :, None]) ** 2
    return G[:, None] + lam * torch.diag_embed(D), H


def formula64(A, B, evals_x, evals_y, lam):
    """c_i = (G + lam D_i)^-1 H[i, :]^T in fp64, from the formula; differentiable."""
    M, H = systems64(A, B, evals_x, evals_y, lam)
    return torch.linalg.solve(M, H[..., None])[..., 0]


def assert_condition(A, B, evals_x, evals_y, lam=LAM):
    M, _ = systems64(A.detach().cpu(), B.detach().cpu(), evals_x.detach().cpu(), evals_y.detach().cpu(), lam)
    cond = float(torch.linalg.cond(M).max())
    assert cond <= COND_MAX, "the inputs are worse conditioned than the tests allow: %.3e" % cond
    return cond


def _share(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def run_case(dev, K, F, P):
    """One row of the case table on the kernels: forward, and backward under a random dC, against the formula in fp64."""
    from diffusion_net import ops
    A, B, ex, ey = op_inputs(K, F, P)
    cond = assert_condition(A, B, ex, ey)
    dC = torch.randn(P, K, K, generator=torch.Generator().manual_seed(K * F + P))
    a64, b64 = A.double().requires_grad_(True), B.double().requires_grad_(True)
    ref = formula64(a64, b64, ex, ey, LAM32)
    ref.backward(dC.double())
    a, b = A.to(dev).requires_grad_(True), B.to(dev).requires_grad_(True)
    got = ops.fmap_solve(a, b, ex.to(dev), ey.to(dev), LAM)
    assert tuple(got.shape) == (P, K, K) and got.dtype == torch.float32
    got.backward(dC.to(dev))
    shares = dict(c=_share(got, ref.detach()), d_a=_share(a.grad, a64.grad), d_b=_share(b.grad, b64.grad))
    print("fmap op K=%d F=%d P=%d: cond %.2e; max |got - ref| / max |ref|: C %.3e, dA %.3e, dB %.3e (bound %.3e)" % (
        K, F, P, cond, shares["c"], shares["d_a"], shares["d_b"], OP_BOUND))
    helpers.record_margin("fmap_k%d_f%d_p%d" % (K, F, P), dev, cond=cond, bound=OP_BOUND, **shares)
    assert max(shares.values()) <= OP_BOUND, shares
    if P == 1:                                    # the unbatched call is the same launch
        one = ops.fmap_solve(A[0].to(dev), B[0].to(dev), ex[0].to(dev), ey[0].to(dev), LAM)
        assert tuple(one.shape) == (K, K) and torch.equal(one, got.detach()[0])


def run_determinism(dev):
    """Two calls on the same inputs are the same bits, forward and backward (several pairs, F past a tile)."""
    from diffusion_net import ops
    A, B, ex, ey = (t.to(dev) for t in op_inputs(30, 131, 3))
    dC = torch.randn(3, 30, 30, generator=torch.Generator().manual_seed(3)).to(dev)
    outs = []
    for _ in range(2):
        a, b = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
        C = ops.fmap_solve(a, b, ex, ey, LAM)
        C.backward(dC)
        outs.append((C.detach(), a.grad, b.grad))
    for x, y in zip(*outs):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y)


def run_singular_row(dev):
    """Pair 0 has A = 0 and evals_x[0] == evals_y[0] == 0: G + lam D_0 has a zero pivot.  That row of C is NaN and the rest finite; the
    status word counts 1; check=True raises; the backward fills that pair's gradients with NaN and leaves the other pair's finite."""
    import pytest
    from diffusion_net import ops
    A, B, ex, ey = op_inputs(5, 3, 2)
    A[0] = 0.0
    assert float(ex[0, 0]) == 0.0 and float(ey[0, 0]) == 0.0
    A, B, ex, ey = (t.to(dev) for t in (A, B, ex, ey))
    a, b = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
    C = ops.fmap_solve(a, b, ex, ey, LAM)
    nan = torch.isnan(C.detach()).cpu()
    want = torch.zeros(2, 5, 5, dtype=torch.bool)
    want[0, 0] = True
    assert torch.equal(nan, want) and bool(torch.isfinite(C.detach().cpu()[~want]).all())
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ops.fmap_solve_fwd(A, B, ex, ey, LAM, status)
    assert int(status.item()) == 1
    with pytest.raises(RuntimeError, match="1 row"):
        ops.fmap_solve(A, B, ex, ey, LAM, check=True)
    ops.fmap_solve(A[1], B[1], ex[1], ey[1], LAM, check=True)          # a regular pair passes the check
    C.backward(torch.ones_like(C))
    for g in (a.grad.cpu(), b.grad.cpu()):
        assert bool(torch.isnan(g[0]).all()) and bool(torch.isfinite(g[1]).all())


def run_limits(dev):
    """K = 65 is past the kernel: ``ops.fmap_solve`` raises, ``fmaps`` takes the torch route; shape, dtype and device errors."""
    import pytest
    from diffusion_net import fmaps, ops
    A, B, ex, ey = (t.to(dev) for t in op_inputs(65, 20, 1))
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        ops.fmap_solve(A, B, ex, ey, LAM)
    got = fmaps.solve(A, B, ex, ey, LAM)
    ref = formula64(A.cpu(), B.cpu(), ex.cpu(), ey.cpu(), LAM)
    cond = assert_condition(A, B, ex, ey)
    # fp32 LU on systems of condition `cond`: first-order bound K * 2^-24 * cond on the relative error of a solve
    assert _share(got, ref) <= 65 * 2.0 ** -24 * cond
    A, B, ex, ey = (t.to(dev) for t in op_inputs(5, 3, 1))
    with pytest.raises(ValueError, match="square maps"):
        ops.fmap_solve(A, B, ex[:, :4], ey, LAM)
    with pytest.raises(ValueError, match="one shape"):
        ops.fmap_solve(A, B[:, :, :2], ex, ey, LAM)
    with pytest.raises(TypeError, match="fp32"):
        ops.fmap_solve(A.double(), B, ex, ey, LAM)
    with pytest.raises(ValueError, match="not for the eigenvalues"):
        ops.fmap_solve(A, B, ex.clone().requires_grad_(True), ey, LAM)
    if torch.device(dev).type != "cpu":
        with pytest.raises(RuntimeError):
            ops.fmap_solve(A, B.cpu(), ex, ey, LAM)
    empty = ops.fmap_solve(A[:0], B[:0], ex[:0], ey[:0], LAM, check=True)
    assert tuple(empty.shape) == (0, 5, 5)


# ------------------------------------------------------------------------------------------------ the reference's recorded outputs
def golden_cases():
    z = np.load(os.path.join(GOLDEN, "geom_fmap_ref.npz"))
    assert float(z["lam"]) == LAM
    for name in z["cases"]:
        name = str(name)
        yield name, {key.split("/", 1)[1]: torch.from_numpy(z[key]) for key in z.files if key.startswith(name + "/")}


def _trans(t, s, K, dtype, dev):
    """evecs^T diag(mass) of the first K eigenvectors without the V x V matrix."""
    return (t["evecs_" + s][:, :K].to(dtype).t() * t["mass_" + s].to(dtype)[None, :]).to(dev).contiguous()


def _call(how, t, dtype, dev):
    """-> (C [K, K], feat_x, feat_y) of one fixture case through ``how`` in ('compute_correspondence', 'functional_map', 'ops')."""
    from diffusion_net import fmaps, ops
    K = t["evals_x"].shape[0]
    fx, fy = (t[k].to(dtype).to(dev).requires_grad_(True) for k in ("feat_x", "feat_y"))
    ex, ey = t["evals_x"].to(dtype).to(dev), t["evals_y"].to(dtype).to(dev)
    if how == "functional_map":
        C = fmaps.functional_map(fx, fy, t["mass_x"].to(dtype).to(dev), t["mass_y"].to(dtype).to(dev), ex, ey,
                                 t["evecs_x"].to(dtype).to(dev), t["evecs_y"].to(dtype).to(dev), n_fmap=K, lambda_param=LAM)
    elif how == "compute_correspondence":
        C = fmaps.compute_correspondence(fx, fy, ex, ey, _trans(t, "x", K, dtype, dev), _trans(t, "y", K, dtype, dev), lambda_param=LAM)
        assert tuple(C.shape) == (1, K, K)
        C = C[0]
    else:
        C = ops.fmap_solve(_trans(t, "x", K, dtype, dev) @ fx, _trans(t, "y", K, dtype, dev) @ fy, ex, ey, LAM)
    assert tuple(C.shape) == (K, K) and C.dtype == dtype
    return C, fx, fy


def _with_grads(how, t, dtype, dev):
    C, fx, fy = _call(how, t, dtype, dev)
    ((C - t["c_gt"].to(dtype).to(dev)) ** 2).mean().backward()
    return C.detach().cpu().double(), fx.grad.cpu().double(), fy.grad.cpu().double()


def fixture_condition(t):
    K = t["evals_x"].shape[0]
    A = _trans(t, "x", K, torch.float64, "cpu") @ t["feat_x"].double()
    B = _trans(t, "y", K, torch.float64, "cpu") @ t["feat_y"].double()
    return assert_condition(A[None], B[None], t["evals_x"][None], t["evals_y"][None])


def run_reference_fixture(dev, how, names=None):
    """fp32 results of ``how`` on the fixture's inputs against the reference's fp64 output and gradients, on the scale of the fp32 evaluations."""
    ran = 0
    for name, t in golden_cases():
        if names is not None and name not in names:
            continue
        cond = fixture_condition(t)
        C64, gx64, gy64 = t["C_f64"], t["grad_feat_x_f64"], t["grad_feat_y_f64"]
        _, gx32, gy32 = _torch_host_fp32(t)
        C, gx, gy = _with_grads(how, t, torch.float32, dev)
        rows = (("c", C, C64, t["C_f32"].double()), ("d_feat_x", gx, gx64, gx32), ("d_feat_y", gy, gy64, gy32))
        rec = {}
        for what, got, r64, r32 in rows:
            rec[what], rec[what + "_fp32_eval"] = float((got - r64).abs().max()), float((r32 - r64).abs().max())
        print("fmap fixture %s via %s: cond %.2e; max |got - ref64| vs max |fp32 evaluation - ref64|: %s" % (
            name, how, cond, ", ".join("%s %.3e / %.3e" % (w, rec[w], rec[w + "_fp32_eval"]) for w, *_ in rows)))
        helpers.record_margin("fmap_fixture_%s_%s" % (name, how), dev, cond=cond, scale_c=float(C64.abs().max()), **rec)
        for what, *_ in rows:
            assert rec[what] <= 4.0 * rec[what + "_fp32_eval"], (name, what, rec)
        ran += 1
    assert ran == (len(names) if names is not None else 8)


def _torch_host_fp32(t):
    """torch's fp32 autograd of this package's torch route on the host: the fp32 evaluation the gradients are measured against."""
    from diffusion_net import fmaps
    K = t["evals_x"].shape[0]
    fx, fy = t["feat_x"].clone().requires_grad_(True), t["feat_y"].clone().requires_grad_(True)
    A, B = _trans(t, "x", K, torch.float32, "cpu") @ fx, _trans(t, "y", K, torch.float32, "cpu") @ fy
    C = fmaps._solve_torch(A, B, t["evals_x"], t["evals_y"], LAM)
    ((C - t["c_gt"]) ** 2).mean().backward()
    return C.detach().double(), fx.grad.double(), fy.grad.double()


# ------------------------------------------------------------------------------------------------ C ABI on host buffers
def run_abi_errors():
    """Every non-zero return of dn_fmap_solve_*_f32, through ctypes, on host buffers: nothing is launched, the outputs keep their fill; the
    workspace query is honoured to the byte."""
    from diffusion_net import _hip
    L = _hip.lib()
    assert L.dn_fmap_max_k() == 64 == _hip.FMAP_MAX_K
    K, F, P = 5, 3, 2
    A, B, ex, ey = op_inputs(K, F, P)
    dC = torch.randn(P, K, K, generator=torch.Generator().manual_seed(1))
    big = torch.randn(1, 65, 4)
    C = torch.full((P, K, K), -7.0)
    dA, dB = torch.full((P, K, F), -7.0), torch.full((P, K, F), -7.0)
    ws = torch.zeros(1 << 20, dtype=torch.uint8)
    status = torch.full((1,), -7, dtype=torch.int32)
    need = L.dn_fmap_workspace_bytes(P, K, F)
    assert need >= 4 * P * K * K * 8 and L.dn_fmap_workspace_bytes(0, K, F) == 0
    p = _hip.ptr

    def fwd(a=A, b=B, x=ex, y=ey, P_=P, K_=K, F_=F, c=C, w=ws, wb=ws.numel()):
        return L.dn_fmap_solve_fwd_f32(p(a), p(b), p(x), p(y), P_, K_, F_, LAM, p(c), p(w), wb, p(status), None)

    def bwd(a=A, b=B, x=ex, y=ey, d=dC, P_=P, K_=K, F_=F, da=dA, db=dB, w=ws, wb=ws.numel()):
        return L.dn_fmap_solve_bwd_f32(p(a), p(b), p(x), p(y), p(d), P_, K_, F_, LAM, p(da), p(db), p(w), wb, p(status), None)

    for call in (fwd, bwd):
        assert call(K_=0) != 0                              # K < 1
        assert call(a=big, b=big, K_=65, F_=4, P_=1) != 0   # K > dn_fmap_max_k()
        assert call(F_=0) != 0                              # F < 1
        assert call(P_=-1) != 0                             # P < 0
        assert call(a=None) != 0 and call(b=None) != 0 and call(x=None) != 0 and call(y=None) != 0   # a NULL operand while P > 0
        assert call(w=None) != 0                            # no workspace
        assert call(wb=need - 1) != 0                       # a workspace smaller than the query says
    assert fwd(c=None) != 0 and bwd(d=None) != 0 and bwd(da=None) != 0 and bwd(db=None) != 0
    assert fwd(P_=0) == 0 and bwd(P_=0) == 0                # P == 0: success, nothing launched
    assert fwd(a=None, b=None, x=None, y=None, c=None, w=None, wb=0, P_=0) == 0
    for t in (C, dA, dB):
        assert bool((t == -7.0).all())
    assert int(status) == -7
    assert fwd(wb=need) == 0 and bwd(wb=need) == 0          # the exact size is enough
    assert int(status) == 0
    L.dn_fmap_solve_fwd_f32(p(A), p(B), p(ex), p(ey), P, K, F, LAM, p(C), p(ws), need, None, None)   # status may be NULL
    a64, b64 = A.double().requires_grad_(True), B.double().requires_grad_(True)
    ref = formula64(a64, b64, ex, ey, LAM32)
    ref.backward(dC.double())
    assert max(_share(C, ref.detach()), _share(dA, a64.grad), _share(dB, b64.grad)) <= OP_BOUND

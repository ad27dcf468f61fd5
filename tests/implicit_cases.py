"""Shared bodies of the implicit-diffusion tests (test_implicit_host.py: the numpy route; test_implicit_emu.py: the emulator build of
dn_implicit.hip on host buffers; test_implicit_gpu.py: the device).

Yardstick, never the code under test: for every (mesh, channel) ``numpy.linalg.solve`` in fp64 on diag(m) + t_c L.toarray(), with the same
fp32-rounded m, L and u the op receives; for the gradients torch autograd in fp64 through ``torch.linalg.solve`` on the same operands.

Forward bound, a priori, per (mesh, channel), 2-norms over that mesh's rows, x* the yardstick:

    ||x - x*|| <= rtol ||m u|| / min(m) + 2^-24 ||x*||                                                         =: BX

(A = diag(m) + t L has lambda_min >= min m and the solver stops at ||r|| <= rtol ||m u||, so ||x - x*|| = ||A^-1 r|| <= the first term; the
second is the fp32 store.)

Backward bounds.  The backward solves A g = d_x with the same solver, so the fp64 g~ it holds has ||g~ - g*|| <= rtol ||d_x|| / min(m) =: EG.
  d_u = fp32(m g~):                  ||d_u - m g*|| <= max(m) EG + 2^-24 ||m g*||                              per (mesh, channel)
  d_t[c] = - sum_b g~_bc . (L_b x~_bc) with x~ the saved fp32 x (||x~ - x*|| <= BX):
      |d_t - d_t*| <= sum_b ||L_b||_2 (EG_b (||x*_b|| + BX_b) + ||g*_b|| BX_b) + 2^-24 |d_t*|                  per channel
(Cauchy-Schwarz on (g~ - g*) . L x~ and g* . L (x~ - x*); the last term is the fp32 store; the fp64 sums are far below both.)"""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import helpers

U32 = 2.0 ** -24
TIMES = (1e-8, 1e-4, 1e-2, 0.1, 1.0)
RTOL, MAX_ITER = 1e-10, 200
WIDTHS = (1, 5, 64, 65, 130)
FAMILIES = ("sphere300", "sphere300_mass6", "sphere300_chan", "graph200", "ragged", "tile_edges")


def rows_per_tile():
    from diffusion_net import _hip
    r = _hip.lib().dn_implicit_rows_per_tile()
    assert 2 <= r <= 1024
    return r


def times(C):
    return np.resize(np.array(TIMES, dtype=np.float32), C)


def _sphere(V, seed=3):
    """(L scipy CSR fp32 with sorted columns, m fp32) of ``synthetic.sphere_mesh(V, seed)``: host cotan L and vertex areas."""
    from diffusion_net import precompute as P, synthetic
    v, f = synthetic.sphere_mesh(V, seed=seed)
    L = sp.csr_matrix(P.cotan_laplacian(v, f, 1e-10)).astype(np.float32)
    L.sort_indices()
    return L, P.vertex_areas(v, f).astype(np.float32)


def _graph200():
    """A weighted graph Laplacian D - W on 200 nodes: a hub (node 3) with about 100 neighbours, an empty row (node 7: no entry at all, not
    even the diagonal) and a diagonal-only row (node 11: one entry, 0.5)."""
    n, rng = 200, np.random.RandomState(5)
    W = np.where(rng.rand(n, n) < 0.03, rng.uniform(0.1, 2.0, (n, n)), 0.0)
    W[3, rng.choice(n, 100, replace=False)] = rng.uniform(0.1, 2.0, 100)
    W = np.triu(W, 1)
    W = W + W.T
    W[[7, 11], :] = 0.0
    W[:, [7, 11]] = 0.0
    d = W.sum(axis=1)
    d[11] = 0.5
    L = sp.csr_matrix(np.diag(d) - W).astype(np.float32)          # (from dense: zeros are not stored, row 7 has no entry)
    L.sort_indices()
    lens = np.diff(L.indptr)
    assert lens[7] == 0 and lens[11] == 1 and lens[3] >= 90, (lens[7], lens[11], lens[3])
    return L, rng.uniform(0.5, 1.5, n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def family(name):
    """(L scipy CSR fp32 block diagonal, m fp32, sizes), never modified."""
    if name in ("sphere300", "sphere300_chan"):
        L, m = _sphere(300)
        sizes = [300]
    elif name == "sphere300_mass6":
        L, m = _sphere(300)
        m = (m.astype(np.float64) * 10.0 ** np.random.RandomState(6).uniform(-3, 3, 300)).astype(np.float32)
        sizes = [300]
    elif name == "graph200":
        L, m = _graph200()
        sizes = [200]
    elif name in ("ragged", "small", "tile_edges", "v1"):
        if name == "tile_edges":
            r = rows_per_tile()
            sizes = [r - 1, r, r + 1, 2 * r + 1]
        else:
            sizes = {"ragged": [40, 150, 300, 1], "small": [70, 40, 1], "v1": [1]}[name]       # small: two tiles, one tile, one row
        parts = [(sp.csr_matrix((1, 1), dtype=np.float32), np.array([0.5], dtype=np.float32)) if v == 1 else _sphere(v) for v in sizes]
        L = sp.csr_matrix(sp.block_diag([p[0] for p in parts], format="csr")).astype(np.float32)
        L.sort_indices()
        m = np.concatenate([p[1] for p in parts])
    else:
        raise KeyError(name)
    L.data.setflags(write=False)
    m.setflags(write=False)
    return L, m, tuple(sizes)


@functools.lru_cache(maxsize=None)
def rhs(name, C):
    V = family(name)[0].shape[0]
    u = np.random.RandomState(100 + C).randn(V, C).astype(np.float32)
    if name == "sphere300_chan":
        u = (u * (2.0 ** np.where(np.arange(C) % 2 == 0, 20.0, -20.0))[None, :]).astype(np.float32)
    u.setflags(write=False)
    return u


def segments(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(off[i]), int(off[i + 1])) for i in range(len(sizes))]


def dense_solve(L, m, t, b, sizes):
    """A_bc^-1 b_bc in fp64 with ``numpy.linalg.solve``, mesh by mesh and channel by channel."""
    Ld, m64 = L.toarray().astype(np.float64), m.astype(np.float64)
    out = np.empty(b.shape, dtype=np.float64)
    for lo, hi in segments(sizes):
        for c in range(b.shape[1]):
            out[lo:hi, c] = np.linalg.solve(np.diag(m64[lo:hi]) + float(t[c]) * Ld[lo:hi, lo:hi], b[lo:hi, c].astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name, C):
    L, m, sizes = family(name)
    x = dense_solve(L, m, times(C), m.astype(np.float64)[:, None] * rhs(name, C).astype(np.float64), sizes)
    x.setflags(write=False)
    return x


def mesh_norms(a, sizes):
    """2-norms per (mesh, channel) of a [V, C] array."""
    return np.stack([np.linalg.norm(a[lo:hi].astype(np.float64), axis=0) for lo, hi in segments(sizes)])


def forward_bound(name, C, rtol=RTOL):
    L, m, sizes = family(name)
    m64 = m.astype(np.float64)
    mmin = np.array([m64[lo:hi].min() for lo, hi in segments(sizes)])[:, None]
    return rtol * mesh_norms(m64[:, None] * rhs(name, C), sizes) / mmin + U32 * mesh_norms(yardstick(name, C), sizes)


def device_operands(name, C, dev):
    L, m, sizes = family(name)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return (t(L.indptr.astype(np.int32)), t(L.indices.astype(np.int32)), t(L.data), t(m), t(times(C)), t(rhs(name, C)), list(sizes))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def solve(name, C, dev, **kw):
    from diffusion_net import ops
    kw.setdefault("rtol", RTOL)
    kw.setdefault("max_iter", MAX_ITER)
    x, info = ops.implicit_solve(*device_operands(name, C, dev), return_info=True, **kw)
    V = family(name)[0].shape[0]
    n_mesh = len(family(name)[2])
    assert tuple(x.shape) == (V, C) and x.dtype == torch.float32 and x.device.type == torch.device(dev).type
    assert tuple(info["iterations"].shape) == tuple(info["residual"].shape) == (n_mesh, C)
    assert info["iterations"].dtype == torch.int32 and info["residual"].dtype == torch.float64
    return x, info


def check_forward(name, C, dev, x, info, form="check", rtol=RTOL, record=True):
    """Every (mesh, channel) against the bound; the solver's own residual at or below rtol; the cap."""
    sizes = family(name)[2]
    err = mesh_norms(x.detach().cpu().numpy().astype(np.float64) - yardstick(name, C), sizes)
    share = float((err / forward_bound(name, C, rtol)).max())
    its, res = info["iterations"].cpu().numpy(), info["residual"].cpu().numpy()
    print("implicit_solve %s C=%d %s on %s: worst error %.3f of the bound, iterations %d .. %d, residual <= %.2e, %d launches"
          % (name, C, form, dev, share, its.min(), its.max(), res.max(), info["launches"]))
    if record:
        helpers.record_margin("implicit_solve", dev, family=name, C=C, form=form, rtol=rtol, share_of_bound=share, iterations_min=int(its.min()),
                              iterations_max=int(its.max()), residual_max=float(res.max()), launches=int(info["launches"]))
    assert np.isfinite(x.detach().cpu().numpy()).all() and share <= 1.0, share
    assert (res <= rtol).all() and its.max() <= MAX_ITER
    return share


def run_family(name, dev, C=5):
    x, info = solve(name, C, dev)
    check_forward(name, C, dev, x, info)
    return x, info


@functools.lru_cache(maxsize=None)
def host_iterations(name, C):
    from diffusion_net import precompute as P
    L, m, sizes = family(name)
    _, info = P.implicit_diffusion_host(L, m, times(C), rhs(name, C), sizes, rtol=RTOL, max_iter=MAX_ITER, return_info=True)
    return info["iterations"]


def run_iteration_counts(name, dev):
    """``info["iterations"]`` per (mesh, channel) equals the numpy route's, plus or minus 1 (the last iteration sits on the tolerance)."""
    _, info = solve(name, 5, dev)
    got, want = info["iterations"].cpu().numpy().astype(np.int64), host_iterations(name, 5)
    print("iterations %s on %s: kernel %s numpy %s" % (name, dev, got.tolist(), want.tolist()))
    assert np.abs(got - want).max() <= 1, (got, want)
    assert got.max() <= MAX_ITER // 2, "the cap no longer leaves 2x room"


def run_call_forms(dev):
    """iters_per_check 1 and 16 and check=False at 200 and at 260 iterations: the same bits (freezing); x0 given; two runs bitwise equal."""
    from diffusion_net import ops
    name, C = "small", 5
    a, ia = solve(name, C, dev, iters_per_check=16)
    b, ib = solve(name, C, dev, iters_per_check=1)
    c, ic = solve(name, C, dev, check=False, max_iter=200)
    d, id_ = solve(name, C, dev, check=False, max_iter=260)
    e, _ = solve(name, C, dev, iters_per_check=16)
    check_forward(name, C, dev, a, ia, "check16")
    check_forward(name, C, dev, c, ic, "nocheck200")
    for other, what in ((b, "iters_per_check=1"), (c, "check=False, 200"), (d, "check=False, 260"), (e, "a second run")):
        assert torch.equal(bits(a), bits(other)), what
    for info in (ib, ic, id_):
        assert torch.equal(info["iterations"], ia["iterations"]) and torch.equal(info["residual"], ia["residual"])
    # launches: 2 (init) + 4 per iteration + 1 (the count) per group + 1 (finish); check=True stops at the first group that leaves nothing
    k = int(ia["iterations"].max())
    assert ia["launches"] == 3 + 65 * max(1, -(-k // 16)) and ib["launches"] == 3 + 5 * max(1, k)
    assert ic["launches"] == 3 + 4 * 200 + 1 and id_["launches"] == 3 + 4 * 260 + 1
    # x0 given: the yardstick itself (rounded to fp32) -- nearly nothing left to do -- and zeros
    ops_ = device_operands(name, C, dev)
    x0 = torch.from_numpy(yardstick(name, C).astype(np.float32)).to(dev)
    f, inf = ops.implicit_solve(*ops_, x0=x0, rtol=RTOL, max_iter=MAX_ITER, return_info=True)
    check_forward(name, C, dev, f, inf, "x0=yardstick")
    assert int(inf["iterations"].sum()) < int(ia["iterations"].sum())
    g, ing = ops.implicit_solve(*ops_, x0=torch.zeros_like(x0), rtol=RTOL, max_iter=MAX_ITER, return_info=True)
    check_forward(name, C, dev, g, ing, "x0=0")
    # every mesh of the batch alone: the same bits as inside the batch (tiles, norms and scalars are per mesh)
    L, m, sizes = family(name)
    for (lo, hi) in segments(sizes)[:2]:
        Ls = sp.csr_matrix(L[lo:hi, lo:hi])
        Ls.sort_indices()
        t = lambda arr: torch.from_numpy(np.array(arr)).to(dev)
        alone = ops.implicit_solve(t(Ls.indptr.astype(np.int32)), t(Ls.indices.astype(np.int32)), t(Ls.data.astype(np.float32)), t(m[lo:hi]),
                                   t(times(C)), t(rhs(name, C)[lo:hi]), rtol=RTOL, max_iter=MAX_ITER)
        assert torch.equal(bits(alone), bits(a[lo:hi])), "a mesh alone differs from the mesh inside the batch"


def run_max_iter_raises(dev):
    import pytest
    with pytest.raises(RuntimeError, match="did not reach rtol"):
        solve("sphere300", 5, dev, max_iter=1)


def run_isolation(dev):
    """A NaN planted in one mesh's u leaves the other meshes bitwise untouched; a NaN in one channel leaves the other channels untouched."""
    from diffusion_net import ops
    name, C, n_it = "small", 5, 60                      # (both spheres are done well before 60 iterations; the bits are compared at 60)
    rowptr, col, val, m, t, u, sizes = device_operands(name, C, dev)
    clean = ops.implicit_solve(rowptr, col, val, m, t, u, sizes, rtol=RTOL, max_iter=n_it, check=False)
    check_forward(name, C, dev, clean, ops.implicit_solve(rowptr, col, val, m, t, u, sizes, rtol=RTOL, max_iter=n_it, return_info=True)[1],
                  "nocheck60", record=False)
    seg = segments(sizes)
    lo, hi = seg[1]
    bad = u.clone()
    bad[lo + 3, :] = float("nan")
    got = ops.implicit_solve(rowptr, col, val, m, t, bad, sizes, rtol=RTOL, max_iter=n_it, check=False)
    assert bool(torch.isnan(got[lo:hi]).all()), "a NaN in u did not reach its whole system"
    keep = torch.ones(u.shape[0], dtype=torch.bool)
    keep[lo:hi] = False
    assert torch.equal(bits(got)[keep], bits(clean)[keep]), "a NaN in one mesh changed another mesh"
    others = [c for c in range(C) if c != 3]
    for planted in (float("nan"), float("inf")):
        bad = u.clone()
        bad[seg[0][0] + 5, 3] = planted
        got = ops.implicit_solve(rowptr, col, val, m, t, bad, sizes, rtol=RTOL, max_iter=n_it, check=False)
        assert torch.equal(bits(got)[:, others], bits(clean)[:, others]), "a non-finite value in one channel changed another channel"
        assert bool(torch.isnan(got[seg[0][0]:seg[0][1], 3]).all())
        assert torch.equal(bits(got)[keep_rows(seg, 0, u.shape[0]), 3], bits(clean)[keep_rows(seg, 0, u.shape[0]), 3])
    with __import__("pytest").raises(RuntimeError, match="did not reach rtol"):      # check=True sees the system that can never finish
        ops.implicit_solve(rowptr, col, val, m, t, bad, sizes, rtol=RTOL, max_iter=32)


def keep_rows(seg, mesh, V):
    keep = torch.ones(V, dtype=torch.bool)
    keep[seg[mesh][0]:seg[mesh][1]] = False
    return keep


# ------------------------------------------------------------------------------------------------------------------------------
# gradients
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_yardstick(name, C):
    """(w [V, C] fp32 the gradient of the output, d_u* [V, C], d_t* [C], g* [V, C]) in fp64 by torch autograd through ``torch.linalg.solve``."""
    L, m, sizes = family(name)
    w = np.random.RandomState(200 + C).randn(L.shape[0], C).astype(np.float32)
    Ld = torch.from_numpy(L.toarray().astype(np.float64))
    m64 = torch.from_numpy(m.astype(np.float64))
    u = torch.from_numpy(rhs(name, C).astype(np.float64)).requires_grad_(True)
    t = torch.from_numpy(times(C).astype(np.float64)).requires_grad_(True)
    loss = 0.0
    for lo, hi in segments(sizes):
        A = torch.diag(m64[lo:hi])[None] + t[:, None, None] * Ld[lo:hi, lo:hi][None]                    # [C, v, v]
        x = torch.linalg.solve(A, (m64[lo:hi, None] * u[lo:hi]).t().unsqueeze(-1)).squeeze(-1).t()      # [v, C]
        loss = loss + (x * torch.from_numpy(w[lo:hi].astype(np.float64))).sum()
    loss.backward()
    g = dense_solve(L, m, times(C), w, sizes)
    return w, u.grad.numpy(), t.grad.numpy(), g


def backward_bounds(name, C, rtol=RTOL):
    """(bound of d_u per (mesh, channel), bound of d_t per channel), as derived in the module docstring."""
    L, m, sizes = family(name)
    w, du, dt, g = grad_yardstick(name, C)
    m64 = m.astype(np.float64)
    seg = segments(sizes)
    mmin = np.array([m64[lo:hi].min() for lo, hi in seg])[:, None]
    mmax = np.array([m64[lo:hi].max() for lo, hi in seg])[:, None]
    lnorm = np.array([np.linalg.norm(L[lo:hi, lo:hi].toarray().astype(np.float64), 2) for lo, hi in seg])[:, None]
    EG = rtol * mesh_norms(w, sizes) / mmin
    BX = forward_bound(name, C, rtol)
    b_du = mmax * EG + U32 * mesh_norms(m64[:, None] * g, sizes)
    b_dt = (lnorm * (EG * (mesh_norms(yardstick(name, C), sizes) + BX) + mesh_norms(g, sizes) * BX)).sum(axis=0) + U32 * np.abs(dt)
    return b_du, b_dt


def check_backward(name, C, dev, d_u, d_t, what, rtol=RTOL):
    sizes = family(name)[2]
    w, du, dt, g = grad_yardstick(name, C)
    b_du, b_dt = backward_bounds(name, C, rtol)
    s_du = float((mesh_norms(d_u.detach().cpu().numpy().astype(np.float64) - du, sizes) / b_du).max())
    s_dt = float((np.abs(d_t.detach().cpu().numpy().astype(np.float64) - dt) / b_dt).max())
    print("%s %s C=%d on %s: d_u %.3f of its bound, d_t %.3f of its bound" % (what, name, C, dev, s_du, s_dt))
    helpers.record_margin("implicit_backward", dev, family=name, C=C, form=what, rtol=rtol, d_u_share_of_bound=s_du, d_t_share_of_bound=s_dt)
    assert s_du <= 1.0 and s_dt <= 1.0, (s_du, s_dt)
    return s_du, s_dt


def run_backward(name, dev, C=5):
    """``ops.ImplicitDiffusionFn``: forward and both gradients against the fp64 yardstick."""
    from diffusion_net import ops
    rowptr, col, val, m, t, u, sizes = device_operands(name, C, dev)
    op = ops.ImplicitOperator(rowptr, col, val, m, sizes)
    u, t = u.clone().requires_grad_(True), t.clone().requires_grad_(True)
    x = ops.ImplicitDiffusionFn.apply(u, t, op, RTOL, MAX_ITER)
    err = mesh_norms(x.detach().cpu().numpy().astype(np.float64) - yardstick(name, C), sizes)
    assert float((err / forward_bound(name, C)).max()) <= 1.0
    x.backward(torch.from_numpy(grad_yardstick(name, C)[0]).to(dev))
    check_backward(name, C, dev, u.grad, t.grad, "ImplicitDiffusionFn")


def run_custom_operator(dev):
    """``torch.ops.diffusion_net.implicit_solve`` (the check=False form) equals ``ops.implicit_solve``; its autograd formula meets the bounds."""
    from diffusion_net import ops, torchlib  # noqa: F401
    name, C, n_it = "small", 5, 64                      # (the check=False form: 64 iterations, both spheres are done before)
    rowptr, col, val, m, t, u, sizes = device_operands(name, C, dev)
    want, info = ops.implicit_solve(rowptr, col, val, m, t, u, sizes, rtol=RTOL, max_iter=n_it, check=False, return_info=True)
    check_forward(name, C, dev, want, info, "nocheck64", record=False)
    u, t = u.clone().requires_grad_(True), t.clone().requires_grad_(True)
    got = torch.ops.diffusion_net.implicit_solve(rowptr, col, val, m, t, u, sizes, None, RTOL, n_it)
    assert torch.equal(bits(got), bits(want))
    got.backward(torch.from_numpy(grad_yardstick(name, C)[0]).to(dev))
    check_backward(name, C, dev, u.grad, t.grad, "torch.ops.diffusion_net.implicit_solve")
    meta = lambda a: torch.empty(a.shape, dtype=a.dtype, device="meta")
    fake = torch.ops.diffusion_net.implicit_solve(meta(rowptr), meta(col), meta(val), meta(m), meta(t), meta(u), sizes, None, RTOL, n_it)
    assert tuple(fake.shape) == tuple(u.shape) and fake.dtype == torch.float32 and fake.device.type == "meta"


# ------------------------------------------------------------------------------------------------------------------------------
# refused C calls, op errors
# ------------------------------------------------------------------------------------------------------------------------------
def run_refused_calls(dev):
    """Every refused call returns non-zero and launches nothing: the sentinel in the output and the workspace survives."""
    from diffusion_net import _hip, ops
    Lb = _hip.lib()
    name, C = "sphere300", 5                            # one mesh of five tiles: a table of four cannot cover it
    rowptr, col, val, m, t, u, sizes = device_operands(name, C, dev)
    op = ops.ImplicitOperator(rowptr, col, val, m, sizes)
    V, nt, nm = op.V, op.n_tiles, op.n_mesh
    need = int(Lb.dn_implicit_workspace_bytes(V, C, nt, nm))
    assert need > 8 * 4 * V * C
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    out = torch.full((V, C), 7.25, dtype=torch.float32, device=dev)
    word = torch.full((1,), -5, dtype=torch.int32, device=dev)
    p = lambda a: a.data_ptr()

    def init(rp=p(rowptr), c=p(col), v=p(val), mass=p(m), time=p(t), tiles=p(op.tiles), n_tiles=nt, off=p(op.mesh_tile_off), n_mesh=nm, rows=V,
             width=C, rhs=p(u), rtol=RTOL, w=p(ws), wb=need):
        return Lb.dn_implicit_init_f32(rp, c, v, mass, time, tiles, n_tiles, off, n_mesh, rows, width, rhs, 1, None, rtol, w, wb, None)

    def iterate(rp=p(rowptr), tiles=p(op.tiles), n_tiles=nt, n_mesh=nm, rows=V, width=C, n=1, flag=p(word), w=p(ws), wb=need):
        return Lb.dn_implicit_iterate_f32(rp, p(col), p(val), p(m), p(t), tiles, n_tiles, p(op.mesh_tile_off), n_mesh, rows, width, n, flag, w, wb, None)

    def finish(tiles=p(op.tiles), n_tiles=nt, rows=V, width=C, o=p(out), w=p(ws), wb=need):
        return Lb.dn_implicit_finish_f32(p(m), tiles, n_tiles, p(op.mesh_tile_off), nm, rows, width, 0, o, None, None, w, wb, None)

    def lx_dot(rp=p(rowptr), n_tiles=nt, rows=V, width=C, x=p(u), dt=p(out), w=p(ws), wb=need):
        return Lb.dn_implicit_lx_dot_f32(rp, p(col), p(val), p(op.tiles), n_tiles, p(op.mesh_tile_off), nm, rows, width, x, dt, w, wb, None)

    too_wide = 65535 * 64 + 1
    refused = {
        "init": (init, dict(null_rowptr=dict(rp=None), null_col=dict(c=None), null_val=dict(v=None), null_mass=dict(mass=None), null_time=dict(time=None),
                            null_tiles=dict(tiles=None), null_off=dict(off=None), null_rhs=dict(rhs=None), null_ws=dict(w=None),
                            negative_rows=dict(rows=-1), negative_width=dict(width=-1), negative_tiles=dict(n_tiles=-1), negative_meshes=dict(n_mesh=-1),
                            small_ws=dict(wb=need - 1), too_wide=dict(width=too_wide), short_table=dict(n_tiles=nt - 1), nan_rtol=dict(rtol=float("nan")))),
        "iterate": (iterate, dict(null_rowptr=dict(rp=None), null_tiles=dict(tiles=None), null_flag=dict(flag=None), null_ws=dict(w=None),
                                  negative_iterations=dict(n=-1), negative_rows=dict(rows=-1), small_ws=dict(wb=need - 1), too_wide=dict(width=too_wide),
                                  short_table=dict(n_tiles=nt - 1))),
        "finish": (finish, dict(null_tiles=dict(tiles=None), null_out=dict(o=None), null_ws=dict(w=None), negative_width=dict(width=-1),
                                small_ws=dict(wb=need - 1), too_wide=dict(width=too_wide), short_table=dict(n_tiles=nt - 1))),
        "lx_dot": (lx_dot, dict(null_rowptr=dict(rp=None), null_x=dict(x=None), null_d_time=dict(dt=None), null_ws=dict(w=None),
                                negative_rows=dict(rows=-1), small_ws=dict(wb=need - 1), too_wide=dict(width=too_wide), short_table=dict(n_tiles=nt - 1))),
    }
    assert nm <= nt - 1 and (nt - 1) * rows_per_tile() < V, "the short table of this test must not be able to cover the rows"
    for call, (fn, cases) in refused.items():
        for what, kw in cases.items():
            assert fn(**kw) != 0, (call, what)
    assert Lb.dn_implicit_workspace_bytes(-1, C, nt, nm) == 0 and Lb.dn_implicit_workspace_bytes(V, too_wide, nt, nm) == 0
    assert init(rows=0, n_tiles=0, n_mesh=0) == 0 and init(width=0) == 0 and finish(width=0) == 0       # nothing to do: nothing launched
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert bool((ws == 0x5A).all()) and bool((out == 7.25).all()) and int(word) == -5, "a refused call wrote something"
    assert init() == 0 and iterate(n=0) == 0 and int(word) > 0 and iterate(n=100) == 0 and int(word) == 0 and finish() == 0
    err = mesh_norms(out.cpu().numpy().astype(np.float64) - yardstick(name, C), sizes)
    assert float((err / forward_bound(name, C)).max()) <= 1.0


def run_op_errors(dev):
    """``ops.implicit_solve`` raises before any launch."""
    import pytest
    from diffusion_net import ops
    rowptr, col, val, m, t, u, sizes = device_operands("ragged", 5, dev)
    V = u.shape[0]
    bad = col.clone()
    bad[1] = V
    with pytest.raises(ValueError, match="column index"):
        ops.implicit_solve(rowptr, bad, val, m, t, u, sizes)
    bad[1] = -1
    with pytest.raises(ValueError, match="column index"):
        ops.implicit_solve(rowptr, bad, val, m, t, u, sizes)
    badp = rowptr.clone()
    badp[-1] += 1
    with pytest.raises(ValueError, match="row pointer"):
        ops.implicit_solve(badp, col, val, m, t, u, sizes)
    with pytest.raises(ValueError, match="sizes"):
        ops.implicit_solve(rowptr, col, val, m, t, u, [V - 1])
    with pytest.raises(ValueError, match="sizes"):
        ops.implicit_solve(rowptr, col, val, m, t, u, [V, 0])
    with pytest.raises(TypeError):
        ops.implicit_solve(rowptr.long(), col, val, m, t, u, sizes)
    with pytest.raises(TypeError):
        ops.implicit_solve(rowptr, col, val.double(), m, t, u, sizes)
    with pytest.raises(TypeError):
        ops.implicit_solve(rowptr, col, val, m, t, u.double(), sizes)
    with pytest.raises(TypeError):
        ops.implicit_solve(rowptr, col, val, m, t[:4], u, sizes)
    with pytest.raises(TypeError):
        ops.implicit_solve(rowptr, col, val, m, t, u, sizes, x0=u[:, :4])
    with pytest.raises(ValueError):
        ops.implicit_solve(rowptr, col, val, m[:-1], t, u, sizes)
    with pytest.raises(ValueError):
        ops.implicit_solve(rowptr, col, val, m, t, u, sizes, iters_per_check=0)
    with pytest.raises(RuntimeError, match="no gradient"):
        ops.implicit_solve(rowptr, col, val, m.clone().requires_grad_(True), t, u, sizes)
    with pytest.raises(RuntimeError, match="no gradient"):
        ops.implicit_solve(rowptr, col, val.clone().requires_grad_(True), m, t, u, sizes)
    out, info = ops.implicit_solve(rowptr, col, val, m, t[:0], u[:, :0], sizes, return_info=True)
    assert tuple(out.shape) == (V, 0) and info["launches"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# LearnedTimeDiffusion / DiffusionNet with 'implicit_sparse'
# ------------------------------------------------------------------------------------------------------------------------------
def torch_sparse(L, dev):
    coo = sp.coo_matrix(L)
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)), torch.from_numpy(coo.data.astype(np.float32)),
                                   L.shape).coalesce().to(dev)


def run_layer(dev):
    """``LearnedTimeDiffusion("implicit_sparse")`` against the fp64 solve, forward and both gradients: within the bounds at the layer's default
    rtol, and no further from the yardstick than ``"implicit_dense"`` (fp32 Cholesky) on the same inputs; the in-place clamp is observed."""
    from diffusion_net import layers
    name, C = "sphere300", 5
    L, m, sizes = family(name)
    w, du, dt, g = grad_yardstick(name, C)
    # "implicit_dense" is the reference's torch code and runs on HOST tensors: ``torch.linalg.cholesky`` of that route raises
    # hipErrorLaunchFailure on gfx950 at [1, 5, 300, 300], and the fp32 Cholesky yardstick does not need the device
    Lt, mt = torch_sparse(L, dev), torch.from_numpy(np.array(m)).to(dev)
    L_host, m_host = torch_sparse(L, "cpu"), torch.from_numpy(np.array(m))

    def layer_with_gradients(method, where, L_, m_, batched):
        lay = layers.LearnedTimeDiffusion(C, method=method).to(where)
        assert lay.implicit_rtol == 1e-9 and lay.implicit_max_iter == 1000 and lay.implicit_check is True
        assert list(lay.state_dict()) == ["diffusion_time"]
        with torch.no_grad():
            lay.diffusion_time.copy_(torch.from_numpy(times(C)))
            lay.diffusion_time[0] = -1.0                              # clamped in place to 1e-8 = TIMES[0]
        u = torch.from_numpy(np.array(rhs(name, C))).to(where).requires_grad_(True)
        x = lay(u[None], L_.unsqueeze(0), m_[None], None, None)[0] if batched else lay(u, L_, m_, None, None)
        assert float(lay.diffusion_time.detach()[0]) == float(np.float32(1e-8)), "the clamp of diffusion_time is not observed"
        x.backward(torch.from_numpy(w).to(where))
        return tuple(a.detach().cpu().numpy().astype(np.float64) for a in (x, u.grad, lay.diffusion_time.grad))
    got = {"implicit_sparse": layer_with_gradients("implicit_sparse", dev, Lt, mt, False),
           "implicit_dense": layer_with_gradients("implicit_dense", "cpu", L_host, m_host, True)}      # (the dense route takes the batched form only)
    x, d_u, d_t = got["implicit_sparse"]
    assert float((mesh_norms(x - yardstick(name, C), sizes) / forward_bound(name, C, 1e-9)).max()) <= 1.0
    check_backward(name, C, dev, torch.from_numpy(d_u), torch.from_numpy(d_t), "LearnedTimeDiffusion", rtol=1e-9)
    for i, (what, ref) in enumerate((("x", yardstick(name, C)), ("d_u", du), ("d_t", dt))):
        es, ed = np.linalg.norm(got["implicit_sparse"][i] - ref), np.linalg.norm(got["implicit_dense"][i] - ref)
        print("layer %s on %s: implicit_sparse %.3e, implicit_dense %.3e from the fp64 solve" % (what, dev, es, ed))
        helpers.record_margin("implicit_layer", dev, quantity=what, sparse_error=float(es), dense_error=float(ed))
        assert es <= ed, (what, es, ed)
    # the batched form gives the same rows
    lay = layers.LearnedTimeDiffusion(C, method="implicit_sparse").to(dev)
    with torch.no_grad():
        lay.diffusion_time.copy_(torch.from_numpy(times(C)))
    u = torch.from_numpy(np.array(rhs(name, C))).to(dev)
    two = lay(torch.stack([u, u]), torch.stack([Lt, Lt]), torch.stack([mt, mt]), None, None)
    one = lay(u, Lt, mt, None, None)
    assert tuple(two.shape) == (2, 300, C) and torch.equal(bits(two[0]), bits(one)) and torch.equal(bits(two[1]), bits(one))
    import pytest
    with pytest.raises(RuntimeError, match="no gradient"):
        lay(u, Lt, mt.clone().requires_grad_(True), None, None)


def _net_operands(dev):
    from diffusion_net import geometry, synthetic
    v, f = synthetic.sphere_mesh(300, seed=3)
    verts, faces = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
    frames, mass, L, evals, evecs, gradX, gradY = geometry.compute_operators(verts, faces, 8)
    return verts, mass, L, gradX, gradY


def run_network(dev):
    import diffusion_net
    from diffusion_net import layers
    verts, mass, L, gradX, gradY = _net_operands(dev)

    def make(method):
        torch.manual_seed(11)
        net = layers.DiffusionNet(3, 5, C_width=32, N_block=2, diffusion_method=method, dropout=False).to(dev)
        with torch.no_grad():
            for blk in net.blocks:
                blk.diffusion.diffusion_time.copy_(torch.from_numpy(times(32)))
        return net

    sparse, dense, spectral = make("implicit_sparse"), make("implicit_dense"), make("spectral")
    assert list(sparse.state_dict()) == list(spectral.state_dict())
    sparse.load_state_dict(spectral.state_dict())                    # a spectral checkpoint loads into an implicit network
    kw = dict(L=L, evals=None, evecs=None, gradX=gradX, gradY=gradY)
    out = sparse(verts, mass, **kw)
    assert tuple(out.shape) == (300, 5) and bool(torch.isfinite(out).all())
    out.square().sum().backward()
    for k, p in sparse.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, k
    # the yardstick: the same network with the diffusion layer swapped for an fp64 dense solve (a torch function), the rest unchanged
    yard = make("implicit_sparse")

    def fp64_diffusion(lay):
        def forward(x, L_, mass_, evals_, evecs_):
            t = lay.diffusion_time.double().clamp(min=1e-8)
            Ld = L_.to_dense().double()
            Ld = Ld[None] if Ld.dim() == 2 else Ld                      # (an unbatched call hands L over as it is)
            A = torch.diag_embed(mass_.double())[:, None] + t[None, :, None, None] * Ld[:, None]     # [B, C, V, V]
            b = (x.double() * mass_.double().unsqueeze(-1)).transpose(1, 2).unsqueeze(-1)
            return torch.linalg.solve(A, b).squeeze(-1).transpose(1, 2).float()
        return forward
    for blk in yard.blocks:
        blk.diffusion.forward = fp64_diffusion(blk.diffusion)
    # the dense network's diffusion layers run the reference's torch code on host tensors (see run_layer), the rest of it on the device

    def dense_on_host(lay):
        twin = layers.LearnedTimeDiffusion(lay.C_inout, method="implicit_dense")
        with torch.no_grad():
            twin.diffusion_time.copy_(lay.diffusion_time.detach().cpu())
        return lambda x, L_, mass_, evals_, evecs_: twin(x.cpu(), L_.cpu(), mass_.cpu(), None, None).to(x.device)
    for blk in dense.blocks:
        blk.diffusion.forward = dense_on_host(blk.diffusion)
    with torch.no_grad():
        ref = yard(verts, mass, **kw).double()
        d_sparse = float((out.detach().double() - ref).norm())
        d_dense = float((dense(verts, mass, **kw).double() - ref).norm())
        print("network on %s: implicit_sparse %.3e, implicit_dense %.3e from the network with fp64 dense diffusion" % (dev, d_sparse, d_dense))
        helpers.record_margin("implicit_network", dev, sparse_distance=d_sparse, dense_distance=d_dense)
        assert d_sparse <= 2.0 * d_dense, (d_sparse, d_dense)
        # batched [B, V, C] and unbatched calls give the same rows
        one = out.detach()
        two = sparse(torch.stack([verts, verts]), torch.stack([mass, mass]), L=torch.stack([L, L]), evals=None, evecs=None,
                     gradX=torch.stack([gradX, gradX]), gradY=torch.stack([gradY, gradY]))
        assert tuple(two.shape) == (2, 300, 5)
        assert torch.equal(bits(two[0]), bits(one)) and torch.equal(bits(two[1]), bits(one))
    import pytest
    with pytest.raises(ValueError, match="invalid setting for diffusion_method"):
        layers.DiffusionNet(3, 5, diffusion_method="implicit")
    assert diffusion_net.layers.DiffusionNetBlock(8, [8], diffusion_method="implicit_sparse").diffusion.method == "implicit_sparse"

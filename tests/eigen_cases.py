"""Shared bodies of the eigenbasis tests (test_eigen_host.py: the numpy route; test_eigen_emu.py: the emulator build on host buffers;
test_eigen_gpu.py: the device).

1. The kernel, ``dn_cheb_step_f64`` / ``ops.cheb_step``:  out = alpha S Y + beta Y + gamma Z  against ``numpy.longdouble`` on the SAME CSR arrays.
   Bound, a priori, element by element: |got - ref| <= gamma_(n_i + 3) (|alpha| |S||Y| + |beta| |Y| + |gamma| |Z|), gamma_n = n u / (1 - n u),
   u = 2^-53, n_i the entries of row i -- n_i roundings of the fma chain, one of the product with alpha, one of each further fma.  Where the
   right side is 0 (an empty row with beta = gamma = 0) the result must be exactly 0.
2. The solver: every run is checked in numpy against its INPUTS (L, massvec) -- residual, M-orthonormality, eigenvalues against
   ``precompute.laplacian_eigenbasis`` (shift-invert eigsh), the subspace against eigsh's where the reference itself shows a gap, conventions.
   The eigsh reference of a mesh is computed once and shared by the tiers."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import helpers

U64 = 2.0 ** -53
NBS = (1, 8, 63, 64, 65, 160, 288)
PAD = 5                       # ld = nb + PAD in the padded cases
SENTINEL = 7.25               # what the padding of ``out`` holds before a call
UB, A = 209.5, 3.25           # the scalars of a filter on [A, UB]
C_, E_ = (UB + A) / 2.0, (UB - A) / 2.0
SCALARS = {"product": (1.0, 0.0, 0.0), "first": (1.0 / E_, -C_ / E_, 0.0), "recurrence": (2.0 / E_, -2.0 * C_ / E_, -1.0)}


def gamma(n):
    return n * U64 / (1.0 - n * U64)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the operator of the kernel cases
# ------------------------------------------------------------------------------------------------------------------------------
LENS = tuple(range(0, 41))
HUB_LEN, LAST_LEN, N_IRREGULAR, UNUSED = 310, 37, 403, 7


@functools.lru_cache(maxsize=None)
def irregular_csr(rpw):
    """403 x 403 CSR with sorted columns, ``rpw`` = rows per workgroup: row lengths 0 .. 40 in seeded order, an empty first row, the whole
    workgroup [2 rpw, 3 rpw) empty, a hub row of 310 entries (several fetch loops), a last row of 37, explicit zeros, column 7 unreferenced."""
    n = N_IRREGULAR
    rng = np.random.RandomState(17)
    lens = rng.permutation(np.resize(np.array(LENS), n))
    lens[0] = 0
    lens[2 * rpw:3 * rpw] = 0
    hub = 3 * rpw + 2
    lens[hub] = HUB_LEN
    lens[n - 1] = LAST_LEN
    others = np.array([c for c in range(n) if c != UNUSED])
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.sort(rng.choice(others, k, replace=False)) for k in lens if k] or [np.zeros(0, dtype=np.int64)])
    vals = rng.randn(rows.shape[0]) * 3.0
    vals[np.arange(rows.shape[0]) % 11 == 3] = 0.0
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    assert rowptr[-1] == cols.shape[0] and lens.max() == HUB_LEN and set(LENS) <= set(lens.tolist())
    assert lens[0] == 0 and not lens[2 * rpw:3 * rpw].any() and lens[-1] == LAST_LEN and UNUSED not in cols and (vals == 0).sum() > 10
    out = (rowptr.astype(np.int32), cols.astype(np.int32), vals.astype(np.float64))
    for a in out:
        a.setflags(write=False)
    return out


def small_csr(n, seed=23):
    """n x n: row lengths drawn from 0 .. min(n, 9), an empty first row from n = 2 on, the last row full."""
    rng = np.random.RandomState(seed + n)
    lens = rng.randint(0, min(n, 9) + 1, size=n)
    lens[0] = 0 if n > 1 else 1
    lens[n - 1] = min(n, 9) if n > 1 else 1
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens if k])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), cols.astype(np.int32), rng.randn(rows.shape[0])


def reference(csr, Y, Z, alpha, beta, gamma_):
    """(ref, bound) in ``numpy.longdouble`` from the CSR arrays as they are; a term whose scalar is 0 is not formed."""
    rowptr, col, val = csr
    ld = np.longdouble
    n, nb = Y.shape
    lens = np.diff(rowptr)
    rows = np.repeat(np.arange(n), lens)
    prod = val.astype(ld)[:, None] * Y.astype(ld)[col]
    s, sa = np.zeros((n, nb), dtype=ld), np.zeros((n, nb), dtype=ld)
    np.add.at(s, rows, prod)
    np.add.at(sa, rows, np.abs(prod))
    ref, scale = ld(alpha) * s, abs(ld(alpha)) * sa
    if beta != 0.0:
        ref, scale = ref + ld(beta) * Y.astype(ld), scale + abs(ld(beta)) * np.abs(Y.astype(ld))
    if gamma_ != 0.0:
        ref, scale = ref + ld(gamma_) * Z.astype(ld), scale + abs(ld(gamma_)) * np.abs(Z.astype(ld))
    g = np.array([gamma(int(k) + 3) for k in lens], dtype=ld)[:, None]
    return ref, g * scale


def block(values, ld_, dev, fill, misaligned=False):
    """``values`` [n, nb] as the leading columns of a block of leading dimension ``ld_`` on ``dev`` whose other columns hold ``fill``;
    ``misaligned``: the first element sits 8 bytes past a 16-byte boundary.  -> (view [n, nb], whole block [n, ld_])."""
    n, nb = values.shape
    buf = torch.empty(n * ld_ + 2, dtype=torch.float64, device=dev)
    off = ((buf.data_ptr() // 8) % 2) ^ (1 if misaligned else 0)
    whole = buf[off:off + n * ld_].view(n, ld_)
    assert whole.data_ptr() % 16 == (8 if misaligned else 0)
    whole.fill_(fill)
    whole[:, :nb] = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    return whole[:, :nb], whole


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def device_csr(csr, dev):
    return tuple(torch.from_numpy(np.array(a)).to(dev) for a in csr)


def run_step(dev, csr, nb, pad, form="recurrence", out_form="new", misaligned=False, seed=0, record=None):
    """One call through ``ops.cheb_step`` on blocks of leading dimension nb + pad (the padding of Y and Z is NaN, that of ``out`` a sentinel
    that must survive), checked against the bound.  ``out_form``: "new" (out=None), "given" (a pre-filled block), "z" (out is Z).
    Returns the result as numpy."""
    from diffusion_net import ops
    rowptr, col, val = csr
    n = rowptr.shape[0] - 1
    alpha, beta, gamma_ = SCALARS[form]
    rng = np.random.RandomState(1000 * nb + 7 * n + seed)
    Yh, Zh = rng.randn(n, nb), rng.randn(n, nb)
    d = device_csr(csr, dev)
    ld_ = nb + pad
    Y, Yw = block(Yh, ld_, dev, float("nan"), misaligned)
    Z, Zw = block(Zh, ld_, dev, float("nan"), misaligned)
    use_z = gamma_ != 0.0 or out_form == "z"
    if out_form == "z":
        before = bits(Zw)
        got = ops.cheb_step(*d, Y, Z, alpha, beta, gamma_, out=Z)
        assert got.data_ptr() == Z.data_ptr()
        after = bits(Zw)
        assert torch.equal(after[:, nb:], before[:, nb:]), "the padding of out (= Z) was written"
    elif out_form == "given":
        out, outw = block(np.full((n, nb), SENTINEL), ld_, dev, SENTINEL, misaligned)
        got = ops.cheb_step(*d, Y, Z if use_z else None, alpha, beta, gamma_, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert bool((outw[:, nb:] == SENTINEL).all()), "the padding of out was written"
    else:
        got = ops.cheb_step(*d, Y, Z if use_z else None, alpha, beta, gamma_)
        assert tuple(got.shape) == (n, nb) and got.dtype == torch.float64 and got.device.type == torch.device(dev).type
    if out_form != "z":
        assert torch.equal(bits(Zw)[:, :nb], bits(torch.from_numpy(Zh))), "Z was written"
    assert torch.equal(bits(Yw)[:, :nb], bits(torch.from_numpy(Yh))), "Y was written"
    got = got.detach().cpu().numpy().copy()
    ref, bound = reference(csr, Yh, Zh, alpha, beta, gamma_)
    err = np.abs(got.astype(np.longdouble) - ref)
    share = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))))
    print("cheb_step n=%d nb=%d ld=%d %s out=%s%s: worst error %.3f of the bound" % (n, nb, ld_, form, out_form, " misaligned" if misaligned else "", share))
    if record:
        helpers.record_margin("eigen_cheb_step", dev, n=n, nb=nb, ld=ld_, form=form, out=out_form, misaligned=bool(misaligned),
                              longest_row=int(np.diff(rowptr).max()), share_of_bound=share)
    assert np.isfinite(got).all() and share <= 1.0, share
    return got


def rows_per_workgroup():
    from diffusion_net import _hip
    r = _hip.lib().dn_cheb_rows_per_workgroup()
    assert 2 <= r <= 64
    return r


def run_shapes(dev, nb, pad):
    """The irregular operator at one block width: the recurrence step into a given block, the other two scalar sets into new ones."""
    csr = irregular_csr(rows_per_workgroup())
    run_step(dev, csr, nb, pad, "recurrence", "given", record=True)
    run_step(dev, csr, nb, pad, "product", "new", record=True)
    run_step(dev, csr, nb, pad, "first", "new", record=True)


def run_small_rows(dev, nb):
    r = rows_per_workgroup()
    for n in (1, 2, r - 1, r, r + 1):
        for pad in (0, PAD):
            run_step(dev, small_csr(n), nb, pad, "recurrence", "given")


def run_call_forms(dev):
    """out is Z; Z None with gamma = 0; Z given but gamma = 0 (not read: it holds NaN); the same bits from two calls; a base pointer
    8 bytes past a 16-byte boundary."""
    from diffusion_net import ops
    csr = irregular_csr(rows_per_workgroup())
    a = run_step(dev, csr, 65, PAD, "recurrence", "z")
    b = run_step(dev, csr, 65, PAD, "recurrence", "given")
    assert np.array_equal(a, b), "out = Z differs from a separate out"
    assert np.array_equal(run_step(dev, csr, 65, 0, "recurrence", "new"), b), "the leading dimension changed the bits"
    assert np.array_equal(run_step(dev, csr, 65, PAD, "recurrence", "new"), b), "a second call gave other bits"
    run_step(dev, csr, 65, PAD, "first", "given")
    c = run_step(dev, csr, 160, 0, "product", "new")
    assert np.array_equal(run_step(dev, csr, 160, 0, "product", "new"), c), "a second call gave other bits"
    for form in SCALARS:
        run_step(dev, csr, 65, PAD, form, "given", misaligned=True, record=True)
    # gamma = 0 with a Z full of NaN: the term is not formed
    d = device_csr(csr, dev)
    Y = torch.from_numpy(np.random.RandomState(2).randn(N_IRREGULAR, 8)).to(dev)
    Z = torch.full_like(Y, float("nan"))
    assert torch.equal(ops.cheb_step(*d, Y, Z, 1.0, 0.5, 0.0), ops.cheb_step(*d, Y, None, 1.0, 0.5, 0.0))


def run_refused_calls(dev):
    """The C entry: every refused call returns non-zero and writes nothing; the accepted degenerate sizes return 0 and write nothing."""
    from diffusion_net import _hip
    L = _hip.lib()
    csr = irregular_csr(rows_per_workgroup())
    rowptr, col, val = device_csr(csr, dev)
    n, nb = N_IRREGULAR, 9
    Y = torch.from_numpy(np.random.RandomState(3).randn(n, nb)).to(dev)
    Z = Y + 1.0
    out = torch.full((n, nb), SENTINEL, dtype=torch.float64, device=dev)
    y0, z0 = bits(Y), bits(Z)
    p = lambda t: t.data_ptr()

    def call(rp=p(rowptr), c=p(col), v=p(val), rows=n, y=p(Y), z=p(Z), o=p(out), width=nb, ld_=nb, g=-1.0):
        return L.dn_cheb_step_f64(rp, c, v, rows, y, z, o, width, ld_, 2.0, 0.5, g, None)

    refused = dict(null_rowptr=dict(rp=None), null_col=dict(c=None), null_val=dict(v=None), null_y=dict(y=None), null_out=dict(o=None),
                   null_z_with_gamma=dict(z=None), negative_rows=dict(rows=-1), negative_width=dict(width=-1, ld_=0), small_ld=dict(ld_=nb - 1),
                   out_is_y=dict(o=p(Y)))
    for name, kw in refused.items():
        assert call(**kw) != 0, name
    assert call(rows=0) == 0 and call(width=0, ld_=0) == 0
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and torch.equal(bits(Y), y0) and torch.equal(bits(Z), z0), "a refused call wrote something"
    assert call(z=None, g=0.0) == 0 and call() == 0
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


def run_op_errors(dev):
    """``ops.cheb_step`` raises before any launch."""
    import pytest
    from diffusion_net import ops
    csr = small_csr(9)
    rowptr, col, val = device_csr(csr, dev)
    Y = torch.ones(9, 4, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        ops.cheb_step(rowptr, col, val, Y, None, 1.0, 0.0, -1.0)                    # gamma without Z
    with pytest.raises(ValueError):
        ops.cheb_step(rowptr, col, val, Y, None, 1.0, 0.0, 0.0, out=Y)              # out is Y
    with pytest.raises(TypeError):
        ops.cheb_step(rowptr, col, val, Y.float(), None, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError):
        ops.cheb_step(rowptr.long(), col, val, Y, None, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError):
        ops.cheb_step(rowptr, col, val, Y[:8], None, 1.0, 0.0, 0.0)                 # rows do not fit
    with pytest.raises(ValueError):
        ops.cheb_step(rowptr, col, val, Y, torch.ones(9, 6, dtype=torch.float64, device=dev)[:, :4], 1.0, 0.0, 1.0)   # another leading dimension
    bad = col.clone()
    bad[1] = 9
    with pytest.raises(ValueError):
        ops.cheb_step(rowptr, bad, val, Y, None, 1.0, 0.0, 0.0)
    bad[1] = -1
    with pytest.raises(ValueError):
        ops.cheb_step(rowptr, bad, val, Y, None, 1.0, 0.0, 0.0)
    badp = rowptr.clone()
    badp[-1] += 1
    with pytest.raises(ValueError):
        ops.cheb_step(badp, col, val, Y, None, 1.0, 0.0, 0.0)
    assert tuple(ops.cheb_step(rowptr, col, val, Y[:, :0], None, 1.0, 0.0, 0.0).shape) == (9, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the solver
# ------------------------------------------------------------------------------------------------------------------------------
RTOL = 1e-9
MESH_SEED = 1          # chosen on the reference alone: eigsh's lambda_(k+1) - lambda_k > 1e-3 lambda_k in every case below (asserted)
# name -> (mesh, k)
SOLVER_CASES = {"sphere40_k8": ("sphere40", 8), "sphere300_k16": ("sphere300", 16), "sphere300_k64": ("sphere300", 64),
                "two_spheres_k32": ("two_spheres", 32), "sphere2000_k128": ("sphere2000", 128), "cloud500_k30": ("cloud500", 30)}
EMU_CASES = ("sphere40_k8", "sphere300_k16", "sphere300_k64")          # the kernel route at V <= 300


@functools.lru_cache(maxsize=None)
def pencil(mesh):
    """(L scipy CSR fp64, massvec fp64) as ``compute_operators`` forms them, never modified."""
    from diffusion_net import precompute as P, synthetic
    if mesh == "cloud500":
        import cloud_cases
        L, m = P.point_cloud_laplacian_host(cloud_cases.sample(500, MESH_SEED).astype(np.float64), 30)
    else:
        V = {"sphere40": 40, "sphere300": 300, "two_spheres": 300, "sphere2000": 2000}[mesh]
        v, f = synthetic.sphere_mesh(V, seed=MESH_SEED)
        if mesh == "two_spheres":          # two components and a vertex no face references: 601 vertices
            v, f = np.concatenate([v, v * 0.7 + np.array([3.0, 0.0, 0.0]), [[9.0, 9.0, 9.0]]]), np.concatenate([f, f + V])
        L, m = P.cotan_laplacian(v, f, 1e-10), P.vertex_areas(v, f)
    m = m + P.EPS * m.mean()
    L = sp.csr_matrix(L).astype(np.float64)
    L.sort_indices()
    L.data.setflags(write=False)
    m.setflags(write=False)
    return L, m


@functools.lru_cache(maxsize=None)
def eigsh_reference(name):
    """``precompute.laplacian_eigenbasis`` with k + 1 pairs, once per case: (evals [k + 1], evecs [V, k + 1])."""
    from diffusion_net import precompute as P
    mesh, k = SOLVER_CASES[name]
    ev, U = P.laplacian_eigenbasis(*pencil(mesh), k + 1)
    ev.setflags(write=False)
    U.setflags(write=False)
    return ev, U


def check_run(name, evals, evecs, info, dev, rtol=RTOL, max_iter=100):
    """The five checks of a solver run, in numpy, against the inputs alone."""
    from diffusion_net import precompute as P
    mesh, k = SOLVER_CASES[name]
    L, m = pencil(mesh)
    V = L.shape[0]
    assert isinstance(evals, torch.Tensor) and isinstance(evecs, torch.Tensor) and evals.dtype == evecs.dtype == torch.float64
    lam, Phi = evals.detach().cpu().numpy(), evecs.detach().cpu().numpy()
    assert lam.shape == (k,) and Phi.shape == (V, k) and np.isfinite(lam).all() and np.isfinite(Phi).all()
    lam_k = lam[-1]
    # 1. the stopping rule, recomputed independently
    R = ((L + P.EPS * sp.identity(V)) @ Phi - (m[:, None] * Phi) * lam) / np.sqrt(m)[:, None]
    res = float(np.linalg.norm(R, axis=0).max())
    # 2. M-orthonormality
    orth = float(np.abs(Phi.T @ (m[:, None] * Phi) - np.eye(k)).max())
    # 3. eigenvalues against eigsh, in order
    ev, Uref = eigsh_reference(name)
    ev_k = np.clip(ev[:k], 0.0, np.inf)
    dlam = float(np.abs(lam - ev_k).max())
    # 4. the subspace, once the reference alone has shown a gap behind lambda_k
    gap = float((ev[k] - ev[k - 1]) / ev[k - 1])
    sv = np.linalg.svd(Uref[:, :k].T @ (m[:, None] * Phi), compute_uv=False)
    print("eigenbasis %s on %s (%s): residual %.3e (allowed %.3e), orthonormality %.3e, eigenvalues %.3e (allowed %.3e), gap %.3e, "
          "1 - smallest singular value %.3e, %d iterations, %d products, degrees %s" % (
              name, dev, info["route"], res, 2 * rtol * lam_k, orth, dlam, 2 * rtol * lam_k, gap, 1.0 - sv.min(), info["iterations"],
              info["products"], info["degrees"]))
    helpers.record_margin("eigenbasis", dev, name=name, route=info["route"], V=V, k=k, nb=info["nb"], rtol=rtol, lambda_k=float(lam_k),
                          residual=res, residual_allowed=2 * rtol * lam_k, orthonormality=orth, orthonormality_allowed=1e-10,
                          eigenvalue_difference=dlam, eigenvalue_allowed=2 * rtol * lam_k, reference_gap=gap,
                          one_minus_smallest_singular_value=float(1.0 - sv.min()), iterations=info["iterations"], products=info["products"],
                          degrees=[int(x) for x in info["degrees"]], ub=float(info["ub"]), solver_residual=float(info["residual"]))
    assert res <= 2 * rtol * lam_k, (res, 2 * rtol * lam_k)
    assert orth <= 1e-10, orth
    assert dlam <= 2 * rtol * lam_k, (dlam, 2 * rtol * lam_k)
    assert gap > 1e-3, "the reference shows no gap behind lambda_k: choose another mesh seed"
    assert sv.min() >= 1.0 - 1e-8, sv.min()
    # 5. conventions
    top = np.abs(Phi).argmax(axis=0)
    assert (Phi[top, np.arange(k)] > 0).all(), "sign convention"
    assert (np.diff(lam) >= 0).all() and (lam >= 0).all()
    assert info["iterations"] <= max_iter and all(2 <= d <= 64 for d in info["degrees"]) and info["nb"] == k + max(16, -(-k // 4))
    if 2 * info["nb"] > V:
        assert info["route"] == "dense" and info["products"] == 0
    else:
        assert info["products"] == info["iterations"] + sum(info["degrees"]) and len(info["degrees"]) == info["iterations"] - 1
        assert info["residual"] <= rtol * lam_k and info["ub"] >= lam_k


def solve(name, dev, route, **kw):
    """One run of ``geometry.laplacian_eigenbasis`` in fp64 with the mass on ``dev``; ``route``: what ``info`` must name."""
    from diffusion_net import geometry
    mesh, k = SOLVER_CASES[name]
    L, m = pencil(mesh)
    evals, evecs, info = geometry.laplacian_eigenbasis(L, torch.from_numpy(np.array(m)).to(dev), k, dtype=torch.float64, return_info=True, **kw)
    assert evals.device.type == evecs.device.type == torch.device(dev).type
    V, nb = L.shape[0], k + max(16, -(-k // 4))
    assert info["route"] == ("dense" if 2 * nb > V else route), info["route"]
    return evals, evecs, info


def solve_numpy(name, **kw):
    """The numpy route itself (``geometry.laplacian_eigenbasis`` would take the kernel route where a device is present)."""
    from diffusion_net import precompute as P
    mesh, k = SOLVER_CASES[name]
    evals, evecs, info = P.laplacian_eigenbasis_subspace(*pencil(mesh), k, return_info=True, **kw)
    assert evals.dtype == evecs.dtype == np.float64 and info["route"] in ("numpy", "dense")
    return torch.from_numpy(evals), torch.from_numpy(np.ascontiguousarray(evecs)), info


def run_solver(name, dev, route):
    evals, evecs, info = solve_numpy(name) if route == "numpy" else solve(name, dev, route)
    check_run(name, evals, evecs, info, dev)
    return evals, evecs, info


# ------------------------------------------------------------------------------------------------------------------------------
# 3. compute_operators_with / get_operators with eigensolver="subspace"
# ------------------------------------------------------------------------------------------------------------------------------
def _sparse_parts(t):
    t = t.coalesce()
    return t.indices().cpu(), t.values().cpu()


def run_compute_operators(dev):
    """A 300-vertex mesh in fp64 (so that the cast of the results loses nothing), k = 32: the six other outputs bit for bit the default
    route's, the eigenvalues within check 3, the eigenvectors of the same shape and dtype."""
    from diffusion_net import geometry, synthetic
    v, f = synthetic.sphere_mesh(300, seed=MESH_SEED)
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    ref = geometry.compute_operators(verts, faces, 32)
    got = geometry.compute_operators_with(verts, faces, 32, eigensolver="subspace")
    for i, name in ((0, "frames"), (1, "mass")):
        assert torch.equal(got[i], ref[i]), name
    for i, name in ((2, "L"), (5, "gradX"), (6, "gradY")):
        (gi, gv), (ri, rv) = _sparse_parts(got[i]), _sparse_parts(ref[i])
        assert got[i].shape == ref[i].shape and torch.equal(gi, ri) and torch.equal(gv, rv), name
    lam, lam_ref = got[3].cpu().numpy(), ref[3].cpu().numpy()
    assert got[3].dtype == ref[3].dtype == torch.float64 and got[3].device == ref[3].device
    assert np.abs(lam - lam_ref).max() <= 2 * RTOL * lam_ref[-1], np.abs(lam - lam_ref).max()
    assert got[4].shape == ref[4].shape == (300, 32) and got[4].dtype == ref[4].dtype and got[4].device == ref[4].device
    return got


def run_cache_round_trip(dev, tmp_path, monkeypatch):
    import os
    import pytest
    from diffusion_net import geometry, precompute, synthetic
    v, f = synthetic.sphere_mesh(300, seed=MESH_SEED)
    verts, faces = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
    first = geometry.get_operators(verts, faces, 16, op_cache_dir=str(tmp_path), eigensolver="subspace")
    assert len(os.listdir(tmp_path)) == 1
    monkeypatch.setattr(precompute, "compute_operators_with", lambda *a, **k: pytest.fail("the cache was not used"))
    again = geometry.get_operators(verts, faces, 16, op_cache_dir=str(tmp_path), eigensolver="subspace")
    assert torch.equal(again[3], first[3]) and torch.equal(again[4], first[4]) and torch.equal(again[1], first[1])
    lists = geometry.get_all_operators([verts], [faces], 16, op_cache_dir=str(tmp_path), eigensolver="subspace")
    assert torch.equal(lists[4][0], first[4])
    monkeypatch.undo()
    for fn in (lambda: geometry.compute_operators_with(verts, faces, 16, eigensolver="arpack"),
               lambda: geometry.get_operators(verts, faces, 16, eigensolver="lobpcg"),
               lambda: geometry.get_all_operators([verts], [faces], 16, eigensolver=1)):
        with pytest.raises(ValueError, match="eigensolver"):
            fn()

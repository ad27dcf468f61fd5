"""Shared bodies of the triangle-mesh operator tests (drivers: test_mesh_emu.py on the emulator build of dn_mesh.hip, test_mesh_gpu.py on
the device, test_mesh_host.py for the yardstick itself and the keyword on host tensors).

The yardstick is the fp64 host route of ``precompute`` -- ``vertex_normals``, ``tangent_frames``, ``cotan_laplacian``, ``vertex_areas``,
``gradient_operator`` -- on the SAME fp32 positions cast to fp64.  Both routes evaluate the same formulas in fp64 and differ in the order
of their sums and in FMA contraction only, so every bound below is counted from the operations, with u = 2^-53, and none is tuned to a
result.  test_mesh_host.py first shows that the host route with its faces shuffled and rotated -- other summation orders -- passes the same
bounds: they are neither vacuous nor too tight.

L.  One corner term is w = 0.5 d / (n + 1e-10), d = a.b, n = |a x b|.  With q = |a||b| / (n + 1e-10): the dot product errs by <= 3 u |a||b|,
    the cross product (norm-wise) by <= 2 sqrt(2) u |a||b|, its norm by 3 u n more, the sum with 1e-10 and the division by u each; the
    factor 0.5 is exact.  So |dw| <= 0.5 u (3 q + 2.83 q^2 + 3 q + 2 q) <= 4 u q (1 + q): the scale is q (1 + q), NOT |w| -- w cancels to
    zero at a right angle while its error does not.  Adding the T terms of an entry errs by <= (T - 1) u sum |w| <= 0.5 T u sum q, a
    diagonal term (the sum of two weights on the device) by one more u.  One route: (4 + T / 2) u sum q (1 + q); the difference of two
    routes twice that, (8 + T) u sum q (1 + q).  The test allows c = T + OPS_W with OPS_W = 24, the plain operation count of one term
    (dot 5, cross 9, norm 6, + eps 1, / 1, x 0.5 1, the diagonal's + 1), which is above the 8 the analysis needs.
mass.  area / 3 per face: cross 9, norm 6, x 0.5, / 3, the sum: c = deg + OPS_M with OPS_M = 18, times u times the entry.
normals.  A unit face normal n / (|n| + 1e-6): cross 9, norm 6, + eps 1, three divisions: 19; the sum of deg of them (each of length
    <= 1) errs by deg u more each; the normalisation (norm 6, three divisions) 9 more: c = deg + OPS_N with OPS_N = 28, and the bound is
    c u deg / |sum n_f| -- deg terms of unit size, divided by the length of their sum.
frames.  basisX = (c - n (n.c)) / (|.| + 1e-6): the projection has length >= sqrt(1 - 0.81) = 0.43 (|n_x| < 0.9) or >= sqrt(1 - 0.19) =
    0.9 (the other branch), so an error e of the normal moves basisX by <= (2 / 0.43) e + its own 14 operations, and basisY = n x basisX
    by e more: <= FRAME_AMP e with FRAME_AMP = 6, plus OPS_F = 24 operations: c = FRAME_AMP (deg + OPS_N) + OPS_F, same scale
    u deg / |sum n_f| (which is >= u).  No test vertex may lie within 1e-6 of the branch | |n_x| - 0.9 | = 0 (test_mesh_host.py asserts it).
gradients.  Row i: t_j (difference exact, two dot products: 10), G (6 per edge, summed over deg edges), the 2 x 2 inverse (9), the
    coefficients (6 per edge), the diagonal's sum over deg: OPS_G = 40 plus 2 deg.  A relative error e of the t_j (own round-off, or the
    frame's error c_frame u when the normals are the device's) moves G^-1 t by <= kappa(G) (e + 2 e) in the 2-norm, sqrt(2) more per
    component: GRAD_AMP = 5.  Bound: GRAD_AMP (2 deg + OPS_G + c_frame) u kappa(G_i) max_j |coef_ij|, kappa from the host route's own G_i.
fp32 tensors of ``geometry.mesh_operators``: one rounding more, 2^-24 |ref|."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import helpers

U = 2.0 ** -53
EPS32 = 2.0 ** -24
OPS_W, OPS_M, OPS_N, OPS_F, OPS_G = 24, 18, 28, 24, 40
FRAME_AMP, GRAD_AMP = 6, 5
BRANCH_MARGIN = 1e-6

CASES = ("single_triangle", "right_triangle", "tetrahedron", "sphere200", "sphere1500", "open_grid", "three_faces_on_an_edge", "duplicated_face",
         "obtuse", "hub_fan", "strip255", "strip256", "strip257")
DEGENERATE = ("repeated_index", "zero_area_on_axis")
FALLBACK = ("unreferenced_vertex", "opposing_faces")            # a vertex without a finite normal: the normals of the host rule


# ----------------------------------------------------------------------------------------------------------------- the meshes
def _strip(n_faces, seed):
    """A zig-zag triangle strip of n_faces faces, gently bent out of its plane."""
    rs = np.random.RandomState(seed)
    k = np.arange(n_faces + 2)
    v = np.stack([0.5 * k, (k % 2) * 0.8 + 0.05 * rs.rand(len(k)), 0.1 * np.sin(0.3 * k) + 0.05 * rs.rand(len(k))], axis=1)
    f = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]                              # one orientation
    return v, f


def _grid(nx, ny, seed):
    rs = np.random.RandomState(seed)
    x, y = np.meshgrid(np.arange(nx) / 4.0, np.arange(ny) / 4.0, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), 0.1 * rs.rand(nx * ny)], axis=1)
    v[:, :2] += 0.05 * rs.rand(nx * ny, 2)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel()
    f = np.concatenate([np.stack([a, a + ny, a + 1], axis=1), np.stack([a + 1, a + ny, a + ny + 1], axis=1)])
    return v, f


TETRA_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.3, 0.3, 0.8]])
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts [V, 3] fp32, faces [F, 3] int64), never modified."""
    from diffusion_net import synthetic
    if name == "single_triangle":
        v, f = np.array([[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.3, 0.9, 0.4]]), np.array([[0, 1, 2]])
    elif name == "right_triangle":                               # the right angle at vertex 0: w = 0 exactly, L[1,2] = L[2,1] = -0 stays an entry
        v, f = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([[0, 1, 2]])
    elif name == "tetrahedron":
        v, f = TETRA_V, TETRA_F
    elif name.startswith("sphere"):
        v, f = synthetic.sphere_mesh(int(name[6:]), seed=3)
    elif name == "open_grid":
        v, f = _grid(7, 5, 1)
    elif name == "three_faces_on_an_edge":                       # non-manifold: the edge (0, 1) has three faces
        v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.4, 0.9, 0.0], [0.5, -0.3, 0.8], [0.6, -0.7, -0.5]])
        f = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    elif name == "duplicated_face":
        v, f = TETRA_V, np.concatenate([TETRA_F, TETRA_F[:1]])
    elif name == "obtuse":                                       # apex angles of about 150 degrees: negative weights
        k = np.arange(12)
        v = np.stack([k * 1.0, (k % 2) * 0.27 + 0.01 * np.cos(k), 0.02 * np.sin(k)], axis=1)
        f = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
        f[1::2] = f[1::2][:, [1, 0, 2]]
    elif name == "hub_fan":                                      # a closed fan of 300 faces: the hub's row of L has 301 entries
        n = 300
        t = 2 * np.pi * np.arange(n) / n
        rs = np.random.RandomState(2)
        rim = np.stack([np.cos(t) * (1 + 0.1 * rs.rand(n)), np.sin(t) * (1 + 0.1 * rs.rand(n)), 0.1 * rs.rand(n)], axis=1)
        v = np.concatenate([[[0.0, 0.0, 0.5]], rim])
        f = np.stack([np.zeros(n, dtype=np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1)
    elif name.startswith("strip"):                               # face counts on both sides of the face pass's 256-face workgroup
        v, f = _strip(int(name[5:]), 5)
    elif name == "repeated_index":                               # a face that names a vertex twice
        v, f = TETRA_V, np.concatenate([TETRA_F, [[0, 0, 1]]])
    elif name == "zero_area_on_axis":                            # vertices 0, 1, 2 on the x axis at small integers: a cross product of exactly zero
        v = np.array([[1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [4.0, 0.0, 0.0], [2.0, 1.0, 0.5], [3.0, -1.0, 0.25]])
        f = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [1, 0, 4], [2, 1, 4]])
    elif name == "unreferenced_vertex":
        v, f = np.concatenate([TETRA_V, [[2.0, 2.0, 2.0]]]), TETRA_F
    elif name == "opposing_faces":                               # the two unit normals cancel exactly at every vertex
        v, f = TETRA_V[:3], np.array([[0, 1, 2], [0, 2, 1]])
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


# ----------------------------------------------------------------------------------------------------------------- the yardstick and its bounds
def _sorted_csr(m):
    m = sp.csr_matrix(m)
    m.sum_duplicates()
    m.sort_indices()
    return m


def corner_terms(v, f):
    """(rows, cols, q (1 + q), 1) of every term of ``precompute.cotan_laplacian``, in its own order."""
    rows, cols, qs = [], [], []
    for k in range(3):
        i, j, o = f[:, (k + 1) % 3], f[:, (k + 2) % 3], f[:, k]
        a, b = v[i] - v[o], v[j] - v[o]
        q = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) / (np.linalg.norm(np.cross(a, b), axis=1) + 1e-10)
        rows += [i, j, i, j]
        cols += [i, j, j, i]
        qs += [q * (1 + q)] * 4
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(qs)


def host_route(v32, f, normals=None):
    """The fp64 host route on fp32 positions: a dict of its outputs, all with sorted CSR patterns."""
    from diffusion_net import precompute as P
    v = np.asarray(v32, dtype=np.float64)
    V = v.shape[0]
    n = P.vertex_normals(v, f) if normals is None else normals
    frames = P.tangent_frames(n)
    L = _sorted_csr(P.cotan_laplacian(v, f))
    Lc = L.tocoo()
    grad = _sorted_csr(P.gradient_operator(v, frames, np.stack([Lc.row, Lc.col])))
    # an unreferenced vertex has an empty row in L and one explicit 0 on the gradient's diagonal: the same matrix, stated on L's pattern
    gc = grad.tocoo()
    drop = (np.diff(L.indptr) == 0)[gc.row] & (gc.row == gc.col) & (gc.data == 0)
    grad = _sorted_csr(sp.coo_matrix((gc.data[~drop], (gc.row[~drop], gc.col[~drop])), shape=(V, V)))
    assert np.array_equal(grad.indptr, L.indptr) and np.array_equal(grad.indices, L.indices), "the host gradient operator is not on L's pattern"
    with np.errstate(invalid="ignore", divide="ignore"):
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        fn = fn / (np.linalg.norm(fn, axis=1, keepdims=True) + 1e-6)
        nsum = np.zeros_like(v)
        for k in range(3):
            np.add.at(nsum, f[:, k], fn)
        raw = nsum / np.linalg.norm(nsum, axis=1, keepdims=True)
    return dict(V=V, normals=n, raw_normals=raw, nsum_len=np.linalg.norm(nsum, axis=1), frames=frames, L=L, mass=P.vertex_areas(v, f), grad=grad,
                deg=np.bincount(f.reshape(-1), minlength=V))


def bounds_of(v32, f, host, device_normals):
    """The bounds of the module docstring for this mesh, from the host route's own numbers.  ``device_normals``: the frames are those of
    normals with the normals' error (otherwise of given, identical normals)."""
    v = np.asarray(v32, dtype=np.float64)
    V, L, deg = host["V"], host["L"], host["deg"].astype(np.float64)
    rows, cols, qq = corner_terms(v, f)
    Q = _sorted_csr(sp.coo_matrix((qq, (rows, cols)), shape=(V, V)))
    T = _sorted_csr(sp.coo_matrix((np.ones_like(qq), (rows, cols)), shape=(V, V)))
    assert np.array_equal(Q.indptr, L.indptr) and np.array_equal(Q.indices, L.indices) and np.array_equal(T.indices, L.indices)
    b_l = (T.data + OPS_W) * U * Q.data
    b_mass = (deg + OPS_M) * U * host["mass"]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = U * deg / host["nsum_len"]                        # (inf or NaN where the sum vanishes: such a vertex has no raw normal to compare)
    b_normal = (deg + OPS_N) * scale
    c_frame = (FRAME_AMP * (deg + OPS_N) * (deg / np.where(host["nsum_len"] > 0, host["nsum_len"], 1.0)) if device_normals else np.zeros(V)) + OPS_F
    b_frame = c_frame * U
    # gradients: kappa of the host route's own G_i, from its own tangent coordinates
    Lc = L.tocoo()
    keep = Lc.row != Lc.col
    tail, tip = Lc.row[keep], Lc.col[keep]
    d = v[tip] - v[tail]
    tx, ty = np.einsum("ij,ij->i", d, host["frames"][tail, 0]), np.einsum("ij,ij->i", d, host["frames"][tail, 1])
    gxx = np.bincount(tail, weights=tx * tx, minlength=V) + 1e-5
    gxy = np.bincount(tail, weights=tx * ty, minlength=V)
    gyy = np.bincount(tail, weights=ty * ty, minlength=V) + 1e-5
    half, disc = 0.5 * (gxx + gyy), np.sqrt((0.5 * (gxx - gyy)) ** 2 + gxy ** 2)
    kappa = (half + disc) / (half - disc)
    g = host["grad"]
    row_of = np.repeat(np.arange(V), np.diff(g.indptr))
    cmax = np.zeros(V)
    np.maximum.at(cmax, row_of, np.maximum(np.abs(g.data.real), np.abs(g.data.imag)))
    edges = np.bincount(tail, minlength=V)
    b_grad_row = GRAD_AMP * (2 * edges + OPS_G + c_frame) * U * kappa * cmax
    return dict(L=b_l, mass=b_mass, normal=b_normal, frame=b_frame, grad=b_grad_row[row_of], grad_row=b_grad_row, kappa=kappa)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(host route, bounds with given normals, bounds with the device's normals) of a case: computed once, shared, never modified."""
    v, f = mesh(name)
    host = host_route(v, f)
    return host, bounds_of(v, f, host, False), bounds_of(v, f, host, True)


def share(diff, bound):
    """max |diff| / bound; an entry with a zero bound must agree exactly."""
    diff, bound = np.abs(np.asarray(diff, dtype=np.float64)).ravel(), np.asarray(bound, dtype=np.float64).ravel()
    if diff.size == 0:
        return 0.0
    assert (diff[bound == 0] == 0).all(), "an entry whose terms are all exact differs"
    pos = bound > 0
    return float((diff[pos] / bound[pos]).max()) if pos.any() else 0.0


def compare(got, host, b, normals_compared=True, extra=0.0):
    """Shares of the bounds of ``got`` (a dict as ``host_route`` returns, or the fields of it a caller has).  ``extra``: a relative
    allowance on top (2^-24 for fp32 tensors)."""
    out = {}
    L, g = host["L"], host["grad"]
    if "L" in got:
        out["L"] = share(got["L"] - L.data, b["L"] + extra * np.abs(L.data))
    if "mass" in got:
        out["mass"] = share(got["mass"] - host["mass"], b["mass"] + extra * host["mass"])
    if "raw_normals" in got and normals_compared:
        ok = np.isfinite(host["raw_normals"]).all(axis=1)
        assert np.array_equal(ok, np.isfinite(got["raw_normals"]).all(axis=1)), "the routes disagree on which vertices have a normal"
        out["normal"] = share((got["raw_normals"] - host["raw_normals"])[ok], np.repeat(b["normal"][ok], 3))
    if "frames" in got:
        out["frame"] = share(got["frames"] - host["frames"], np.repeat(b["frame"], 9) + extra * np.abs(host["frames"]).ravel())
    if "gx" in got:
        out["gradX"] = share(got["gx"] - g.data.real, b["grad"] + extra * np.abs(g.data.real))
        out["gradY"] = share(got["gy"] - g.data.imag, b["grad"] + extra * np.abs(g.data.imag))
    return out


# ----------------------------------------------------------------------------------------------------------------- running the kernels
def _np(t):
    return t.detach().cpu().numpy()


def tensors(dev, name):
    v, f = mesh(name)
    return torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev)


def run_ops(tv, tf, normals):
    """The two ops -> numpy dict; ``normals`` [V, 3] fp64 numpy for the vertex pass."""
    from diffusion_net import ops
    rowptr, col, lval, mass, nsum = ops.mesh_assemble(tv, tf)
    V = tv.shape[0]
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and tuple(rowptr.shape) == (V + 1,) and col.shape == lval.shape
    assert lval.dtype == mass.dtype == nsum.dtype == torch.float64 and tuple(mass.shape) == (V,) and tuple(nsum.shape) == (V, 3)
    assert rowptr.device == col.device == lval.device == mass.device == nsum.device == tv.device
    frames, gx, gy = ops.mesh_frames_gradients(tv, rowptr, col, torch.from_numpy(np.ascontiguousarray(normals)).to(tv.device))
    assert frames.dtype == gx.dtype == gy.dtype == torch.float64 and tuple(frames.shape) == (V, 3, 3) and gx.shape == gy.shape == col.shape
    assert frames.device == gx.device == gy.device == tv.device
    with np.errstate(invalid="ignore", divide="ignore"):
        raw = _np(nsum) / np.linalg.norm(_np(nsum), axis=1, keepdims=True)
    return dict(rowptr=_np(rowptr), col=_np(col), L=_np(lval), mass=_np(mass), nsum=_np(nsum), raw_normals=raw, frames=_np(frames), gx=_np(gx),
                gy=_np(gy))


def check_structure(got, host, bL, what):
    """Pattern == scipy's CSR of the host L (explicit zeros included), L == L^T bit for bit, row sums within the L bound of zero."""
    L, V = host["L"], host["V"]
    assert np.array_equal(got["rowptr"], L.indptr) and np.array_equal(got["col"], L.indices), "%s: the pattern differs from the host route's" % what
    D = np.zeros((V, V), dtype=np.int64)                          # (the bits as integers: +0 and -0 stay apart)
    rows = np.repeat(np.arange(V), np.diff(got["rowptr"]))
    D[rows, got["col"]] = got["L"].view(np.int64)
    assert np.array_equal(D, D.T), "%s: L != L^T bit for bit" % what
    rowsum = np.abs(np.bincount(rows, weights=got["L"], minlength=V))
    allowed = np.bincount(rows, weights=bL, minlength=V)
    return share(rowsum, allowed)


def check(dev, name):
    """The two ops on one case, with the host route's normals for the vertex pass: structure, values against the bounds, repeatability."""
    host, b, _ = reference(name)
    tv, tf = tensors(dev, name)
    got = run_ops(tv, tf, host["normals"])
    rs = check_structure(got, host, b["L"], name)
    shares = compare(got, host, b)
    print("mesh %s on %s: V %d, F %d, nnz %d; shares of the bounds %s, row sums %.3f; largest kappa(G) %.3e" % (
        name, dev, host["V"], tf.shape[0], len(got["col"]), {k: round(s, 4) for k, s in shares.items()}, rs, float(b["kappa"].max()) if host["V"] else 0.0))
    helpers.record_margin("mesh_" + name, dev, V=host["V"], F=int(tf.shape[0]), nnz=len(got["col"]), rowsum_share_of_bound=rs,
                          **{k + "_share_of_bound": s for k, s in shares.items()})
    assert rs <= 1.0, ("row sums", rs)
    for k, s in shares.items():
        assert s <= 1.0, (k, s)
    again = run_ops(tv, tf, host["normals"])
    for key in got:
        assert np.array_equal(got[key].view(np.int32), again[key].view(np.int32)), "%s differs between two calls" % key
    return got


def check_mesh_operators(dev, name):
    """``geometry.mesh_operators`` (the device's own normals, or the host rule's where a vertex has none) against the host route: fp32
    tensors on the device, L's pattern for all three matrices, the bounds plus one fp32 rounding."""
    from diffusion_net import geometry
    host, _, b = reference(name)
    tv, tf = tensors(dev, name)
    V = host["V"]
    frames, mass, L, gX, gY = geometry.mesh_operators(tv, tf)
    rows = np.repeat(np.arange(V), np.diff(host["L"].indptr))
    for t, shape in ((frames, (V, 3, 3)), (mass, (V,)), (L, (V, V)), (gX, (V, V)), (gY, (V, V))):
        assert t.dtype == torch.float32 and t.device == tv.device and tuple(t.shape) == shape
    for m in (L, gX, gY):
        assert m.is_sparse and m.is_coalesced()
        idx = _np(m.indices())
        assert np.array_equal(idx[0], rows) and np.array_equal(idx[1], host["L"].indices), "not L's pattern"
    got = dict(L=_np(L.values()), mass=_np(mass), frames=_np(frames), gx=_np(gX.values()), gy=_np(gY.values()))
    shares = compare(got, host, b, extra=EPS32)
    print("mesh_operators %s on %s: shares of the bounds (with one fp32 rounding) %s" % (name, dev, {k: round(s, 4) for k, s in shares.items()}))
    helpers.record_margin("mesh_operators_" + name, dev, V=V, **{k + "_share_of_bound": s for k, s in shares.items()})
    for k, s in shares.items():
        assert s <= 1.0, (k, s)
    # given normals are used as they are
    rs = np.random.RandomState(4).randn(max(V, 1), 3)[:V]
    given = rs / np.linalg.norm(rs, axis=1, keepdims=True)
    given[np.abs(np.abs(given[:, 0]) - 0.9) < 1e-3] = [0.0, 0.0, 1.0]
    frames2 = geometry.mesh_operators(tv, tf, normals=torch.from_numpy(given).to(tv.device))[0]
    from diffusion_net import precompute
    want = precompute.tangent_frames(given)
    assert V == 0 or np.abs(_np(frames2) - want).max() <= OPS_F * U / 0.43 + EPS32          # (entries of at most 1, rounded to fp32 once)


def run_empty(dev):
    """V = 0 and F = 0, and vertices without a face."""
    from diffusion_net import geometry, ops
    v0, f0 = torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    rowptr, col, lval, mass, nsum = ops.mesh_assemble(v0, f0)
    assert rowptr.tolist() == [0] and col.numel() == 0 and lval.numel() == 0 and tuple(mass.shape) == (0,) and tuple(nsum.shape) == (0, 3)
    frames, gx, gy = ops.mesh_frames_gradients(v0, rowptr, col, nsum)
    assert tuple(frames.shape) == (0, 3, 3) and gx.numel() == 0 and gy.numel() == 0
    v5 = torch.from_numpy(np.array(mesh("tetrahedron")[0])).to(dev)
    rowptr, col, lval, mass, nsum = ops.mesh_assemble(v5, f0)
    assert rowptr.tolist() == [0] * 5 and col.numel() == 0 and (mass == 0).all() and (nsum == 0).all()
    normals = torch.tensor([[0.0, 0.0, 1.0]] * 4, dtype=torch.float64, device=dev)
    frames, gx, gy = ops.mesh_frames_gradients(v5, rowptr, col, normals)
    assert torch.equal(frames[:, 0], torch.tensor([[1.0, 0.0, 0.0]] * 4, dtype=torch.float64, device=dev) / (1.0 + 1e-6)) and gx.numel() == 0
    out = geometry.mesh_operators(v0, f0)
    assert tuple(out[0].shape) == (0, 3, 3) and tuple(out[2].shape) == (0, 0) and out[2]._nnz() == 0


def run_bad_indices(dev):
    """A face index outside [0, V): IndexError with the count, before any output is read; the launch itself counts the faces in the status
    word and assembles the other faces alone."""
    from diffusion_net import ops
    tv, tf = tensors(dev, "tetrahedron")
    for value, faces_hit in ((4, [1]), (-1, [0, 3])):
        bad = tf.clone()
        for r in faces_hit:
            bad[r, 1] = value
        try:
            ops.mesh_assemble(tv, bad)
        except IndexError as err:
            assert ("%d face" % len(faces_hit)) in str(err)
        else:
            raise AssertionError("an index outside [0, V) was accepted")
        rowptr, col, lval, vrec, count, status = ops._mesh_assemble_launch(tv, bad)
        assert int(status.item()) == len(faces_hit)
        keep = np.array([r not in faces_hit for r in range(4)])
        v, f = mesh("tetrahedron")
        host = host_route(v, f[keep])
        b = bounds_of(v, f[keep], host, False)
        nnz = int(count.item())
        got = dict(rowptr=_np(rowptr), col=_np(col)[:nnz], L=_np(lval)[:nnz], mass=_np(vrec)[:, 0])
        check_structure(got, host, b["L"], "bad index")
        for k, s in compare(got, host, b).items():
            assert s <= 1.0, (k, s)
    # a pattern the vertex pass cannot walk
    host, _, _ = reference("tetrahedron")
    rowptr, col = ops.mesh_assemble(tv, tf)[:2]
    n = torch.from_numpy(host["normals"]).to(dev)
    for rp, cl in ((rowptr, torch.where(col == 3, torch.full_like(col, 7), col)), (rowptr.flip(0).contiguous(), col),
                   (rowptr, torch.where(col == 0, torch.full_like(col, 1), col))):      # column out of range; decreasing pointers; no diagonal in row 0
        try:
            ops.mesh_frames_gradients(tv, rp, cl, n)
        except IndexError:
            continue
        raise AssertionError("a broken pattern was accepted")


def run_ops_validation(dev):
    from diffusion_net import ops
    tv, tf = tensors(dev, "tetrahedron")
    rowptr, col, _, _, nsum = ops.mesh_assemble(tv, tf)
    for args, exc in (((tv[:, :2], tf), ValueError), ((tv, tf[:, :2]), ValueError), ((tv, tf.int()), TypeError), ((tv.double(), tf), TypeError),
                      ((tv, tf.reshape(-1)), ValueError)):
        try:
            ops.mesh_assemble(*args)
        except exc:
            continue
        raise AssertionError("ops.mesh_assemble accepted %s" % (tuple(tuple(a.shape) for a in args),))
    for args, exc in (((tv[:, :2], rowptr, col, nsum), ValueError), ((tv, rowptr[:-1], col, nsum), ValueError), ((tv, rowptr.long(), col, nsum), TypeError),
                      ((tv, rowptr, col.long(), nsum), TypeError), ((tv, rowptr, col, nsum.float()), TypeError), ((tv, rowptr, col, nsum[:3]), ValueError),
                      ((tv.double(), rowptr, col, nsum), TypeError), ((tv, rowptr, col.reshape(-1, 2), nsum), ValueError)):
        try:
            ops.mesh_frames_gradients(*args)
        except exc:
            continue
        raise AssertionError("ops.mesh_frames_gradients accepted %s" % (tuple(tuple(a.shape) for a in args),))
    if tv.is_cuda:
        for fn in (lambda: ops.mesh_assemble(tv, tf.cpu()), lambda: ops.mesh_frames_gradients(tv, rowptr, col, nsum.cpu())):
            try:
                fn()
            except RuntimeError:
                continue
            raise AssertionError("tensors on two devices were accepted")


def run_abi_errors():
    """Every non-zero return of the entry points, through ctypes, on host buffers: nothing is launched, the outputs keep their fill."""
    from diffusion_net import _hip
    L = _hip.lib()
    V, F = 5, 7
    assert L.dn_mesh_workspace_bytes(V, F) == 264 * 8 and L.dn_mesh_workspace_bytes(V, 8) == 264 * 8 and L.dn_mesh_workspace_bytes(0, 0) == 0
    for bad in ((-1, F), (V, -1), (V, 300_000_000)):
        assert L.dn_mesh_workspace_bytes(*bad) == 0
    ws_bytes = 264 * 8
    verts, faces = torch.zeros(V, 3), torch.zeros(F, 3, dtype=torch.int64)
    fill = dict(ws=torch.full((ws_bytes,), 0xF9, dtype=torch.uint8), status=torch.full((1,), -7, dtype=torch.int32),
                rowptr=torch.full((V + 1,), -7, dtype=torch.int32), col=torch.full((64,), -7, dtype=torch.int32),
                out=torch.full((64,), -7.0, dtype=torch.float64), count=torch.full((1,), -7, dtype=torch.int32),
                frames=torch.full((V, 9), -7.0, dtype=torch.float64), gx=torch.full((64,), -7.0, dtype=torch.float64),
                gy=torch.full((64,), -7.0, dtype=torch.float64))
    p = lambda key, null=None: None if key == null else fill[key].data_ptr()

    def emit(v_=V, f_=F, verts_=verts, faces_=faces, null=None, bytes_=ws_bytes):
        return L.dn_mesh_emit_f32(_hip.ptr(verts_), v_, _hip.ptr(faces_), f_, p("ws", null), bytes_, p("status", null), None)

    assert emit(v_=-1) != 0 and emit(f_=-1) != 0 and emit(f_=300_000_000) != 0
    assert emit(verts_=None) != 0 and emit(faces_=None) != 0 and emit(null="ws") != 0 and emit(null="status") != 0
    assert emit(bytes_=ws_bytes - 1) != 0
    assert emit(f_=0, faces_=None, null="ws", bytes_=0) == 0 and emit(f_=0, null="status") == 0      # no face: success, nothing launched

    m = 12
    keys, perm, vals, rank = torch.zeros(m, dtype=torch.int64), torch.arange(m), torch.zeros(m, 4, dtype=torch.float64), torch.ones(m, dtype=torch.int64)

    def seg(keys_=keys, perm_=perm, vals_=vals, m_=m, rank_=rank, rows_=V, csr=True, null=None):
        outs = [p(key, null) if (csr or key == "out") else None for key in ("rowptr", "col", "out", "count")]
        return L.dn_segment_sum_f64_f64(_hip.ptr(keys_), _hip.ptr(perm_), _hip.ptr(vals_), m_, _hip.ptr(rank_), rows_, *outs, None)

    def seg4(keys_=keys, perm_=perm, vals_=vals, m_=m, rows_=V, null=None):
        return L.dn_segment_sum4_f64_f64(_hip.ptr(keys_), _hip.ptr(perm_), _hip.ptr(vals_), m_, rows_, p("out", null), None)

    assert seg(m_=-1) != 0 and seg(rows_=-1) != 0 and seg4(m_=-1) != 0 and seg4(rows_=-1) != 0
    for kw in (dict(keys_=None), dict(perm_=None), dict(vals_=None), dict(rank_=None), dict(null="col"), dict(null="out"), dict(null="count")):
        assert seg(**kw) != 0, kw
    for kw in (dict(keys_=None), dict(perm_=None), dict(vals_=None), dict(null="out")):
        assert seg(csr=False, **kw) != 0, kw
        assert seg4(**kw) != 0, kw
    assert seg(m_=0, rows_=0, keys_=None, perm_=None, vals_=None, rank_=None, csr=False, null="out") == 0
    assert seg4(m_=0, rows_=0, keys_=None, perm_=None, vals_=None, null="out") == 0

    normals = torch.zeros(V, 3, dtype=torch.float64)

    def vert(v_=V, nnz_=20, verts_=verts, normals_=normals, null=None):
        return L.dn_mesh_frames_gradients_f64(_hip.ptr(verts_), v_, p("rowptr", null), p("col", null), nnz_, _hip.ptr(normals_), p("frames", null),
                                              p("gx", null), p("gy", null), p("status", null), None)

    assert vert(v_=-1) != 0 and vert(nnz_=-1) != 0 and vert(v_=0) != 0          # (entries without a vertex)
    assert vert(verts_=None) != 0 and vert(normals_=None) != 0
    for key in ("rowptr", "col", "frames", "gx", "gy", "status"):
        assert vert(null=key) != 0, key
    assert vert(v_=0, nnz_=0, verts_=None, normals_=None, null="status") == 0                        # no vertex: success, nothing launched
    for key, t in fill.items():
        assert bool((t == (0xF9 if key == "ws" else -7)).all()), key


def run_library_ops(dev):
    """``torch.ops.diffusion_net.mesh_assemble`` / ``.mesh_frames_gradients`` equal the Python ops; their fake kernels give the shapes."""
    from diffusion_net import ops, torchlib  # noqa: F401
    host, _, _ = reference("sphere200")
    tv, tf = tensors(dev, "sphere200")
    n = torch.from_numpy(host["normals"]).to(dev)
    a = torch.ops.diffusion_net.mesh_assemble(tv, tf)
    want = ops.mesh_assemble(tv, tf)
    assert len(a) == 5 and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, want))
    g = torch.ops.diffusion_net.mesh_frames_gradients(tv, a[0], a[1], n)
    want = ops.mesh_frames_gradients(tv, a[0], a[1], n)
    assert len(g) == 3 and all(torch.equal(x, y) for x, y in zip(g, want))
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    with FakeTensorMode(shape_env=ShapeEnv(), allow_non_fake_inputs=False) as mode:
        fa = torch.ops.diffusion_net.mesh_assemble(mode.from_tensor(tv), mode.from_tensor(tf))
        fg = torch.ops.diffusion_net.mesh_frames_gradients(mode.from_tensor(tv), mode.from_tensor(a[0]), mode.from_tensor(a[1]), mode.from_tensor(n))
    assert tuple(fa[0].shape) == (201,) and fa[0].dtype == fa[1].dtype == torch.int32 and fa[1].dim() == 1 and fa[2].dim() == 1
    assert fa[2].dtype == fa[3].dtype == fa[4].dtype == torch.float64 and tuple(fa[3].shape) == (200,) and tuple(fa[4].shape) == (200, 3)
    assert tuple(fg[0].shape) == (200, 3, 3) and tuple(fg[1].shape) == tuple(a[1].shape) == tuple(fg[2].shape)
    assert all(t.dtype == torch.float64 for t in fg)


# ----------------------------------------------------------------------------------------------------------------- compute_operators_via
@functools.lru_cache(maxsize=None)
def sphere300():
    from diffusion_net import synthetic
    v, f = synthetic.sphere_mesh(300, seed=2)
    return v.astype(np.float32), f


@functools.lru_cache(maxsize=None)
def sphere300_host(k, eigensolver):
    from diffusion_net import geometry
    v, f = sphere300()
    return geometry.compute_operators_with(torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f)), k, eigensolver=eigensolver)


def run_compute_operators(dev, eigensolver):
    """``compute_operators_via(..., assembly="device")`` on a 300-vertex sphere: seven fp32 tensors on the device; eigenvalues as the host
    route's to the tolerance test_cloud_lap_gpu.py uses for the same comparison of a device route with the host route (rtol 1e-4 from the
    first non-zero one on, the eigenvalue 0 of the constants to 1e-4 of that one); eigenvectors orthonormal in the mass to 1e-4."""
    from diffusion_net import geometry
    v, f = sphere300()
    tv, tf = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev)
    V, K = 300, 16
    out = geometry.compute_operators_via(tv, tf, K, eigensolver=eigensolver, assembly="device")
    assert len(out) == 7
    for t, shape in zip(out, ((V, 3, 3), (V,), (V, V), (K,), (V, K), (V, V), (V, V))):
        assert t.dtype == torch.float32 and t.device == tv.device and tuple(t.shape) == shape
    for m in (out[2], out[5], out[6]):
        assert m.is_sparse and m.is_coalesced()
    host = sphere300_host(K, eigensolver)
    ev, ev_host = out[3].cpu().double().numpy(), host[3].double().numpy()
    print("mesh operators on %s (%s): device evals %s, host evals %s" % (dev, eigensolver, ev[:4], ev_host[:4]))
    assert np.allclose(ev[1:], ev_host[1:], rtol=1e-4, atol=0.0)
    assert abs(ev[0] - ev_host[0]) <= 1e-4 * ev_host[1]
    e, m = out[4].cpu().double(), out[1].cpu().double()
    assert torch.allclose(e.T @ (m[:, None] * e), torch.eye(K, dtype=torch.float64), atol=1e-4)
    for i in (0, 1, 2, 5, 6):                                    # the other five: one fp32 rounding of numbers that agree to fp64 round-off
        a, b = out[i].cpu(), host[i]
        a, b = (a.to_dense(), b.to_dense()) if a.is_sparse else (a, b)
        assert torch.allclose(a, b, rtol=2.0 ** -22, atol=1e-9), i
    return out


def run_cache_round_trip(dev, tmp_path):
    """``get_operators(..., assembly="device")`` writes an entry that the default route reads back; the keyword passes through
    ``get_all_operators``; a bad value raises everywhere."""
    import os
    import pytest
    from diffusion_net import geometry, precompute
    v, f = sphere300()
    tv, tf = torch.from_numpy(np.array(v)).to(dev), torch.from_numpy(np.array(f)).to(dev)
    first = geometry.get_operators(tv, tf, 8, op_cache_dir=str(tmp_path), assembly="device")
    assert len(os.listdir(tmp_path)) == 1
    real = precompute.compute_operators_with
    try:
        precompute.compute_operators_with = lambda *a, **k: pytest.fail("the cache was not used")
        again = geometry.get_operators(tv, tf, 8, op_cache_dir=str(tmp_path))
    finally:
        precompute.compute_operators_with = real
    for i in range(7):
        a, b = (again[i].to_dense(), first[i].to_dense()) if first[i].is_sparse else (again[i], first[i])
        assert torch.equal(a, b) and a.device == tv.device, i
    lists = geometry.get_all_operators([tv], [tf], 8, op_cache_dir=str(tmp_path), assembly="device")
    assert len(lists) == 7 and torch.equal(lists[1][0], first[1])
    cloud = geometry.compute_operators_via(tv[:60], tf[:0], 4, laplacian="delaunay", assembly="device")     # empty faces: accepted, the cloud's own route
    assert len(cloud) == 7 and tuple(cloud[4].shape) == (60, 4)
    for fn in (lambda: geometry.compute_operators_via(tv, tf, 8, assembly="host"), lambda: geometry.get_operators(tv, tf, 8, assembly="gpu"),
               lambda: geometry.get_all_operators([tv], [tf], 8, assembly=1)):
        with pytest.raises(ValueError, match="assembly"):
            fn()


def run_forward_backward(dev, operators, verts):
    import diffusion_net
    from diffusion_net import synthetic
    frames, massvec, L, evals, evecs, gX, gY = operators
    torch.manual_seed(4)
    model = diffusion_net.layers.DiffusionNet(3, 6, C_width=32, N_block=2, outputs_at="vertices", dropout=False)
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=4))
    model.to(dev).train()
    got = model(verts, massvec, L=L, evals=evals, evecs=evecs, gradX=gX, gradY=gY)
    assert tuple(got.shape) == (verts.shape[0], 6) and bool(torch.isfinite(got).all())
    got.square().mean().backward()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)

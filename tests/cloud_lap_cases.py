"""Shared bodies of the point-cloud Laplacian tests (drivers: test_cloud_lap_emu.py on the emulator build of dn_cloud_lap.hip,
test_cloud_lap_gpu.py on the device, test_cloud_lap_host.py for the numpy route and ``compute_operators(..., laplacian="delaunay")``).

The oracle is ``precompute.point_cloud_laplacian_from_table`` -- the numpy statement of the same construction in fp64 -- fed the SAME fp32
frames and neighbour table the kernels were given, so that the projected coordinates differ by fp64 round-off only (test_cloud_lap_host.py
ties the oracle's stars to ``scipy.spatial.Delaunay``).  ``check`` first asserts that every combinatorial decision of the input has a margin
far above that round-off (1e-15): the stars must then be identical, and the values are one fp32 rounding of the fp64 sums apart -- the bound
is 2^-23 T per entry, T the sum of the absolute terms of the entry (2^-24 for the rounding, a factor 2 of room).  Derived, not tuned."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

import helpers

EPS = 2.0 ** -23
INCIRCLE_MARGIN = 1e-10      # min |in-circle(a, b, c)| / max(W_a, W_b, W_c)^2
CROSS_MARGIN = 1e-8          # min |cross(a, b)| / sqrt(W_a W_b)

# (n, k, seed, kind)
CASES = [
    (9, 8, 1, "sphere"),      # smallest two-workgroup launch (8 points each) with a ragged tail
    (70, 32, 2, "sphere"),    # full lane groups
    (300, 16, 3, "sphere"),
    (257, 31, 4, "sphere"),   # odd everything
    (200, 12, 5, "plane"),    # noisy plane patch: hull points have open stars
]


def sample(n, seed, kind="sphere"):
    rs = np.random.RandomState(seed)
    if kind == "sphere":
        p = rs.randn(n, 3)
        p = p / np.linalg.norm(p, axis=1, keepdims=True)
    else:
        p = np.stack([rs.rand(n), rs.rand(n), 0.05 * rs.randn(n)], axis=1)
    return p.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- oracle and margins
def oracle(pts, nbr, frames):
    """(L csr fp64, mass fp64, parts) of the numpy route on this table and these frames."""
    from diffusion_net import precompute
    return precompute.point_cloud_laplacian_from_table(np.asarray(pts), np.asarray(nbr), np.asarray(frames), with_parts=True)


def decision_margins(pts, nbr, frames):
    """(smallest |in-circle| / max(W)^2 over all triples of distinct live slots, smallest |cross| / sqrt(W_a W_b) over all pairs)."""
    from diffusion_net import precompute
    X, Y, W = precompute.cloud_project(pts, nbr, frames)
    live = W > 0
    cr = X[:, :, None] * Y[:, None, :] - Y[:, :, None] * X[:, None, :]                    # [n, a, b]
    k = X.shape[1]
    off = ~np.eye(k, dtype=bool)[None]
    pair = live[:, :, None] & live[:, None, :] & off
    rel_cr = np.abs(cr) / np.sqrt(np.where(pair, W[:, :, None] * W[:, None, :], 1.0))
    m_cr = float(rel_cr[pair].min()) if pair.any() else np.inf
    # in-circle(a, b, c) = W_c cr(a,b) - W_b cr(a,c) + W_a cr(b,c)
    inc = (W[:, None, None, :] * cr[:, :, :, None] - W[:, None, :, None] * cr[:, :, None, :] + W[:, :, None, None] * cr[:, None, :, :])
    wmax = np.maximum(np.maximum(W[:, :, None, None], W[:, None, :, None]), W[:, None, None, :])
    tri = pair[:, :, :, None] & pair[:, :, None, :] & pair[:, None, :, :]
    rel_in = np.abs(inc) / np.where(tri, wmax, 1.0) ** 2
    m_in = float(rel_in[tri].min()) if tri.any() else np.inf
    return m_in, m_cr


def stars_of(partner):
    """partner [n, k] -> per point the set of its triangles as frozensets of two slots."""
    return [{frozenset((a, int(b))) for a, b in enumerate(row) if b >= 0} for row in np.asarray(partner)]


def csr_of(n, rowptr, col, val):
    return sp.csr_matrix((np.asarray(val), np.asarray(col), np.asarray(rowptr)), shape=(n, n))


def check_invariants(n, rowptr, col, val, mass, what):
    """The four invariants of the fp32 result, whatever the input: symmetric bit for bit, row sums and smallest eigenvalue within the entry
    rounding (Weyl: a symmetric perturbation E moves eigenvalues by at most ||E||_2 <= || |E| ||_inf <= 2^-24 || |L| ||_inf), mass >= 0."""
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32 and mass.dtype == np.float32
    assert rowptr.shape == (n + 1,) and rowptr[0] == 0 and rowptr[-1] == len(col) == len(val) and (np.diff(rowptr) >= 0).all()
    assert np.isfinite(val).all() and np.isfinite(mass).all(), what
    if len(col):
        assert col.min() >= 0 and col.max() < n
    for r in range(n):
        assert (np.diff(col[rowptr[r]:rowptr[r + 1]]) > 0).all(), "columns of row %d are not strictly ascending" % r
    D = np.zeros((n, n), dtype=np.float32)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    D[rows, col] = val
    assert np.array_equal(D.view(np.int32), np.ascontiguousarray(D.T).view(np.int32)), "%s: L != L^T bit for bit" % what
    D64 = D.astype(np.float64)
    absrow = np.abs(D64).sum(axis=1)
    rowsum = np.abs(D64.sum(axis=1))
    assert (rowsum <= EPS * absrow).all(), ("%s: row sums" % what, float((rowsum / np.maximum(absrow, 1e-300)).max()))
    lam = float(np.linalg.eigvalsh(D64).min()) if n else 0.0
    bound = EPS * float(absrow.max()) if n else 0.0
    assert lam >= -bound, ("%s: smallest eigenvalue" % what, lam, bound)
    assert (mass >= 0).all()
    return float((rowsum / np.maximum(EPS * absrow, 1e-300)).max()) if n else 0.0, lam, bound


# ----------------------------------------------------------------------------------------------------------------- running the kernels
def _np(t):
    return t.detach().cpu().numpy()


def inputs(dev, pts, k, frames=None):
    """The tensors the kernels are given: points, the table of ``ops.knn`` and the frames of ``ops.cloud_operators`` (or the caller's)."""
    from diffusion_net import ops
    t = torch.from_numpy(np.array(pts)).to(dev)
    nbr = ops.knn(t, t, k, omit_diagonal=True)[1]
    fr = ops.cloud_operators(t, nbr)[1] if frames is None else torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(dev)
    return t, nbr, fr


def run(t, nbr, fr):
    from diffusion_net import ops
    partner, rowptr, col, val, mass = ops.cloud_laplacian(t, nbr, fr)
    assert partner.device == rowptr.device == col.device == val.device == mass.device == t.device
    return dict(partner=_np(partner), rowptr=_np(rowptr), col=_np(col), val=_np(val), mass=_np(mass))


def check(dev, pts, k, case, frames=None):
    """Margins of the input, stars, values, invariants, repeatability."""
    n = len(pts)
    t, nbr, fr = inputs(dev, pts, k, frames)
    nbr_h, fr_h = _np(nbr), _np(fr)
    m_in, m_cr = decision_margins(pts, nbr_h, fr_h)
    print("cloud laplacian %s on %s: decision margins in-circle %.3e (needs %.0e), cross %.3e (needs %.0e)" % (
        case, dev, m_in, INCIRCLE_MARGIN, m_cr, CROSS_MARGIN))
    assert m_in >= INCIRCLE_MARGIN, "a triple of neighbours is nearly co-circular with its point: %.3e (change the seed, not the threshold)" % m_in
    assert m_cr >= CROSS_MARGIN, "two neighbours are nearly collinear with their point: %.3e (change the seed, not the threshold)" % m_cr
    L, mass, parts = oracle(pts, nbr_h, fr_h)
    got = run(t, nbr, fr)
    # stars
    assert got["partner"].dtype == np.int32 and got["partner"].shape == (n, k)
    assert stars_of(got["partner"]) == stars_of(parts["partner"]), "the stars differ from the oracle's"
    assert sum(len(s) for s in stars_of(got["partner"])) == int((got["partner"] >= 0).sum()), "a triangle was found by both of its slots"
    # values
    assert np.array_equal(got["rowptr"], L.indptr) and np.array_equal(got["col"], L.indices), "the pattern differs from the oracle's"
    T, Tm = parts["L_abs"].data, parts["mass_abs"]
    assert np.array_equal(parts["L_abs"].indices, L.indices)
    share_l = float((np.abs(got["val"].astype(np.float64) - L.data) / (EPS * T)).max()) if len(T) else 0.0
    live = Tm > 0
    share_m = float((np.abs(got["mass"].astype(np.float64) - mass)[live] / (EPS * Tm[live])).max()) if live.any() else 0.0
    assert (got["mass"][~live] == 0).all()
    # invariants of the fp32 result
    share_row, lam, lam_bound = check_invariants(n, got["rowptr"], got["col"], got["val"], got["mass"], case)
    print("cloud laplacian %s on %s: %d triangles, %d entries; values %.3f of the bound, mass %.3f, row sums %.3f; smallest eigenvalue %.3e (bound -%.3e)" % (
        case, dev, int((got["partner"] >= 0).sum()), len(T), share_l, share_m, share_row, lam, lam_bound))
    helpers.record_margin("cloud_lap_" + case, dev, n=n, k=k, incircle_margin=m_in, cross_margin=m_cr, val_share_of_bound=share_l,
                          mass_share_of_bound=share_m, rowsum_share_of_bound=share_row, min_eig=lam, min_eig_bound=-lam_bound, bound=EPS)
    assert share_l <= 1.0, ("values", share_l)
    assert share_m <= 1.0, ("mass", share_m)
    # repeatability
    again = run(t, nbr, fr)
    for key in got:
        assert np.array_equal(got[key].view(np.int32), again[key].view(np.int32)), "%s differs between two calls" % key
    return got


def run_case(dev, n, k, seed, kind):
    check(dev, sample(n, seed, kind), k, "n%d_k%d_%s" % (n, k, kind))


def run_k1(dev):
    """One neighbour: no triangle exists.  L has no entry, the mass is zero, the status word is 0."""
    from diffusion_net import ops
    pts = sample(20, 6)
    t, nbr, fr = inputs(dev, pts, 1)
    got = run(t, nbr, fr)
    assert (got["partner"] == -1).all() and got["partner"].shape == (20, 1)
    assert len(got["col"]) == 0 and len(got["val"]) == 0 and (got["rowptr"] == 0).all() and (got["mass"] == 0).all()
    out = ops._cloud_laplacian_launch(t, nbr, fr)
    assert int(out[6].item()) == 0 and int(out[5].item()) == 0


def run_k2(dev):
    """Two neighbours: every lane has at most one possible partner, every point at most one triangle."""
    got = check(dev, sample(50, 7), 2, "n50_k2")
    assert ((got["partner"] >= 0).sum(axis=1) <= 1).all() and (got["partner"] >= 0).any()


def run_given_frames(dev):
    """Caller-given frames -- those of arbitrary unit normals, NOT the surface's: the stars are those of these projections."""
    from diffusion_net import precompute
    pts = sample(64, 8)
    nrm = np.random.RandomState(11).randn(64, 3)
    frames = precompute.tangent_frames(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    check(dev, pts, 20, "given_frames_n64_k20", frames=frames)


DEGENERATE = ("grid", "collinear", "coincident", "duplicates")


def degenerate_points(name):
    if name == "grid":                     # 6 x 6 regular grid: co-circular quadruples everywhere (coordinates exact in fp32)
        g = np.arange(6) / 8.0
        return np.stack([np.repeat(g, 6), np.tile(g, 6), np.zeros(36)], axis=1).astype(np.float32), 12
    if name == "collinear":
        return (np.arange(50)[:, None] * (np.array([1.0, 2.0, 3.0]) / 8.0)[None, :]).astype(np.float32), 30
    if name == "coincident":
        return np.zeros((40, 3), dtype=np.float32) + np.float32(0.25), 30
    half = sample(100, 9)
    return np.concatenate([half, half[:20]]), 16


def run_degenerate(dev, name):
    """No oracle equality (ties are decided by round-off): finite values, the four invariants, status 0."""
    from diffusion_net import ops
    pts, k = degenerate_points(name)
    t, nbr, fr = inputs(dev, pts, k)
    got = run(t, nbr, fr)                                        # (raises IndexError on a non-zero status word)
    assert int(ops._cloud_laplacian_launch(t, nbr, fr)[6].item()) == 0
    share_row, lam, bound = check_invariants(len(pts), got["rowptr"], got["col"], got["val"], got["mass"], name)
    print("cloud laplacian degenerate %s on %s: %d triangles, %d entries, smallest eigenvalue %.3e (bound -%.3e)" % (
        name, dev, int((got["partner"] >= 0).sum()), len(got["col"]), lam, bound))
    if name in ("collinear", "coincident"):
        assert (got["partner"] == -1).all() and len(got["col"]) == 0 and (got["mass"] == 0).all()
    if name == "grid":
        assert (got["partner"] >= 0).any() and got["mass"].sum() > 0


def _expected_from_partner(pts, nbr, partner):
    from diffusion_net import precompute
    n = len(pts)
    (rows, cols, vals), (mv, mw) = precompute.cloud_laplacian_terms(pts, nbr, partner)
    L = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    T = sp.coo_matrix((np.abs(vals), (rows, cols)), shape=(n, n)).tocsr()
    L.sort_indices()
    T.sort_indices()
    return L, T, np.bincount(mv, weights=mw, minlength=n)


def run_bad_indices(dev):
    """A neighbour equal to i is legal: the slot takes no part.  An index outside [0, n) empties the star of its row and counts in the status
    word, which ``ops.cloud_laplacian`` turns into IndexError; the other rows are untouched and the matrix is the sum over their stars."""
    from diffusion_net import ops
    pts = sample(64, 8)
    t, nbr, fr = inputs(dev, pts, 20)
    clean = run(t, nbr, fr)
    own = nbr.clone()
    own[5, 3] = 5
    got = run(t, own, fr)
    _, _, parts = oracle(pts, _np(own), _np(fr))
    assert got["partner"][5, 3] == -1 and (got["partner"][5] != 3).all()
    assert stars_of(got["partner"]) == stars_of(parts["partner"])
    keep = np.arange(64) != 5
    assert np.array_equal(got["partner"][keep], clean["partner"][keep])
    check_invariants(64, got["rowptr"], got["col"], got["val"], got["mass"], "own index")

    for value, rows in ((64, [7]), (-1, [7, 40])):
        bad = nbr.clone()
        for r in rows:
            bad[r, 0] = value
        try:
            ops.cloud_laplacian(t, bad, fr)
        except IndexError as err:
            assert ("%d row" % len(rows)) in str(err)
        else:
            raise AssertionError("an index outside [0, n) was accepted")
        partner, rowptr, col, val, mass, count, status = ops._cloud_laplacian_launch(t, bad, fr)
        assert int(status.item()) == len(rows)
        partner, nnz = _np(partner), int(count.item())
        keep = ~np.isin(np.arange(64), rows)
        assert (partner[~keep] == -1).all() and np.array_equal(partner[keep], clean["partner"][keep])
        # ... and the matrix is exactly the sum over the stars that are left (a valid index in place of the bad one: its row has no star)
        L, T, m = _expected_from_partner(pts, np.where((_np(bad) < 0) | (_np(bad) >= 64), 0, _np(bad)), partner)
        rowptr, col, val, mass = _np(rowptr), _np(col)[:nnz], _np(val)[:nnz], _np(mass)
        assert np.array_equal(rowptr, L.indptr) and np.array_equal(col, L.indices)
        assert (np.abs(val.astype(np.float64) - L.data) <= EPS * T.data).all() and (np.abs(mass.astype(np.float64) - m) <= EPS * m).all()
        check_invariants(64, rowptr, col, val, mass, "bad index")


def run_ops_validation(dev):
    from diffusion_net import ops
    t, nbr, fr = inputs(dev, sample(40, 1), 5)
    for args, exc in (((t[:, :2], nbr, fr), ValueError), ((t, nbr[:30], fr), ValueError), ((t, nbr.int(), fr), TypeError),
                      ((t.double(), nbr, fr), TypeError), ((t, nbr, fr[:10]), ValueError), ((t, nbr[:, :0], fr), ValueError),
                      ((t, nbr, fr.double()), TypeError)):
        try:
            ops.cloud_laplacian(*args)
        except exc:
            continue
        raise AssertionError("ops.cloud_laplacian accepted %s" % (tuple(tuple(a.shape) for a in args),))
    out = ops.cloud_laplacian(t[:0], nbr[:0], fr[:0])
    assert out[0].shape == (0, 5) and out[1].tolist() == [0] and out[2].numel() == 0 and out[3].numel() == 0 and out[4].shape == (0,)


def run_sparse_equals_raw(dev):
    """``geometry.point_cloud_laplacian`` returns the raw CSR of ``ops.cloud_laplacian`` as a coalesced sparse COO, bit for bit -- with
    the frames it estimates itself and with the caller's."""
    import diffusion_net
    pts = sample(257, 4)
    t, nbr, fr = inputs(dev, pts, 31)
    raw = run(t, nbr, fr)
    rows = np.repeat(np.arange(257), np.diff(raw["rowptr"]))
    for frames in (None, fr):
        L, mass = diffusion_net.geometry.point_cloud_laplacian(t, 31, frames=frames)
        assert L.is_sparse and L.is_coalesced() and L.dtype == torch.float32 and tuple(L.shape) == (257, 257)
        assert L.device == t.device and mass.device == t.device and mass.dtype == torch.float32
        idx = _np(L.indices())
        assert np.array_equal(idx[0], rows) and np.array_equal(idx[1], raw["col"])
        assert np.array_equal(_np(L.values()).view(np.int32), raw["val"].view(np.int32))
        assert np.array_equal(_np(mass).view(np.int32), raw["mass"].view(np.int32))


def run_abi_errors():
    """Every non-zero return of the four entry points, through ctypes, on host buffers: nothing is launched, the outputs keep their fill."""
    from diffusion_net import _hip
    L = _hip.lib()
    n, k = 40, 5
    pts = torch.from_numpy(sample(n, 1))
    nbr = torch.zeros(n, 32, dtype=torch.int64)
    frames = torch.zeros(n, 9)
    ws_bytes = L.dn_cloud_laplacian_workspace_bytes(n, k)
    assert ws_bytes == 192 * n * k
    for bad in ((n, 0), (n, 33), (-1, k), (10_000_000, 30)):
        assert L.dn_cloud_laplacian_workspace_bytes(*bad) == 0
    fill = dict(partner=torch.full((n, 32), -7, dtype=torch.int32), status=torch.full((1,), -7, dtype=torch.int32),
                ws=torch.full((ws_bytes,), 0xF9, dtype=torch.uint8), rowptr=torch.full((n + 1,), -7, dtype=torch.int32),
                col=torch.full((64,), -7, dtype=torch.int32), out=torch.full((64,), -7.0), count=torch.full((1,), -7, dtype=torch.int32))
    p = lambda key, null: None if key == null else fill[key].data_ptr()

    def star(n_=n, k_=k, pts_=pts, nbr_=nbr, frames_=frames, null=None):
        return L.dn_cloud_star_f32(_hip.ptr(pts_), n_, _hip.ptr(nbr_), k_, _hip.ptr(frames_), p("partner", null), p("status", null), None)

    def emit(n_=n, k_=k, pts_=pts, nbr_=nbr, partner_=fill["partner"], null=None, bytes_=ws_bytes):
        return L.dn_cloud_laplacian_emit_f32(_hip.ptr(pts_), n_, _hip.ptr(nbr_), k_, _hip.ptr(partner_), p("ws", null), bytes_, None)

    for call in (star, emit):
        assert call(k_=0) != 0                                   # k < 1
        assert call(k_=33) != 0                                  # k > DN_KNN_MAX_K
        assert call(n_=-1) != 0                                  # n < 0
        assert call(n_=10_000_000, k_=30) != 0                   # 9 n k > INT32_MAX
        assert call(pts_=None) != 0 and call(nbr_=None) != 0     # a required pointer is NULL
        assert call(n_=0) == 0                                   # n == 0: success, nothing launched
    assert star(frames_=None) != 0 and star(null="partner") != 0 and star(null="status") != 0
    assert star(n_=0, pts_=None, nbr_=None, frames_=None, null="status") == 0
    assert emit(partner_=None) != 0 and emit(null="ws") != 0
    assert emit(bytes_=ws_bytes - 1) != 0                        # a workspace smaller than the query says
    assert emit(n_=0, pts_=None, nbr_=None, partner_=None, null="ws", bytes_=0) == 0

    m = 12
    keys, perm, vals, rank = torch.zeros(m, dtype=torch.int64), torch.arange(m), torch.zeros(m, dtype=torch.float64), torch.ones(m, dtype=torch.int64)

    def seg(keys_=keys, perm_=perm, vals_=vals, m_=m, rank_=rank, rows_=n, csr=True, null=None):
        outs = [p(key, null) if (csr or key == "out") else None for key in ("rowptr", "col", "out", "count")]
        return L.dn_segment_sum_f64_f32(_hip.ptr(keys_), _hip.ptr(perm_), _hip.ptr(vals_), m_, _hip.ptr(rank_), rows_, *outs, None)

    assert seg(m_=-1) != 0 and seg(rows_=-1) != 0                # negative counts
    for kw in (dict(keys_=None), dict(perm_=None), dict(vals_=None), dict(rank_=None), dict(null="col"), dict(null="out"), dict(null="count")):
        assert seg(**kw) != 0, kw                                # a pointer the CSR form uses is NULL
    for kw in (dict(keys_=None), dict(perm_=None), dict(vals_=None), dict(null="out")):
        assert seg(csr=False, **kw) != 0, kw                     # ... and the dense form
    assert seg(m_=0, rows_=0, keys_=None, perm_=None, vals_=None, rank_=None, csr=False, null="out") == 0   # nothing to do: success
    for key, t in fill.items():
        assert bool((t == (0xF9 if key == "ws" else -7)).all()), key

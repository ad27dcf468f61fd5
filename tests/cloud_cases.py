"""Shared bodies of the point-cloud operator tests (drivers: test_cloud_emu.py on the emulator build of dn_cloud.hip, test_cloud_gpu.py on
the device, test_cloud_host.py for the host routes and ``compute_operators``).

The truth is the reference's arithmetic in fp64 on the same fp32 points: recorded from the reference itself for the fixture's clouds
(tests/golden/geom_cloud_ref.npz, ``ref64/``), and computed by the package's host route in fp64 for the others (test_cloud_host.py ties that
route to the fixture).  The kernel is fp64 inside and rounds once at the store, so every tolerance is ONE fp32 rounding, doubled:
2^-23 for a component of magnitude <= 1, 2^-23 of the largest entry of its row for a gradient coefficient.  They are derived, not tuned.
``check_cloud`` first asserts that the input is well conditioned for such a comparison and fails loudly if it is not."""
import functools
import os

import numpy as np
import scipy.sparse as sp
import torch

import helpers
import knn_cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -23
KNN_BOUND = knn_cases.rel_bound(3)          # 4.2e-7: what the kNN kernel's fp32 distances are good for

# (N, k, seed, axes, noise): the smallest shapes at which the kernel can still go wrong
CASES = [
    (31, 30, 4, (1.0, 1.0, 1.0), 0.0),      # every other point is a neighbour
    (64, 30, 3, (1.0, 0.7, 0.5), 0.01),     # ellipsoid with noise: neighbourhoods that are far from planar
    (257, 32, 3, (1.0, 1.0, 1.0), 0.0),     # k at the limit, ragged last workgroup (8 points each)
    (100, 3, 3, (1.0, 1.0, 1.0), 0.0),      # fewest neighbours that fix a plane
    (100, 2, 7, (1.0, 0.7, 0.5), 0.0),      # (seed 7: with two neighbours many seeds hold a nearly collinear triple, which the checker's conditions refuse)
]


def sample(N, seed, axes=(1.0, 1.0, 1.0), noise=0.0):
    """N points of the ellipsoid with these axes (directions uniform on the sphere), optional Gaussian noise, rounded to fp32
    (the same construction as tests/golden/make_cloud_golden.py)."""
    rs = np.random.RandomState(seed)
    p = rs.randn(N, 3)
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * np.asarray(axes)
    if noise:
        p = p + noise * rs.randn(N, 3)
    return p.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------- the truth
def _csr(rows, cols, vals, n):
    return sp.coo_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n, n)).tocsr()


def truth_from_host_route(pts, k, normals=None):
    """The package's host route on the points in fp64 -> dict(nbr, normals, frames, gx, gy); gx / gy scipy CSR."""
    import diffusion_net
    v = torch.from_numpy(np.asarray(pts, dtype=np.float64))
    nrm = None if normals is None else torch.from_numpy(np.asarray(normals, dtype=np.float64))
    frames, gX, gY = diffusion_net.geometry.cloud_operators(v, k, normals=nrm)
    assert frames.dtype == torch.float64 and not frames.is_cuda
    nbr = diffusion_net.geometry.find_knn(v, v, k, omit_diagonal=True, method="cpu_kd").indices.numpy()
    n = len(pts)
    csr = lambda t: _csr(t.indices()[0].numpy(), t.indices()[1].numpy(), t.values().numpy(), n)
    return dict(nbr=nbr, normals=frames[:, 2].numpy(), frames=frames.numpy(), gx=csr(gX), gy=csr(gY))


@functools.lru_cache(maxsize=None)
def truth_of_case(N, k, seed, axes, noise):
    pts = sample(N, seed, axes, noise)
    pts.setflags(write=False)
    return pts, truth_from_host_route(pts, k)


@functools.lru_cache(maxsize=None)
def golden():
    """name -> (pts, k, ref64 truth dict, ref32 dict, dev_normals, dev_grad) of the reference's recorded runs."""
    z = np.load(os.path.join(GOLDEN, "geom_cloud_ref.npz"))
    out = {}
    for name in z["cases"]:
        name = str(name)
        pts, k = z[name + "/pts"], int(z[name + "/k"])
        recs = []
        for tag in ("ref64", "ref32"):
            g = lambda key: z["%s/%s/%s" % (name, tag, key)]
            grad = sp.csc_matrix((g("grad_data"), g("grad_indices"), g("grad_indptr")), shape=(len(pts), len(pts)))
            recs.append(dict(nbr=g("nbr"), normals=g("normals"), frames=g("frames"), gx=sp.csr_matrix(grad.real), gy=sp.csr_matrix(grad.imag)))
        out[name] = (pts, k, recs[0], recs[1], float(z[name + "/dev_normals"]), float(z[name + "/dev_grad"]))
    return out


# ----------------------------------------------------------------------------------------------------------------- the checker
def assert_conditions(pts, k, truth, estimated=True):
    """What the comparison hinges on, on the fp64 truth; every point counts, none is left out."""
    from sklearn.neighbors import KDTree
    p = np.asarray(pts, dtype=np.float64)
    n = len(p)
    if estimated:      # relative gap of the two smallest eigenvalues of P^T P (squared singular values of the neighbourhood), in units of the largest
        P = p[truth["nbr"]] - p[:, None, :]
        lam = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", P, P))
        sgap = float(((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min())
        print("cloud conditions: smallest singular gap %.3e" % sgap)
        assert sgap > 1e-3, "a neighbourhood has no well-defined normal: singular gap %.3e" % sgap
    if n - 1 > k:      # relative gap between the k-th and the (k+1)-th neighbour: the choice of neighbours is then the same in fp32
        d = KDTree(p).query(p, k=k + 2)[0]
        ngap = float(((d[:, k + 1] - d[:, k]) / d[:, k]).min())
        print("cloud conditions: smallest neighbour gap %.3e (kNN bound %.3e)" % (ngap, KNN_BOUND))
        assert ngap > 2 * KNN_BOUND, "the k-th and (k+1)-th neighbour of a point are too close: %.3e" % ngap
    xgap = float(np.abs(np.abs(truth["normals"][:, 0]) - 0.9).min())
    print("cloud conditions: min | |n_x| - 0.9 | = %.3e" % xgap)
    assert xgap > 1e-5, "a normal sits on the switch between the two frame candidates: %.3e" % xgap


def _row_top(m):
    return np.asarray(abs(m).max(axis=1).todense()).reshape(-1)


def check_cloud(pts, k, got, truth, case, device, normals_in=None):
    """Items 1-3 of the checker.  ``got``: dict(normals, frames [n,3,3], gx, gy scipy CSR with equal columns of a row summed) and, where the
    raw kernel outputs are at hand, rowptr / col / nbr (the table the kernel was given).  Returns the measured margins (shares of the bounds)."""
    n = len(pts)
    assert_conditions(pts, k, truth, estimated=normals_in is None)
    nd, fd = np.asarray(got["normals"], dtype=np.float64), np.asarray(got["frames"], dtype=np.float64)
    n64, f64 = truth["normals"].astype(np.float64), truth["frames"].astype(np.float64)
    assert got["normals"].dtype == np.float32 and got["frames"].dtype == np.float32
    assert nd.shape == (n, 3) and fd.shape == (n, 3, 3)
    assert np.isfinite(nd).all() and np.isfinite(fd).all()
    s = np.sign(np.einsum("ij,ij->i", nd, n64))
    # 1. normals
    if normals_in is not None:
        assert np.array_equal(got["normals"], normals_in), "normals_in was not copied to the output"
        assert (s == 1).all()
    else:
        lead = np.sort(np.abs(n64), axis=1)
        clear = lead[:, 2] - lead[:, 1] > 1e-3
        top = np.abs(n64).argmax(axis=1)
        assert (nd[np.arange(n), top][clear] > 0).all(), "sign rule: the component of largest magnitude must be positive"
        e_unit = float(np.abs(np.linalg.norm(nd, axis=1) - 1.0).max())
        assert e_unit <= 2 * EPS, ("normal not unit", e_unit)
    e_n = float(np.abs(s[:, None] * nd - n64).max())
    # 2. frames (the 1e-6 in basisX's denominator included: the truth carries it)
    sf = np.stack([np.ones(n), s, s], axis=1)[:, :, None]
    e_f = float(np.abs(sf * fd - f64).max())
    assert np.array_equal(got["frames"][:, 2], got["normals"])
    # 3. gradient rows
    if "col" in got:
        assert got["rowptr"].dtype == np.int32 and got["col"].dtype == np.int32
        assert np.array_equal(got["rowptr"], np.arange(n + 1, dtype=np.int64) * (k + 1))
        col = got["col"].reshape(n, k + 1)
        assert np.array_equal(col[:, 0], np.arange(n)) and np.array_equal(col[:, 1:], got["nbr"]), "column layout: i, then the neighbours in nbr order"
        assert np.array_equal(np.sort(got["nbr"], axis=1), np.sort(truth["nbr"], axis=1)), "the neighbour sets differ from the fp64 truth"
    S = sp.diags(s)
    e_g = 0.0
    for part, dev, ref in (("x", got["gx"], truth["gx"]), ("y", S @ got["gy"], truth["gy"])):
        assert np.isfinite(dev.data).all()
        top = _row_top(ref)
        assert (top > 0).all()
        diff = _row_top(sp.csr_matrix(dev - ref))
        e_g = max(e_g, float((diff / top).max()))
    print("cloud check %s on %s: normals %.3e frames %.3e (bound %.3e), gradient rows %.3e of the row's largest (bound %.3e)" % (
        case, device, e_n, e_f, EPS, e_g, EPS))
    helpers.record_margin("cloud_" + case, device, n=n, k=k, normals_err=e_n, frames_err=e_f, grad_rel_row_err=e_g, bound=EPS)
    assert e_n <= EPS, ("normals", e_n)
    assert e_f <= EPS, ("frames", e_f)
    assert e_g <= EPS, ("gradient rows", e_g)
    return e_n, e_f, e_g


# ----------------------------------------------------------------------------------------------------------------- running the kernel
def _kernel(dev, pts, k, normals=None, nbr=None):
    """ops.knn + ops.cloud_operators on ``dev`` -> dict of numpy arrays as ``check_cloud`` takes them."""
    from diffusion_net import ops
    t = torch.from_numpy(np.array(pts)).to(dev)
    if nbr is None:
        nbr = ops.knn(t, t, k, omit_diagonal=True)[1]
    nrm = None if normals is None else torch.from_numpy(np.ascontiguousarray(normals)).to(dev)
    normals_o, frames, rowptr, col, vx, vy = ops.cloud_operators(t, nbr.to(dev), nrm)
    return raw_to_got(len(pts), k, nbr, normals_o, frames, rowptr, col, vx, vy)


def raw_to_got(n, k, nbr, normals, frames, rowptr, col, vx, vy):
    c = lambda a: a.detach().cpu().numpy()
    rows = np.repeat(np.arange(n), k + 1)
    return dict(nbr=c(nbr), normals=c(normals), frames=c(frames), rowptr=c(rowptr), col=c(col), vx=c(vx), vy=c(vy),
                gx=_csr(rows, c(col), c(vx), n), gy=_csr(rows, c(col), c(vy), n))


def sparse_to_got(frames, gX, gY):
    """The results of ``geometry.cloud_operators`` as ``check_cloud`` takes them."""
    n = frames.shape[0]
    csr = lambda t: _csr(t.indices()[0].cpu().numpy(), t.indices()[1].cpu().numpy(), t.values().cpu().numpy(), n)
    f = frames.detach().cpu().numpy()
    return dict(normals=np.ascontiguousarray(f[:, 2]), frames=f, gx=csr(gX), gy=csr(gY))


def run_case(dev, N, k, seed, axes, noise):
    pts, truth = truth_of_case(N, k, seed, axes, noise)
    got = _kernel(dev, pts, k)
    check_cloud(pts, k, got, truth, "n%d_k%d" % (N, k), dev)
    again = _kernel(dev, pts, k)                                   # two runs give identical bits
    for key in ("normals", "frames", "rowptr", "col", "vx", "vy"):
        assert np.array_equal(got[key].view(np.int32), again[key].view(np.int32)), key


def run_reference_fixture(dev):
    """The kernel on the fixture's clouds against the reference's recorded fp64 outputs, under the same checker."""
    for name, (pts, k, ref64, _, _, _) in golden().items():
        check_cloud(pts, k, _kernel(dev, pts, k), ref64, "fixture_" + name, dev)


def run_single_point_is_rejected(dev):
    from diffusion_net import ops
    t = torch.zeros(1, 3).to(dev)
    try:
        ops.knn(t, t, 1, omit_diagonal=True)
    except ValueError as err:
        assert "0 candidates" in str(err)
    else:
        raise AssertionError("one point has no neighbour: kNN must refuse k = 1")


def run_given_normals(dev):
    """normals_in: arbitrary unit vectors, NOT the surface's -- the estimate must be skipped and the frames be those of the given normals."""
    pts, _ = truth_of_case(64, 30, 3, (1.0, 0.7, 0.5), 0.01)
    rs = np.random.RandomState(11)
    nrm = rs.randn(64, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    truth = truth_from_host_route(pts, 30, normals=nrm)
    check_cloud(pts, 30, _kernel(dev, pts, 30, normals=nrm), truth, "given_normals_n64_k30", dev, normals_in=nrm)


def run_sparse_equals_raw(dev):
    """Item 4: the coalesced gradX / gradY of ``geometry.cloud_operators`` are the raw arrays summed by (row, column); a neighbour table
    cannot hold i itself after ``omit_diagonal``, so here the sum has one term per entry and the bits must agree."""
    import diffusion_net
    pts, truth = truth_of_case(257, 32, 3, (1.0, 1.0, 1.0), 0.0)
    raw = _kernel(dev, pts, 32)
    frames, gX, gY = diffusion_net.geometry.cloud_operators(torch.from_numpy(np.array(pts)).to(dev), 32)
    assert gX.is_coalesced() and gY.is_coalesced() and gX.dtype == torch.float32 and tuple(gX.shape) == (257, 257)
    assert str(gX.device) == str(frames.device) == str(torch.from_numpy(np.array(pts)).to(dev).device)
    got = sparse_to_got(frames, gX, gY)
    assert np.array_equal(got["frames"], raw["frames"])
    for a, b in ((got["gx"], raw["gx"]), (got["gy"], raw["gy"])):
        assert (a != b).nnz == 0
    check_cloud(pts, 32, got, truth, "geometry_route_n257_k32", dev)
    normals = diffusion_net.geometry.vertex_normals(torch.from_numpy(np.array(pts)).to(dev), torch.zeros(0, 3, dtype=torch.long), 32)
    assert np.array_equal(normals.cpu().numpy(), raw["normals"])


def run_collinear(dev):
    """50 points on a line (coordinates exact in fp32): rank-1 neighbourhoods.  Finite outputs, unit normal orthogonal to the line."""
    direction = np.array([1.0, 2.0, 3.0]) / 8.0
    pts = (np.arange(50)[:, None] * direction[None, :]).astype(np.float32)
    got = _kernel(dev, pts, 30)
    for key in ("normals", "frames", "vx", "vy"):
        assert np.isfinite(got[key]).all(), key
    nd = got["normals"].astype(np.float64)
    assert float(np.abs(np.linalg.norm(nd, axis=1) - 1.0).max()) <= 2 * EPS
    off = float(np.abs(nd @ (direction / np.linalg.norm(direction))).max())
    print("collinear: largest |n . line| = %.3e" % off)
    assert off <= 1e-6
    one = np.zeros((40, 3), dtype=np.float32) + np.float32(0.25)          # coincident points: the zero matrix
    got = _kernel(dev, one, 30)
    for key in ("normals", "frames", "vx", "vy"):
        assert np.isfinite(got[key]).all(), key
    assert float(np.abs(np.linalg.norm(got["normals"].astype(np.float64), axis=1) - 1.0).max()) <= 2 * EPS
    assert (got["vx"] == 0).all() and (got["vy"] == 0).all()


def run_duplicates(dev):
    """Every point present twice: zero-length edges.  All outputs finite; the twin's coefficient is exactly 0."""
    half = sample(60, 8)
    pts = np.concatenate([half, half])
    got = _kernel(dev, pts, 30)
    for key in ("normals", "frames", "vx", "vy"):
        assert np.isfinite(got[key]).all(), key
    twin = (np.arange(120) + 60) % 120
    col = got["col"].reshape(120, 31)
    hit = col == twin[:, None]
    assert (hit.sum(axis=1) == 1).all(), "the twin at distance 0 is a neighbour of every point"
    assert (got["vx"].reshape(120, 31)[hit] == 0).all() and (got["vy"].reshape(120, 31)[hit] == 0).all()
    assert np.abs(got["vx"]).max() > 0


def run_bad_indices(dev):
    """A neighbour equal to i is legal (the reference's dropped tail == tip edge): column i, value 0.  An index outside [0, n) zeroes its
    row and counts in the status word, which ``ops.cloud_operators`` turns into IndexError."""
    from diffusion_net import ops
    pts, _ = truth_of_case(64, 30, 3, (1.0, 0.7, 0.5), 0.01)
    t = torch.from_numpy(np.array(pts)).to(dev)
    nbr = ops.knn(t, t, 30, omit_diagonal=True)[1]
    clean = _kernel(dev, pts, 30, nbr=nbr)
    own = nbr.clone()
    own[5, 3] = 5
    got = _kernel(dev, pts, 30, nbr=own)
    col, vx, vy = got["col"].reshape(64, 31), got["vx"].reshape(64, 31), got["vy"].reshape(64, 31)
    assert col[5, 4] == 5 and vx[5, 4] == 0 and vy[5, 4] == 0 and np.isfinite(vx).all() and np.isfinite(vy).all()
    keep = np.arange(64) != 5
    assert np.array_equal(vx[keep], clean["vx"].reshape(64, 31)[keep]) and np.array_equal(got["normals"][keep], clean["normals"][keep])
    # ... and the whole operator is the stencil over the remaining edges: the package's host gradient (which drops tail == tip) on this
    # table, in the frames of the SAME fp32 normals, which the kernel is handed as normals_in
    from diffusion_net import precompute
    nrm = clean["normals"]
    got = _kernel(dev, pts, 30, normals=nrm, nbr=own)
    edges = np.stack([np.repeat(np.arange(64), 30), own.cpu().numpy().reshape(-1)])
    ref = precompute.gradient_operator(pts.astype(np.float64), precompute.tangent_frames(nrm.astype(np.float64)), edges)
    for dev_m, ref_m in ((got["gx"], sp.csr_matrix(ref.real)), (got["gy"], sp.csr_matrix(ref.imag))):
        assert float((_row_top(sp.csr_matrix(dev_m - ref_m)) / _row_top(ref_m)).max()) <= EPS

    for value, rows in ((64, [7]), (-1, [7, 40])):
        bad = nbr.clone()
        for r in rows:
            bad[r, 0] = value
        try:
            ops.cloud_operators(t, bad)
        except IndexError as err:
            assert ("%d row" % len(rows)) in str(err)
        else:
            raise AssertionError("an index outside [0, n) was accepted")
        normals, frames, rowptr, c, x, y, status = ops._cloud_launch(t, bad, None)
        assert int(status.item()) == len(rows)
        c, x, y = c.cpu().numpy().reshape(64, 31), x.cpu().numpy().reshape(64, 31), y.cpu().numpy().reshape(64, 31)
        for r in rows:
            assert (c[r] == 0).all() and (x[r] == 0).all() and (y[r] == 0).all()
            assert (normals[r] == 0).all() and (frames[r] == 0).all()
        keep = ~np.isin(np.arange(64), rows)
        assert np.array_equal(x[keep], clean["vx"].reshape(64, 31)[keep]) and np.array_equal(c[keep], clean["col"].reshape(64, 31)[keep])
        assert np.array_equal(rowptr.cpu().numpy(), clean["rowptr"])


def run_ops_validation(dev):
    from diffusion_net import ops
    t = torch.from_numpy(sample(40, 1)).to(dev)
    nbr = ops.knn(t, t, 5, omit_diagonal=True)[1]
    for args, exc in (((t[:, :2], nbr), ValueError), ((t, nbr[:30]), ValueError), ((t, nbr.int()), TypeError), ((t.double(), nbr), TypeError),
                      ((t, nbr, t[:10]), ValueError), ((t, nbr[:, :0]), ValueError)):
        try:
            ops.cloud_operators(*args)
        except exc:
            continue
        raise AssertionError("ops.cloud_operators accepted %s" % (tuple(tuple(a.shape) for a in args),))
    out = ops.cloud_operators(t[:0], nbr[:0])
    assert out[0].shape == (0, 3) and out[2].tolist() == [0] and out[3].numel() == 0


def run_abi_errors():
    """Every non-zero return of dn_cloud_operators_f32, through ctypes, on host buffers: nothing is launched, the outputs keep their fill."""
    from diffusion_net import _hip
    L = _hip.lib()
    n, k = 40, 5
    pts = torch.from_numpy(sample(n, 1))
    nbr = torch.zeros(n, 32, dtype=torch.int64)
    fill = dict(normals=torch.full((n, 3), -7.0), frames=torch.full((n, 9), -7.0), rowptr=torch.full((n + 1,), -7, dtype=torch.int32),
                col=torch.full((n * 33,), -7, dtype=torch.int32), vx=torch.full((n * 33,), -7.0), vy=torch.full((n * 33,), -7.0),
                status=torch.full((1,), -7, dtype=torch.int32))
    order = ("normals", "frames", "rowptr", "col", "vx", "vy", "status")

    def call(n_=n, k_=k, pts_=pts, nbr_=nbr, null=None):
        outs = [None if key == null else fill[key].data_ptr() for key in order]
        return L.dn_cloud_operators_f32(_hip.ptr(pts_), n_, _hip.ptr(nbr_), k_, None, *outs, None)

    assert call(k_=0) != 0                                   # k < 1
    assert call(k_=33) != 0                                  # k > DN_KNN_MAX_K
    assert call(n_=-1) != 0                                  # n < 0
    assert call(n_=70_000_000, k_=30) != 0                   # n (k + 1) > INT32_MAX
    assert call(pts_=None) != 0 and call(nbr_=None) != 0     # a required pointer is NULL
    for key in order:
        assert call(null=key) != 0, key
    assert call(n_=0) == 0 and call(n_=0, pts_=None, nbr_=None, null="status") == 0   # n == 0: success, nothing launched
    for key, t in fill.items():
        assert bool((t == -7).all()), key

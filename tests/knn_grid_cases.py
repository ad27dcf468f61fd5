"""Shared bodies of the cell-grid k-nearest-neighbour tests (drivers: test_knn_grid_emu.py on the emulator build, test_knn_grid_gpu.py on
the device, test_knn_grid_host.py for what needs neither).

The yardstick is twofold for every result: ``torch.equal`` of distances and of indices with ``ops.knn`` (dn_knn.hip, brute force) on the
same inputs, and ``knn_cases.check_knn`` against fp64 brute force with its derived bound (D + 4) 2^-24 and its cap of 1 % near-tie
positions.  (On the CPU fp32 brute force leaves out 0.01 % of the positions on the sphere, 0.012 % on the clusters, 0.1 % on the cross
query and none in 1-D and 2-D.)"""
import torch

import knn_cases

# (N, M, D, k, flags): the brute kernel's table where D <= 3, and the shapes the grid adds
CASES = [
    (1, 1, 3, 1, ""),               # smallest possible input: one cell, zero extent
    (50, 9, 3, 9, ""),              # k = M: every list holds every target
    (33, 33, 3, 32, "omit"),        # k = M - 1: every list fills only once the whole grid has been seen
    (200, 333, 3, 30, ""),          # sources and targets differ: two key sorts
    (257, 257, 3, 32, "omit"),      # k at the limit; a second workgroup of one query
    (150, 200, 1, 5, ""),           # D = 1
    (300, 300, 2, 10, "omit"),      # D = 2
    (0, 40, 3, 5, ""),              # N = 0: nothing is launched
]
GRIDS = (1, 2, 0, 64)               # forced cells per axis: one cell, two, the library's choice, mostly empty cells


def _both(dev, src, tgt, k, omit=False, cells=0, budget=None, info=False):
    """(ops.knn_grid result, ops.knn result) on ``dev``, host copies."""
    from diffusion_net import ops
    s, t = src.to(dev), tgt.to(dev)
    if src is tgt:
        t = s
    got = ops.knn_grid(s, t, k, omit_diagonal=omit, cells_per_axis=cells, return_info=info, cell_budget=budget)
    want = ops.knn(s, t, k, omit_diagonal=omit)
    return tuple(g.cpu() if isinstance(g, torch.Tensor) else g for g in got), (want[0].cpu(), want[1].cpu())


def assert_same_bits(got, want, what=""):
    assert torch.equal(got[1], want[1]), "indices differ from ops.knn %s" % (what,)
    assert torch.equal(got[0], want[0]), "distances differ from ops.knn %s" % (what,)


def run_case(dev, N, M, D, k, flags, seed=0):
    """One row of the case table: every forced grid and budget 0 give ops.knn's bits, and those pass the fp64 checker."""
    omit = flags == "omit"
    src, tgt = knn_cases.inputs(N, M, D, omit, 300 + seed)
    if omit:
        tgt = src                                    # the self-query form the pipeline uses (one sort)
    want = None
    for cells, budget in [(g, None) for g in GRIDS] + [(0, 0)]:
        got, want = _both(dev, src, tgt, k, omit, cells, budget)
        assert_same_bits(got, want, (cells, budget))
    knn_cases.check_knn(src, tgt, k, False, omit, want)
    if omit and N:                                   # the same points as two tensors: the sources get a sort of their own
        got, _ = _both(dev, src, src.clone(), k, omit)
        assert_same_bits(got, want, "separate tensors")


def run_exact_ties(dev):
    g = torch.Generator().manual_seed(5)
    pts = torch.randint(0, 4, (150, 3), generator=g).float()          # integer lattice: the lower-index rule is all that orders ties
    for omit in (False, True):
        d2, want_idx = knn_cases.lattice_expected(pts, 8, False, omit)
        for cells in GRIDS:
            got, want = _both(dev, pts, pts, 8, omit, cells)
            assert torch.equal(got[1], want_idx), (omit, cells)
            assert_same_bits(got, want, (omit, cells))
        exact = d2.double().sqrt()
        assert bool(((want[0].double() - exact).abs() <= knn_cases.rel_bound(3) * exact).all())
    g = torch.Generator().manual_seed(8)
    pts = torch.randint(0, 9, (400, 3), generator=g).float() / 8      # {0, 1/8, .., 1}^3: points on cell planes (8 cells per axis: all of them)
    for cells in (0, 4, 8):
        got, want = _both(dev, pts, pts, 12, False, cells)
        assert_same_bits(got, want, cells)
    d2, want_idx = knn_cases.lattice_expected(pts * 8, 12, False, False)
    assert torch.equal(want[1], want_idx)


def run_duplicates(dev):
    g = torch.Generator().manual_seed(6)
    half = torch.randn(90, 3, generator=g)
    pts = torch.cat([half, half])                                     # every point twice: the neighbour is the twin at distance 0
    for cells in GRIDS:
        got, want = _both(dev, pts, pts, 1, True, cells)
        assert_same_bits(got, want, cells)
        assert torch.equal(got[1][:, 0], (torch.arange(180) + 90) % 180) and bool((got[0] == 0).all())
    same = half[:1].repeat(90, 1)                                     # 90 identical points: zero extent
    for omit, k in ((False, 7), (True, 7), (True, 32)):
        got, want = _both(dev, same, same, k, omit)
        assert_same_bits(got, want, (omit, k))
        assert bool((got[0] == 0).all())
    t = torch.randn(120, 1, generator=g)
    line = torch.cat([t * 2.0 + 1.0, t * -3.0, t * 0.5 - 2.0], dim=1)  # collinear points: one occupied diagonal of the grid
    for cells in GRIDS:
        got, want = _both(dev, line, line, 9, True, cells)
        assert_same_bits(got, want, cells)
    knn_cases.check_knn(line, line, 9, False, True, want)


def run_clusters(dev):
    """Two tight clusters 10 apart and one far outlier: the box is almost empty, and still every query closes without a scan."""
    g = torch.Generator().manual_seed(9)
    a = torch.randn(600, 3, generator=g) * 0.01
    b = torch.randn(600, 3, generator=g) * 0.01 + torch.tensor([10.0, 0.0, 0.0])
    pts = torch.cat([a, b, torch.tensor([[-50.0, 3.0, 7.0]])])
    got, want = _both(dev, pts, pts, 30, True, info=True)
    assert_same_bits(got, want)
    print("knn_grid clusters:", got[2])
    assert got[2]["full_scans"] == 0 and got[2]["max_shell"] >= 1
    knn_cases.check_knn(pts, pts, 30, False, True, want)


def run_cross(dev):
    """Sources spread far beyond the targets' box: their clamped cells cannot close, and the budget turns them into scans."""
    g = torch.Generator().manual_seed(10)
    src = torch.randn(300, 3, generator=g) * 3
    tgt = torch.rand(1200, 3, generator=g)
    got, want = _both(dev, src, tgt, 8, False, info=True)
    assert_same_bits(got, want)
    print("knn_grid cross query:", got[2])
    assert got[2]["full_scans"] > 0
    got0, _ = _both(dev, src, tgt, 8, False, budget=0, info=True)
    assert_same_bits(got0, want, "budget 0")
    assert got0[2]["full_scans"] == 300 and got0[2]["max_shell"] == 0
    knn_cases.check_knn(src, tgt, 8, False, False, want)


def run_repeat(dev):
    src, tgt = knn_cases.inputs(300, 500, 3, False, 31)
    one, _ = _both(dev, src, tgt, 16)
    two, want = _both(dev, src, tgt, 16)
    assert_same_bits(two, one, "second run")
    assert_same_bits(one, want)


def run_non_finite(dev):
    """One NaN row and one +inf row: unspecified neighbours, but the call returns and every index is a target's."""
    from diffusion_net import ops
    g = torch.Generator().manual_seed(11)
    pts = torch.randn(200, 3, generator=g)
    pts[17] = float("nan")
    pts[101] = float("inf")
    for cells, budget in ((0, None), (5, None), (0, 0)):
        p = pts.to(dev)
        dist, idx = ops.knn_grid(p, p, 6, omit_diagonal=True, cells_per_axis=cells, cell_budget=budget)
        assert tuple(idx.shape) == (200, 6) and int(idx.min()) >= 0 and int(idx.max()) < 200
    clean = pts.clone()
    clean[17] = 0.0
    clean[101] = 1.0
    tgt = clean.to(dev)                                               # finite targets, non-finite queries: the grid is a real one
    dist, idx = ops.knn_grid(pts.to(dev), tgt, 6)
    assert int(idx.min()) >= 0 and int(idx.max()) < 200


def run_pipeline(dev, monkeypatch):
    """cloud_operators and point_cloud_laplacian at 500 points: the grid route (threshold 0) returns the default route's tensors."""
    from diffusion_net import geometry
    g = torch.Generator().manual_seed(12)
    v = torch.nn.functional.normalize(torch.randn(500, 3, generator=g), dim=1).to(dev)
    assert geometry.KNN_GRID_MIN_POINTS is None or geometry.KNN_GRID_MIN_POINTS > 500
    calls = []
    real = geometry.ops.knn_grid
    monkeypatch.setattr(geometry.ops, "knn_grid", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    base_ops = geometry.cloud_operators(v)
    base_lap = geometry.point_cloud_laplacian(v)
    base_n = geometry.vertex_normals(v, torch.empty(0, 3, dtype=torch.int64))
    assert not calls
    monkeypatch.setattr(geometry, "KNN_GRID_MIN_POINTS", 0)
    grid_ops = geometry.cloud_operators(v)
    grid_lap = geometry.point_cloud_laplacian(v)
    grid_n = geometry.vertex_normals(v, torch.empty(0, 3, dtype=torch.int64))
    assert len(calls) == 3
    assert torch.equal(grid_n, base_n)
    for a, b in zip(base_ops + base_lap, grid_ops + grid_lap):
        if a.is_sparse:
            assert torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())
        else:
            assert torch.equal(a, b)


def run_abi_errors():
    """Every non-zero return of the two calls, through ctypes, on host buffers: nothing is launched, the outputs keep their fill."""
    from diffusion_net import _hip
    L = _hip.lib()
    src, tgt = knn_cases.inputs(70, 70, 3, False, 1)
    other = torch.randn(50, 3)
    dist = torch.full((70, 40), -7.0)
    idx = torch.full((70, 40), -7, dtype=torch.int64)
    key = torch.full((70,), -7, dtype=torch.int32)
    skey_buf = torch.full((70,), -7, dtype=torch.int32)
    box = torch.cat((tgt.amin(0), tgt.amax(0)))
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    order = torch.arange(70)
    start = torch.zeros(4 ** 3 + 1, dtype=torch.int32)

    def keys(s, t, dim, k, cells=0, box_=box, tkey=key):
        return L.dn_knn_grid_keys_f32(s.data_ptr(), s.shape[0], t.data_ptr(), t.shape[0], dim, k, cells, _hip.ptr(box_), skey_buf.data_ptr(),
                                      _hip.ptr(tkey), None)

    def search(s, t, dim, k, omit=0, cells=0, ws_bytes=ws.numel(), n_src=None, dist_=dist, start_=start):
        return L.dn_knn_grid_search_f32(s.data_ptr(), s.shape[0] if n_src is None else n_src, t.data_ptr(), t.shape[0], dim, k, omit, cells,
                                        -1, box.data_ptr(), order.data_ptr(), order.data_ptr(), _hip.ptr(start_), _hip.ptr(dist_),
                                        idx.data_ptr(), None, ws.data_ptr(), ws_bytes, None)

    assert L.dn_knn_grid_cell_budget() > 0
    assert L.dn_knn_grid_cells(1200, 8, 3, 0) == 9 and L.dn_knn_grid_cells(1200, 8, 3, 5) == 5       # ceil(cbrt(4 M / k)); a forced value
    assert L.dn_knn_grid_cells(10 ** 6, 30, 3, 0) == 52 and L.dn_knn_grid_cells(10, 30, 3, 100000) == 256   # ... clamped
    assert L.dn_knn_grid_cells(300, 10, 2, 0) == 8 and L.dn_knn_grid_cells(200, 5, 1, 0) == 40
    assert L.dn_knn_grid_cells(100, 5, 4, 0) == 0
    for call in (keys, search):
        assert call(src, tgt, 0, 1) != 0                  # dim < 1
        assert call(src, tgt, 4, 1) != 0                  # dim > 3
        assert call(src, tgt, 3, 0) != 0                  # k < 1
        assert call(src, tgt, 3, 33) != 0                 # k > dn_knn_max_k()
        assert call(src, tgt, 3, 5, cells=-1) != 0        # negative cells_per_axis
    assert keys(src, tgt, 3, 5, box_=None) != 0 and keys(src, tgt, 3, 5, tkey=None) != 0              # NULL required pointers
    assert search(src, other[:31], 3, 32) != 0            # k > n_tgt
    assert search(src[:20], tgt[:20], 3, 20, omit=1) != 0   # k > n_tgt - 1 with the diagonal left out
    assert search(src, other, 3, 1, omit=1) != 0          # omit_diagonal with n_src != n_tgt
    assert search(src, tgt, 3, 5, n_src=-1) != 0          # a negative size
    assert search(src, tgt, 3, 5, dist_=None) != 0 and search(src, tgt, 3, 5, start_=None) != 0
    need = L.dn_knn_grid_workspace_bytes(70, 70, 3, 5, 0)
    assert need >= 70 * 16 and L.dn_knn_grid_workspace_bytes(70, 70, 4, 5, 0) == 0
    assert search(src, tgt, 3, 5, ws_bytes=need - 1) != 0   # workspace smaller than the query says
    assert bool((dist == -7.0).all()) and bool((idx == -7).all()) and bool((key == -7).all()) and bool((skey_buf == -7).all())
    assert search(src, tgt, 3, 5, n_src=0) == 0           # n_src == 0: success, nothing launched
    assert bool((dist == -7.0).all()) and bool((idx == -7).all())
    # and the calls as ops.knn_grid chains them, with the exact workspace size
    G = L.dn_knn_grid_cells(70, 5, 3, 0)
    assert keys(src, tgt, 3, 5) == 0
    skey, perm = torch.sort(key, stable=True)
    cs = torch.searchsorted(skey, torch.arange(G ** 3 + 1, dtype=torch.int32), out_int32=True)
    assert L.dn_knn_grid_search_f32(src.data_ptr(), 70, tgt.data_ptr(), 70, 3, 5, 0, 0, -1, box.data_ptr(), order.data_ptr(), perm.data_ptr(),
                                    cs.data_ptr(), dist.data_ptr(), idx.data_ptr(), None, ws.data_ptr(), need, None) == 0
    knn_cases.check_knn(src, tgt, 5, False, False, (dist.flatten()[:350].reshape(70, 5).clone(), idx.flatten()[:350].reshape(70, 5).clone()))

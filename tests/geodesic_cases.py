"""Shared bodies of the geodesic tests (test_geodesic_emu.py: emulator build on host buffers; test_geodesic_gpu.py: the device; the
fixtures also serve test_geodesic_host.py).  The oracle is ``scipy.sparse.csgraph.dijkstra`` in fp64 on the SAME CSR arrays: the fixed point
of the (min, +) sweeps is the minimum over paths of the left-to-right fp64 sum of the arc lengths, which is what Dijkstra returns, so the
comparison is ``np.array_equal``."""
import functools

import numpy as np
import scipy.sparse
import scipy.sparse.csgraph
import torch


# ---------------------------------------------------------------------------------------------- meshes
@functools.lru_cache(maxsize=None)
def icosphere(n_sub):
    """Unit icosahedron, every face split in four ``n_sub`` times, vertices pushed to the sphere: 10 * 4^n + 2 vertices."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(q, dtype=np.float64) / np.linalg.norm(q) for q in v]
    for _ in range(n_sub):
        mid, nf = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = v[a] + v[b]
                v.append(q / np.linalg.norm(q))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts, faces = np.array(v), np.array(f, dtype=np.int64)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


@functools.lru_cache(maxsize=None)
def planar_delaunay(n=64, seed=5):
    """Delaunay triangulation of ``n`` seeded points of the unit square (z = 0): irregular degrees, slivers along the hull."""
    from scipy.spatial import Delaunay
    xy = np.random.RandomState(seed).rand(n, 2)
    verts = np.concatenate([xy, np.zeros((n, 1))], axis=1)
    faces = Delaunay(xy).simplices.astype(np.int64)
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


def loop_graph(verts, faces, m):
    """The definition of ``geometry.mesh_distance_graph`` in plain loops: ({(position bytes, position bytes): length}, positions).  Nodes
    are identified by position, so the numbering of the Steiner nodes is free."""
    x = np.asarray(verts, dtype=np.float64)
    arcs = {}

    def node(a, b, j):          # j-th node of the edge (a, b): 0 and m + 1 are its vertices
        a, b = (a, b) if a < b else (b, a)
        if j == 0:
            return ("v", a)
        if j == m + 1:
            return ("v", b)
        return ("s", a, b, j)

    def position(nd):
        if nd[0] == "v":
            return x[nd[1]]
        _, a, b, j = nd
        t = j / (m + 1)
        return (1.0 - t) * x[a] + t * x[b]

    def arc(p, q):
        if p != q:
            arcs[frozenset((p, q))] = float(np.sqrt(((position(p) - position(q)) ** 2).sum()))

    for face in np.asarray(faces):
        e = [(int(face[i]), int(face[(i + 1) % 3]), int(face[(i + 2) % 3])) for i in range(3)]
        for a, b, c in e:
            lo, hi = min(a, b), max(a, b)
            for j in range(m + 1):
                arc(node(lo, hi, j), node(lo, hi, j + 1))                     # (i)
            for j in range(1, m + 1):
                arc(node(a, b, j), ("v", c))                                   # (iii)
        for p in range(3):
            for q in range(p + 1, 3):
                for j in range(1, m + 1):
                    for k in range(1, m + 1):
                        arc(node(e[p][0], e[p][1], j), node(e[q][0], e[q][1], k))   # (ii)
    return arcs, position


def loop_graph_csr(verts, faces, m):
    """``loop_graph`` as a scipy CSR matrix with the vertices first (its own Steiner numbering)."""
    arcs, _ = loop_graph(verts, faces, m)
    V = np.asarray(verts).shape[0]
    ids = {("v", i): i for i in range(V)}
    for pair in arcs:
        for nd in sorted(pair):
            if nd not in ids:
                ids[nd] = len(ids)
    i, j, w = [], [], []
    for pair, length in arcs.items():
        p, q = tuple(pair)
        i += [ids[p], ids[q]]
        j += [ids[q], ids[p]]
        w += [length, length]
    n = len(ids)
    return scipy.sparse.coo_matrix((np.array(w, dtype=np.float64), (np.array(i, dtype=np.int64), np.array(j, dtype=np.int64))), shape=(n, n)).tocsr()


# ---------------------------------------------------------------------------------------------- graphs of the op-level cases
def _csr(n, tails, tips, w):
    """Symmetric CSR graph from undirected arcs (explicit zeros are kept: they are arcs of length 0)."""
    tails, tips, w = np.asarray(tails, dtype=np.int64), np.asarray(tips, dtype=np.int64), np.asarray(w, dtype=np.float64)
    g = scipy.sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([tails, tips]), np.concatenate([tips, tails]))), shape=(n, n)).tocsr()
    g.sort_indices()
    return g


@functools.lru_cache(maxsize=None)
def graph(name):
    from diffusion_net import geometry
    rng = np.random.RandomState(11)
    if name == "icosphere":                 # (a) 402 nodes, 6 720 directed arcs
        g = geometry.mesh_distance_graph(*icosphere(1), n_steiner=3)
        assert g.shape[0] == 402 and g.nnz == 6720
    elif name == "planar":                  # (b) irregular degrees
        g = geometry.mesh_distance_graph(*planar_delaunay(), n_steiner=3)
    elif name == "path":                    # (c) 299 sweeps from one end
        g = _csr(300, np.arange(299), np.arange(1, 300), rng.rand(299) + 0.1)
    elif name == "components":              # (d) rows 0 and 11 empty, 5 isolated, {1..4} and {6..10} connected
        tails = [1, 2, 3, 1, 6, 7, 8, 9, 6]
        tips = [2, 3, 4, 4, 7, 8, 9, 10, 10]
        g = _csr(12, tails, tips, rng.rand(len(tails)) + 0.1)
    elif name == "zero_arcs":               # (e) duplicate nodes joined by arcs of length 0
        tails = [0, 1, 2, 3, 4, 5, 0, 2]
        tips = [1, 2, 3, 4, 5, 6, 3, 6]
        g = _csr(7, tails, tips, [0.0, 0.5, 0.0, 0.25, 0.0, 0.0, 0.75, 1.5])
    elif name == "star":                    # (f) a hub of 500 arcs among rows of 2 (the rim is a ring)
        rim = np.arange(1, 501)
        g = _csr(501, np.concatenate([np.zeros(500, dtype=np.int64), rim]), np.concatenate([rim, np.roll(rim, -1)]),
                 np.concatenate([rng.rand(500) + 1.0, rng.rand(500) * 3.0 + 0.1]))
        assert np.diff(g.indptr).max() == 500
    else:
        raise KeyError(name)
    return g


def small_graph(n, seed=3):
    """(g) a ring of n nodes with a chord (n = 1: no arcs; n = 2: one arc)."""
    rng = np.random.RandomState(seed + n)
    if n == 1:
        return scipy.sparse.csr_matrix((1, 1), dtype=np.float64)
    if n == 2:
        return _csr(2, [0], [1], [0.625])
    a = np.arange(n)
    tails, tips = np.concatenate([a, [0]]), np.concatenate([np.roll(a, -1), [n // 2]])
    return _csr(n, tails, tips, rng.rand(n + 1) + 0.1)


def source_list(g, length, seed=7):
    """``length`` seeded source nodes of ``g`` from its whole node range (so Steiner nodes too); from 3 on, the last repeats the first."""
    src = np.random.RandomState(seed + length).randint(0, g.shape[0], size=length).astype(np.int64)
    if length >= 3:
        src[-1] = src[0]
    return src


# ---------------------------------------------------------------------------------------------- bodies
@functools.lru_cache(maxsize=None)
def _oracle_all(name):
    d = scipy.sparse.csgraph.dijkstra(graph(name), directed=True)
    d.setflags(write=False)
    return d


def oracle(g, src, name=None):
    if name is not None:
        return _oracle_all(name)[src]
    if g.shape[0] == 1:
        return np.zeros((len(src), 1))
    return scipy.sparse.csgraph.dijkstra(g, directed=True, indices=src)


def device_csr(g, dev):
    return (torch.from_numpy(g.indptr.astype(np.int32)).to(dev), torch.from_numpy(g.indices.astype(np.int32)).to(dev),
            torch.from_numpy(g.data.astype(np.float64)).to(dev))


def minplus(g, src, dev, **kw):
    from diffusion_net import ops
    out = ops.minplus_distances(*device_csr(g, dev), torch.from_numpy(np.asarray(src, dtype=np.int64)), **kw)
    assert out.dtype == torch.float64 and out.device.type == torch.device(dev).type and tuple(out.shape) == (len(src), g.shape[0])
    return out.cpu().numpy()


def run_graph(dev, name, n_src, **kw):
    g = graph(name)
    src = source_list(g, n_src)
    got = minplus(g, src, dev, **kw)
    want = oracle(g, src, name)
    assert np.array_equal(got, want), "worst difference %g" % np.nanmax(np.abs(np.where(got == want, 0.0, got - want)))
    return got


def run_path(dev, sweeps_per_check):
    """Sources at both ends and inside: from node 299 the lengths travel one node per sweep against the node order."""
    g = graph("path")
    src = np.array([299, 0, 150, 299], dtype=np.int64)
    assert np.array_equal(minplus(g, src, dev, sweeps_per_check=sweeps_per_check), oracle(g, src, "path"))


def run_components(dev):
    g = graph("components")
    src = np.arange(12, dtype=np.int64)
    got, want = minplus(g, src, dev), oracle(g, src, "components")
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.isinf(got).sum() == 144 - (3 + 16 + 25)
    assert np.array_equal(got, want)


def run_small(dev, n):
    g = small_graph(n)
    src = np.array([n - 1, 0, n // 2], dtype=np.int64)
    assert np.array_equal(minplus(g, src, dev), oracle(g, src))


def run_blocks(dev, name):
    """At least three source blocks of a size that is no multiple of 64, and a second run: the same bits."""
    g = graph(name)
    src = source_list(g, 130)
    per_block = 50
    one = minplus(g, src, dev)
    cut = minplus(g, src, dev, max_block_bytes=per_block * 8 * g.shape[0] + 8)
    again = minplus(g, src, dev)
    assert np.array_equal(one, oracle(g, src, name)) and np.array_equal(cut, one) and np.array_equal(again, one)


def run_errors(dev):
    from diffusion_net import ops
    import pytest
    g = graph("zero_arcs")
    rowptr, col, w = device_csr(g, dev)
    src = torch.tensor([0, 3])
    bad_w = w.clone()
    bad_w[2] = -1.0
    with pytest.raises(ValueError):
        ops.minplus_distances(rowptr, col, bad_w, src)
    bad_w[2] = float("nan")
    with pytest.raises(ValueError):
        ops.minplus_distances(rowptr, col, bad_w, src)
    for c in (7, -1):
        bad_col = col.clone()
        bad_col[1] = c
        with pytest.raises(ValueError):
            ops.minplus_distances(rowptr, bad_col, w, src)
    for s in (7, -1):
        with pytest.raises(ValueError):
            ops.minplus_distances(rowptr, col, w, torch.tensor([0, s]))
    assert tuple(ops.minplus_distances(rowptr, col, w, torch.zeros(0, dtype=torch.int64)).shape) == (0, 7)

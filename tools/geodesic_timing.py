"""Measures the all-pairs mesh distances of ``geometry.get_all_pairs_geodesic_distance`` (Steiner-point graph, dn_geodesic.hip).

  accuracy  (CPU route; the device route returns the same bits)  mean and worst relative excess of the graph distance over the true
            distance for n_steiner = 0, 1, 2, 3, 5 on a planar Delaunay mesh (truth: Euclidean) and on an icosphere (truth: great-circle
            arc; the polyhedral geodesic itself is BELOW the arc by O(h^2), so small negative entries there are the mesh, not the graph).
            -> $DN_OUT_DIR/geodesic_accuracy.txt
  timing    (needs a ROCm device)  at a FAUST-sized closed mesh -- the package's synthetic generator ``synthetic.sphere_mesh`` at 6 890
            vertices -- for n_steiner = 0, 1, 3: nodes, arcs, sweeps to the fixed point, the time of the device route (all sources, host
            clock, transfers included), the time of one sweep of a full source block (device events around windows of back-to-back
            sweeps on a converged block, warm-up first, median [min .. max]) and the bytes a sweep reads / that time.  The comparison is the
            host route of this package, scipy's Dijkstra on the same graph: timed on 64 sources and SCALED to all of them, in one process
            (what the host route does) and spread over 16 processes.  The reference's route (igl.exact_geodesic per source in a process
            pool; its own word: "SLOW") needs libigl and is not measured: no figure is claimed for it.
            -> $DN_OUT_DIR/geodesic_timing.txt

python tools/geodesic_timing.py [accuracy] [timing]   (default: both; bash tools/gpu_run.sh geodesic)"""
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import scipy.sparse.csgraph  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
V_FAUST = 6890
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush_to(name):
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, name), "w").write("\n".join(lines) + "\n")
    del lines[:]


# ---------------------------------------------------------------------------------------------- accuracy
def planar_mesh(n=404, seed=1):
    from scipy.spatial import Delaunay
    xy = np.random.RandomState(seed).rand(n, 2)
    return np.concatenate([xy, np.zeros((n, 1))], axis=1), Delaunay(xy).simplices.astype(np.int64)


def icosphere(n_sub):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(q, dtype=np.float64) for q in ((-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                                                 (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1))]
    v = [q / np.linalg.norm(q) for q in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(n_sub):
        mid, nf = {}, []
        for a, b, c in f:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                k = (min(i, j), max(i, j))
                if k not in mid:
                    q = v[i] + v[j]
                    v.append(q / np.linalg.norm(q))
                    mid[k] = len(v) - 1
                m.append(mid[k])
            nf += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        f = nf
    return np.array(v), np.array(f, dtype=np.int64)


def accuracy():
    from diffusion_net import geometry
    say("relative excess of the Steiner-graph distance over the true distance, all pairs of distinct vertices, fp64, CPU route")
    say("(scipy Dijkstra on geometry.mesh_distance_graph; the device route returns the same bits)")
    pv, pf = planar_mesh()
    sv, sf = icosphere(3)
    truth_p = np.sqrt(((pv[:, None] - pv[None]) ** 2).sum(-1))
    truth_s = np.arccos(np.clip(sv @ sv.T, -1.0, 1.0))
    for title, v, f, truth in (("planar Delaunay mesh, %d vertices, %d faces (truth: Euclidean distance)" % (len(pv), len(pf)), pv, pf, truth_p),
                               ("icosphere, %d vertices, %d faces (truth: great-circle arc of the unit sphere; the polyhedral geodesic is "
                                "below it by O(h^2))" % (len(sv), len(sf)), sv, sf, truth_s)):
        say("--- " + title)
        say("  n_steiner    nodes      arcs   mean excess  worst excess  least excess")
        off = ~np.eye(len(v), dtype=bool)
        for m in (0, 1, 2, 3, 5):
            g = geometry.mesh_distance_graph(v, f, m)
            d = scipy.sparse.csgraph.dijkstra(g, directed=True, indices=np.arange(len(v)))[:, :len(v)]
            rel = (d[off] - truth[off]) / truth[off]
            say("  %9d %8d %9d   %10.3f %%  %10.3f %%  %10.3f %%" % (m, g.shape[0], g.nnz // 2, 100 * rel.mean(), 100 * rel.max(), 100 * rel.min()))
    flush_to("geodesic_accuracy.txt")


# ---------------------------------------------------------------------------------------------- timing
_G = None


def _host_rows(src):
    return scipy.sparse.csgraph.dijkstra(_G, directed=True, indices=src).shape[0]


def host_times(g, n_src=64):
    """(seconds for n_src sources in one process, seconds for them spread over 16 processes); workers are forked before the device is opened."""
    global _G
    _G = g
    src = np.random.RandomState(2).choice(V_FAUST, size=n_src, replace=False)
    t0 = time.perf_counter()
    _host_rows(src)
    one = time.perf_counter() - t0
    with multiprocessing.get_context("fork").Pool(16) as pool:
        pool.map(_host_rows, np.array_split(src[:16], 16))              # warm-up: every worker has run once
        t0 = time.perf_counter()
        pool.map(_host_rows, np.array_split(src, 16))
        many = time.perf_counter() - t0
    return one, many


def timing():
    from diffusion_net import geometry, synthetic
    verts, faces = synthetic.sphere_mesh(V_FAUST)
    graphs = {m: geometry.mesh_distance_graph(verts, faces, m) for m in (0, 1, 3)}
    host = {m: host_times(g) for m, g in graphs.items()}                 # before the device is opened: the pool forks
    import torch
    from diffusion_net import _hip, ops
    assert torch.cuda.is_available(), "the timing section measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, torch.__version__))
    say("mesh: synthetic.sphere_mesh(%d) (Fibonacci lattice, convex hull, radial bumps): %d vertices, %d faces -- the FAUST size" % (
        V_FAUST, len(verts), len(faces)))
    say("device route: geometry.geodesic_distances, all %d sources, host clock (graph build, transfers and the host's reads of the changed word" % V_FAUST)
    say("included), 3 runs after one warm-up run.  One sweep: device events around windows of 8 back-to-back sweeps of one full source block at")
    say("its fixed point (every arc read, nothing written), 2 warm-up windows, median [min .. max] of 7.  Bytes of a sweep: 8 (arcs + nodes)")
    say("per source + 12 per arc, as the lanes request them (a row is requested once per arc that names it; what the caches absorb of that is")
    say("the difference between the two node orders).  Host route: scipy Dijkstra on the same graph, timed on 64 sources and SCALED by %d / 64." % V_FAUST)
    say("The reference's route (igl.exact_geodesic per source; its own word: SLOW) needs libigl: not measured, no figure claimed.")
    L = _hip.lib()
    for m, g in graphs.items():
        n, arcs = g.shape[0], g.nnz
        say("--- n_steiner = %d: %d nodes, %d directed arcs, longest row %d" % (m, n, arcs, int(np.diff(g.indptr).max())))
        S = min(V_FAUST, (1 << 30) // (8 * n))
        say("source block: %d sources (%.2f GB)" % (S, 8e-9 * n * S))
        gd, new_of = geometry._band_ordered(g)
        for order, gg, first in (("nodes as the graph numbers them (vertices, then edge by edge)", g, np.arange(S)),
                                 ("nodes in reverse Cuthill-McKee order (what the device route uploads)", gd, new_of[:S])):
            rowptr = torch.from_numpy(gg.indptr.astype(np.int32)).to(dev)
            col = torch.from_numpy(gg.indices.astype(np.int32)).to(dev)
            w = torch.from_numpy(gg.data.astype(np.float64)).to(dev)
            reach = int(np.abs(gg.tocoo().row - gg.tocoo().col).max())
            # sweeps to the fixed point of the first source block, counted one sweep per call
            dist = torch.full((n, S), float("inf"), dtype=torch.float64, device=dev)
            dist[torch.from_numpy(first).to(dev), torch.arange(S, device=dev)] = 0.0
            changed = torch.zeros(1, dtype=torch.int32, device=dev)
            args = (rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), n, dist.data_ptr(), S)
            sweeps = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while True:
                _hip.check(L.dn_minplus_sweeps_f64(*args, 1, changed.data_ptr(), None), "dn_minplus_sweeps_f64")
                sweeps += 1
                if not int(changed.item()):
                    break
            t_conv = time.perf_counter() - t0
            ts = []
            for i in range(9):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _hip.check(L.dn_minplus_sweeps_f64(*args, 8, changed.data_ptr(), None), "dn_minplus_sweeps_f64")
                b.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(a.elapsed_time(b) / 8)
            gb = (8.0 * (arcs + n) * S + 12.0 * arcs) / 1e9
            t = statistics.median(ts)
            say("%s: farthest neighbour %d numbers away" % (order, reach))
            say("  sweeps to the fixed point, the certifying one included: %d (%.3f s, one host read per sweep)" % (sweeps, t_conv))
            say("  one sweep at the fixed point: %8.3f ms [%.3f .. %.3f]; %.2f GB read -> %.2f TB/s" % (t, min(ts), max(ts), gb, gb / t))
            del dist
        tr = []
        for i in range(4):
            t0 = time.perf_counter()
            d = geometry.geodesic_distances(verts, faces, None, n_steiner=m)
            if i:
                tr.append(time.perf_counter() - t0)
        say("device route, all %d sources: %8.2f s [%.2f .. %.2f]" % (V_FAUST, statistics.median(tr), min(tr), max(tr)))
        one, many = host[m]
        say("host route, 64 sources: %.2f s in one process, %.2f s over 16 processes; SCALED to %d sources: %.0f s and %.0f s" % (
            one, many, V_FAUST, one * V_FAUST / 64, many * V_FAUST / 64))
        check = np.random.RandomState(4).choice(V_FAUST, size=4, replace=False)
        same = np.array_equal(d[check], scipy.sparse.csgraph.dijkstra(g, directed=True, indices=check)[:, :V_FAUST])
        say("rows of 4 sources against scipy: %s" % ("same bits" if same else "DIFFERENT"))
        del d
    flush_to("geodesic_timing.txt")


if __name__ == "__main__":
    want = sys.argv[1:] or ["accuracy", "timing"]
    if "accuracy" in want:
        accuracy()
    if "timing" in want:
        timing()

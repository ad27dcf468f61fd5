"""Times the cell-grid neighbour query ``ops.knn_grid`` (dn_knn_grid.hip) against the brute-force query ``ops.knn`` (dn_knn.hip, unchanged)
on the same device, in the same process, in alternating windows: k = 30, ``omit_diagonal``, the self-query of the point-cloud pipeline.
Inputs: the vertices of ``synthetic.sphere_mesh`` (a surface with 10 % radial noise) and uniform points in the unit cube (a volume-filling
cloud), at 2 000, 10 000, 50 000, 200 000 and 1 000 000 points.  Every timed result is
checked against the other route first (``torch.equal`` of distances and indices); at 1 000 000 points brute force runs once, for that check
and for one timing.  Device events around windows of back-to-back calls, warm-up first, median [min .. max] of the windows; "spread" is
max - min of a route's own windows.  Per size also: the shares of the grid route's steps (bounds + keys, sorts + cell table (torch),
gather + search), the ``return_info`` counters, and at 200 000 points ``geometry.point_cloud_laplacian`` end to end on both routes.
The last lines apply the rule that sets ``geometry.KNN_GRID_MIN_POINTS``.  Writes $DN_OUT_DIR/knn_grid_timing.txt
(bash tools/gpu_run.sh knn_grid)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffusion_net import _hip, geometry, ops, synthetic  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
K = 30
SIZES = [int(s) for s in os.environ.get("DN_KNN_GRID_SIZES", "2000,10000,50000,200000,1000000").split(",")]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fns, inner, reps, warm=2):
    """Windows of every callable in turn, ``reps`` rounds -> [(median, min, max)] in ms per call."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(window(fn, inner))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def fmt(t):
    return "%9.3f  [%.3f .. %.3f]" % t


def grid_steps(pts):
    """The device steps of ``ops._knn_grid_launch`` for a self-query as separate callables on buffers of their own."""
    L = _hip.lib()
    n = pts.shape[0]
    dev, st = pts.device, _hip.stream_of(pts)
    G = L.dn_knn_grid_cells(n, K, 3, 0)
    dist = torch.empty(n, K, dtype=torch.float32, device=dev)
    idx = torch.empty(n, K, dtype=torch.int64, device=dev)
    tkey = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(L.dn_knn_grid_workspace_bytes(n, n, 3, K, 0), dtype=torch.uint8, device=dev)
    held = {}

    def keys():
        held["box"] = torch.cat((pts.amin(dim=0), pts.amax(dim=0)))
        _hip.check(L.dn_knn_grid_keys_f32(pts.data_ptr(), n, pts.data_ptr(), n, 3, K, 0, held["box"].data_ptr(), None, tkey.data_ptr(), st), "keys")

    def sort():
        held["skey"], held["order"] = torch.sort(tkey, stable=True)
        held["start"] = torch.searchsorted(held["skey"], torch.arange(G ** 3 + 1, dtype=torch.int32, device=dev), out_int32=True)

    def search():
        _hip.check(L.dn_knn_grid_search_f32(pts.data_ptr(), n, pts.data_ptr(), n, 3, K, 1, 0, -1, held["box"].data_ptr(), held["order"].data_ptr(),
                                            held["order"].data_ptr(), held["start"].data_ptr(), dist.data_ptr(), idx.data_ptr(), None,
                                            ws.data_ptr(), ws.numel(), st), "search")

    for step in (keys, sort, search):
        step()
    torch.cuda.synchronize()
    return keys, sort, search, dist, idx, G


def one(name, n, host_pts, dev, verdict):
    pts = torch.from_numpy(np.ascontiguousarray(host_pts, dtype=np.float32)).to(dev)
    big = n >= 1000000
    inner, reps = (20, 7) if n <= 10000 else ((5, 7) if n <= 50000 else ((2, 5)))
    grid = lambda: ops.knn_grid(pts, pts, K, omit_diagonal=True)          # noqa: E731
    brute = lambda: ops.knn(pts, pts, K, omit_diagonal=True)              # noqa: E731
    gd, gi, info = ops.knn_grid(pts, pts, K, omit_diagonal=True, return_info=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bd, bi = brute()
    torch.cuda.synchronize()
    t_once = (time.perf_counter() - t0) * 1e3
    same = torch.equal(gd, bd) and torch.equal(gi, bi)
    keys, sort, search, sd, si, G = grid_steps(pts)
    same = same and torch.equal(sd, bd) and torch.equal(si, bi)
    say("== %s, %d points, k = %d, omit_diagonal; %d cells per axis; grid == brute (distances and indices, all rows): %s" % (name, n, K, G, same))
    if not same:
        raise SystemExit("the two routes differ: nothing is timed")
    del bd, bi, gd, gi
    if big:
        t_g, = alternate([grid], inner, reps)
        t_b = (t_once, t_once, t_once)
        say("   ops.knn       (brute, ONE run, host clock around a synchronise) ms: %9.3f" % t_once)
    else:
        t_g, t_b = alternate([grid, brute], inner, reps)
        say("   ops.knn       (brute)  ms: %s" % fmt(t_b))
    say("   ops.knn_grid  (grid)   ms: %s     brute / grid = %.2f" % (fmt(t_g), t_b[0] / t_g[0]))
    t_k, t_s, t_q = alternate([keys, sort, search], inner, reps)
    tot = t_k[0] + t_s[0] + t_q[0]
    say("   steps of the grid route, ms (share of their sum): bounds + keys %.3f (%.0f %%), sorts + cell table %.3f (%.0f %%), "
        "gather + search %.3f (%.0f %%)" % (t_k[0], 100 * t_k[0] / tot, t_s[0], 100 * t_s[0] / tot, t_q[0], 100 * t_q[0] / tot))
    say("   counters: largest shell %d, full scans %d" % (info["max_shell"], info["full_scans"]))
    spread = max(t_g[2] - t_g[1], t_b[2] - t_b[1])
    verdict.setdefault(n, []).append(t_g[0] + 2 * spread < t_b[0])
    if n == 200000:
        def lap():
            geometry.point_cloud_laplacian(pts)
            torch.cuda.synchronize()

        res = {}
        for route, thr in (("brute", None), ("grid", 0), ("brute", None), ("grid", 0)):
            geometry.KNN_GRID_MIN_POINTS = thr
            lap()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                lap()
                ts.append((time.perf_counter() - t0) * 1e3)
            res.setdefault(route, []).extend(ts)
        geometry.KNN_GRID_MIN_POINTS = None
        for route in ("brute", "grid"):
            t = res[route]
            say("   geometry.point_cloud_laplacian end to end (host clock, with its host read), %s query, ms: %s"
                % (route, fmt((statistics.median(t), min(t), max(t)))))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("knn_grid_timing needs a ROCm device: nothing is measured on the host")
    dev = torch.device("cuda:0")
    say("# %s, torch %s; times in ms per call, median [min .. max] of alternating windows of back-to-back calls (device events)"
        % (torch.cuda.get_device_name(0), torch.__version__))
    say("# library cell budget %d; cells per axis = ceil(cbrt(4 M / k)) in 3-D" % _hip.lib().dn_knn_grid_cell_budget())
    verdict = {}
    for n in SIZES:
        one("sphere_mesh vertices", n, synthetic.sphere_mesh(n, seed=1)[0], dev, verdict)
        one("uniform cube", n, np.random.RandomState(2).rand(n, 3), dev, verdict)
    say("== rule: KNN_GRID_MIN_POINTS = the smallest size from which grid median + 2 x spread < brute median on both inputs, at that and every larger size")
    ok = None
    for n in sorted(verdict, reverse=True):
        if len(verdict[n]) == 2 and all(verdict[n]):
            ok = n
        else:
            break
    say("   per size (sphere, cube): %s" % ", ".join("%d: %s" % (n, verdict[n]) for n in sorted(verdict)))
    say("   KNN_GRID_MIN_POINTS by the rule: %s" % ok)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "knn_grid_timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

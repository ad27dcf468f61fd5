"""Times the two device steps of the point-cloud operators separately -- the neighbourhood query ``ops.knn`` (dn_knn.hip, k = 30,
omit_diagonal) and the per-point pass ``dn_cloud_operators_f32`` (dn_cloud.hip) -- at 10 000 and 200 000 points, and the host route of
``geometry.cloud_operators`` (KD-tree, batched SVD, vectorised 2 x 2 solves; what the reference does with a Python loop) at 10 000 points.
Device events around windows of back-to-back calls, warm-up first, median [min .. max] of the windows.  The per-point pass is also given as
bytes moved / time, next to the streaming rate the project records for a plain float4 copy (5.2-5.9 TB/s).  The
10 000-point result is checked against the host route in fp64 first.  Writes $DN_OUT_DIR/cloud_timing.txt (bash tools/gpu_run.sh cloud).

The local-Delaunay Laplacian (dn_cloud_lap.hip) is timed the same way on the same clouds, step by step -- star kernel, emit kernel, the
two stable sorts with the run count (torch), the two segment sums -- then ``ops.cloud_laplacian`` whole (with its host read) and
``geometry.point_cloud_laplacian`` (query, frames and Laplacian), and the numpy route at 10 000 points; the 10 000-point result is checked
against that route first.  Those lines go to $DN_OUT_DIR/cloud_laplacian_timing.txt."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffusion_net import _hip, geometry, ops, precompute  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
K = 30
lines = []
lap_lines = []


def say(s, to=None):
    print(s, flush=True)
    (lines if to is None else to).append(s)


def dev_time(fn, inner, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)


def cloud(n, seed=3):
    """The unit sphere with a little noise, rounded to fp32."""
    rs = np.random.RandomState(seed)
    p = rs.randn(n, 3)
    p = p / np.linalg.norm(p, axis=1, keepdims=True) + 0.002 * rs.randn(n, 3)
    return p.astype(np.float32)


def bytes_moved(n, k):
    """What the per-point pass reads and writes (the count dn_cloud.hip reports to the library's profiler): k indices and k gathered points,
    the point itself, its normal, frame and row pointer, and the k + 1 entries of its row in three arrays."""
    return n * (8.0 * k + 12.0 * k + 12.0 + 12.0 + 36.0 + 4.0 + 12.0 * (k + 1))


def laplacian_steps(verts, nbr, frames):
    """The device steps of ``ops._cloud_laplacian_launch`` as separate callables on buffers of their own: star, emit, sort, sum."""
    L = _hip.lib()
    n, k = nbr.shape
    slots, st, dev = n * k, _hip.stream_of(verts), verts.device
    m = 9 * slots
    partner = torch.empty(n, k, dtype=torch.int32, device=dev)
    status, count = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.dn_cloud_laplacian_workspace_bytes(n, k), dtype=torch.uint8, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col, val = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.float32, device=dev)
    mass = torch.zeros(n, dtype=torch.float32, device=dev)
    key_l, val_l = ws[:72 * slots].view(torch.int64), ws[72 * slots:144 * slots].view(torch.float64)
    key_m, val_m = ws[144 * slots:168 * slots].view(torch.int64), ws[168 * slots:192 * slots].view(torch.float64)
    held = {}

    def star():
        _hip.check(L.dn_cloud_star_f32(verts.data_ptr(), n, nbr.data_ptr(), k, frames.data_ptr(), partner.data_ptr(), status.data_ptr(), st), "star")

    def emit():
        _hip.check(L.dn_cloud_laplacian_emit_f32(verts.data_ptr(), n, nbr.data_ptr(), k, partner.data_ptr(), ws.data_ptr(), ws.numel(), st), "emit")

    def sort():
        skey, perm = torch.sort(key_l, stable=True)
        head = torch.ones(m, dtype=torch.bool, device=dev)
        torch.ne(skey[1:], skey[:-1], out=head[1:])
        held.update(skey=skey, perm=perm, rank=torch.cumsum(head, 0, dtype=torch.int64))
        held["skey_m"], held["perm_m"] = torch.sort(key_m, stable=True)

    def sums():
        _hip.check(L.dn_segment_sum_f64_f32(held["skey"].data_ptr(), held["perm"].data_ptr(), val_l.data_ptr(), m, held["rank"].data_ptr(), n,
                                            rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), count.data_ptr(), st), "sum")
        _hip.check(L.dn_segment_sum_f64_f32(held["skey_m"].data_ptr(), held["perm_m"].data_ptr(), val_m.data_ptr(), 3 * slots, None, n, None,
                                            None, mass.data_ptr(), None, st), "sum")

    for step in (star, emit, sort, sums):
        step()
    torch.cuda.synchronize()
    return star, emit, sort, sums, partner, count


def time_laplacian(n, pts, verts, nbr, t_knn):
    lap = lambda s: say(s, lap_lines)
    lap("--- %d points, k = %d" % (n, K))
    frames = ops.cloud_operators(verts, nbr)[1]
    if n == 10000:
        partner, rowptr, col, val, mass = ops.cloud_laplacian(verts, nbr, frames)
        Lh, mh, parts = precompute.point_cloud_laplacian_from_table(pts, nbr.cpu().numpy(), frames.cpu().numpy(), with_parts=True)
        same = np.array_equal(rowptr.cpu().numpy(), Lh.indptr) and np.array_equal(col.cpu().numpy(), Lh.indices)
        share = float((np.abs(val.cpu().numpy().astype(np.float64) - Lh.data) / (2.0 ** -23 * parts["L_abs"].data)).max()) if same else float("nan")
        lap("kernels against the numpy route in fp64 on the same table and frames: partner tables equal: %s, pattern equal: %s, "
            "largest |val - ref| = %.3f of 2^-23 x the entry's absolute terms; %d triangles, %d entries, mass sum %.5f (4 pi = %.5f)" % (
                np.array_equal(partner.cpu().numpy(), parts["partner"]), same, share, int((partner >= 0).sum()), col.numel(), float(mass.sum()),
                4 * np.pi))
    big = n > 50000
    star, emit, sort, sums, partner, count = laplacian_steps(verts, nbr, frames)
    lap("(%d of %d slots hold a triangle; %d matrix entries from %d sorted keys)" % (int((partner >= 0).sum()), partner.numel(), int(count.item()),
                                                                                     9 * partner.numel()))
    inner, reps = (5, 7) if big else (20, 15)
    lap("ops.knn (neighbourhood query, for scale):             %9.3f  [%.3f .. %.3f]" % t_knn)
    lap("dn_cloud_star_f32 (projection, Delaunay stars):       %9.3f  [%.3f .. %.3f]" % dev_time(star, inner, reps))
    lap("dn_cloud_laplacian_emit_f32 (12 keyed terms a slot):  %9.3f  [%.3f .. %.3f]" % dev_time(emit, inner, reps))
    lap("torch.sort (stable) of both key arrays + run count:   %9.3f  [%.3f .. %.3f]" % dev_time(sort, 2 if big else 10, 5 if big else 9, warm=1))
    lap("dn_segment_sum_f64_f32 (matrix and mass):             %9.3f  [%.3f .. %.3f]" % dev_time(sums, inner, reps))
    lap("ops.cloud_laplacian (all of the above + host read):   %9.3f  [%.3f .. %.3f]" % dev_time(
        lambda: ops.cloud_laplacian(verts, nbr, frames), 2 if big else 5, 5 if big else 9, warm=1))
    lap("geometry.point_cloud_laplacian (query, frames, L):    %9.3f  [%.3f .. %.3f]" % dev_time(
        lambda: geometry.point_cloud_laplacian(verts, K), 1 if big else 5, 3 if big else 9, warm=1))
    if n == 10000:
        tb = []
        for _ in range(3):
            t0 = time.perf_counter()
            precompute.point_cloud_laplacian_host(pts.astype(np.float64), K)
            tb.append(1e3 * (time.perf_counter() - t0))
        lap("precompute.point_cloud_laplacian_host (numpy, fp64):  %9.1f  [%.1f .. %.1f]  (host clock, 3 runs, %s CPUs)" % (
            statistics.median(tb), min(tb), max(tb), os.environ.get("OMP_NUM_THREADS", "all")))


def main():
    assert torch.cuda.is_available(), "cloud_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count,
                                          torch.__version__))
    say("times in ms: median [min .. max] over the windows; a window is `inner` back-to-back calls between two device events, after warm-up calls")
    lap_lines.extend(lines)
    for n in (10000, 200000):
        pts = cloud(n)
        verts = torch.from_numpy(pts).to(dev)
        say("--- %d points, k = %d" % (n, K))
        nbr = ops.knn(verts, verts, K, omit_diagonal=True)[1]
        if n == 10000:
            f64, gX64, _ = geometry.cloud_operators(torch.from_numpy(pts.astype(np.float64)), K)
            frames, gX, _ = geometry.cloud_operators(verts, K)
            s = torch.sign((frames[:, 2].cpu().double() * f64[:, 2]).sum(dim=1))
            say("kernel against the host route in fp64: normals (up to sign) %.2e, gradX entries %.2e" % (
                float((s[:, None] * frames[:, 2].cpu().double() - f64[:, 2]).abs().max()),
                float((gX.cpu().double() - gX64).coalesce().values().abs().max() / gX64.values().abs().max())))
        big = n > 50000                      # the brute-force query is quadratic: fewer, shorter windows at 200 000 points
        t_knn = dev_time(lambda: ops.knn(verts, verts, K, omit_diagonal=True), 2 if big else 20, 5 if big else 9, warm=1 if big else 3)
        say("ops.knn (neighbourhood query):                  %9.3f  [%.3f .. %.3f]" % t_knn)
        t_cl = dev_time(lambda: ops._cloud_launch(verts, nbr, None), 20, 15)       # the launch alone: no read of the status word
        gb = bytes_moved(n, K) / 1e9
        say("dn_cloud_operators_f32 (normals, frames, rows): %9.3f  [%.3f .. %.3f]  %.4f GB moved -> %.2f TB/s (plain float4 copy: 5.2-5.9 TB/s)" % (
            t_cl + (gb, gb / t_cl[0])))
        t_all = dev_time(lambda: geometry.cloud_operators(verts, K), 1 if big else 5, 3 if big else 9, warm=1)
        say("geometry.cloud_operators (both + torch coalesce): %7.3f  [%.3f .. %.3f]" % t_all)
        if n == 10000:
            host = torch.from_numpy(pts)
            tb = []
            for _ in range(3):
                t0 = time.perf_counter()
                geometry.cloud_operators(host, K)
                tb.append(1e3 * (time.perf_counter() - t0))
            say("host route of geometry.cloud_operators (fp32):  %9.1f  [%.1f .. %.1f]  (host clock, 3 runs, %s CPUs)" % (
                statistics.median(tb), min(tb), max(tb), os.environ.get("OMP_NUM_THREADS", "all")))
        time_laplacian(n, pts, verts, nbr, t_knn)
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "cloud_timing.txt"), "w").write("\n".join(lines) + "\n")
    open(os.path.join(OUT, "cloud_laplacian_timing.txt"), "w").write("\n".join(lap_lines) + "\n")


if __name__ == "__main__":
    main()

"""Times the two device steps of the point-cloud operators separately -- the neighbourhood query ``ops.knn`` (dn_knn.hip, k = 30,
omit_diagonal) and the per-point pass ``dn_cloud_operators_f32`` (dn_cloud.hip) -- at 10 000 and 200 000 points, and the host route of
``geometry.cloud_operators`` (KD-tree, batched SVD, vectorised 2 x 2 solves; what the reference does with a Python loop) at 10 000 points.
Device events around windows of back-to-back calls, warm-up first, median [min .. max] of the windows.  The per-point pass is also given as
bytes moved / time, next to the streaming rate the project records for a plain float4 copy (5.2-5.9 TB/s).  The
10 000-point result is checked against the host route in fp64 first.  Writes $DN_OUT_DIR/cloud_timing.txt (bash tools/gpu_run.sh cloud)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffusion_net import geometry, ops  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
K = 30
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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


def main():
    assert torch.cuda.is_available(), "cloud_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count,
                                          torch.__version__))
    say("times in ms: median [min .. max] over the windows; a window is `inner` back-to-back calls between two device events, after warm-up calls")
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
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "cloud_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Times ``ops.knn`` (dn_knn.hip) at the two workload shapes of geometry.find_knn -- the FAUST evaluation (6890 x 6890 x 30, k = 1) and the
point-cloud neighbourhood query (10000 x 10000 x 3, k = 30, omit_diagonal) -- against what the same job costs without the kernel:
(a) find_knn's own torch route past the kernel's limits (row blocks of the difference formula + topk) and a row-chunked torch.cdist + topk,
both on the same device, and (b) the reference's way, copy to host + sklearn KDTree.query.  Device events around windows of back-to-back calls, warm-up first, median [min .. max] of the windows.
Every timed result is checked against fp64 brute force first.  Writes $DN_OUT_DIR/knn_timing.txt (bash tools/gpu_run.sh knn)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import torch  # noqa: E402
from diffusion_net import geometry, ops  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
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


def against_fp64(src, tgt, k, omit, got):
    """(share of rows whose index set equals the fp64 top-k, worst relative distance error of the returned pairs)"""
    same, worst = 0, 0.0
    s64, t64 = src.double(), tgt.double()
    for r0 in range(0, src.shape[0], 1024):
        d = torch.cdist(s64[r0:r0 + 1024], t64, compute_mode="donot_use_mm_for_euclid_dist")
        if omit:
            n = d.shape[0]
            d[torch.arange(n), torch.arange(r0, r0 + n)] = float("inf")
        want = torch.topk(d, k, largest=False).indices.sort(dim=1).values
        idx = got[1][r0:r0 + 1024]
        same += int((idx.sort(dim=1).values == want).all(dim=1).sum())
        pair = d.gather(1, idx)
        worst = max(worst, float(((got[0][r0:r0 + 1024].double() - pair).abs() / pair).max()))
    return same / src.shape[0], worst


def cdist_topk(src, tgt, k, omit):
    """torch.cdist (non-matmul mode) + topk over at most 2^26 pairs at a time"""
    rows = max(1, (1 << 26) // tgt.shape[0])
    vals, inds = [], []
    for r0 in range(0, src.shape[0], rows):
        d = torch.cdist(src[r0:r0 + rows], tgt, compute_mode="donot_use_mm_for_euclid_dist")
        if omit:
            n = d.shape[0]
            d[torch.arange(n), torch.arange(r0, r0 + n)] = float("inf")
        top = torch.topk(d, k, largest=False)
        vals.append(top.values)
        inds.append(top.indices)
    return torch.cat(vals), torch.cat(inds)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return "; ".join(" ".join(l.split()) for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "not reported"
    except Exception as e:      # noqa: BLE001
        return "not read (%s)" % e


def main():
    assert torch.cuda.is_available(), "knn_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count,
                                          torch.__version__))
    say("clock state before (read, not set): " + clocks())
    say("times in ms: median [min .. max] over the windows; a window is `inner` back-to-back calls between two device events, after 3 warm-up calls")
    for N, D, k, omit, label in ((6890, 30, 1, False, "FAUST evaluation"), (10000, 3, 30, True, "point-cloud neighbourhoods")):
        g = torch.Generator().manual_seed(21)
        src = torch.randn(N, D, generator=g).to(dev)
        tgt = src if omit else torch.randn(N, D, generator=g).to(dev)
        say("--- %d x %d x %d, k = %d%s (%s)" % (N, N, D, k, ", omit_diagonal" if omit else "", label))
        kern = lambda ns=0: ops.knn(src, tgt, k, omit_diagonal=omit, n_split=ns)     # noqa: E731
        torch_path = lambda: geometry._knn_torch(src, tgt, k, False, omit)              # noqa: E731
        say("kernel against fp64 brute force:     rows with the exact top-k set %.6f, worst relative distance error %.2e" % against_fp64(src, tgt, k, omit, kern()))
        say("torch path against fp64 brute force: rows with the exact top-k set %.6f, worst relative distance error %.2e" % against_fp64(src, tgt, k, omit, tuple(torch_path())))
        say("cdist+topk against fp64 brute force: rows with the exact top-k set %.6f, worst relative distance error %.2e" % against_fp64(src, tgt, k, omit, cdist_topk(src, tgt, k, omit)))
        t = dev_time(kern, 20, 15)
        say("ops.knn (HIP kernel, library's slices):   %8.3f  [%.3f .. %.3f]  (15 windows of 20)" % t)
        t1 = dev_time(lambda: kern(1), 10, 9)
        say("ops.knn (HIP kernel, n_split = 1):        %8.3f  [%.3f .. %.3f]  (9 windows of 10)" % t1)
        ta = dev_time(torch_path, 3, 9)
        say("(a) find_knn's torch path on device:      %8.3f  [%.3f .. %.3f]  (9 windows of 3)" % ta)
        tc = dev_time(lambda: cdist_topk(src, tgt, k, omit), 3, 9)
        say("(a) chunked torch.cdist + topk on device: %8.3f  [%.3f .. %.3f]  (9 windows of 3; see its check above)" % tc)
        try:
            tb = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = geometry._knn_kdtree(src.cpu(), tgt.cpu(), k, omit)
                r.indices.to(dev)
                torch.cuda.synchronize()
                tb.append(1e3 * (time.perf_counter() - t0))
            say("(b) copy to host + sklearn KDTree.query:  %8.1f  [%.1f .. %.1f]  (host clock, 3 runs, %s CPUs)" % (
                statistics.median(tb), min(tb), max(tb), os.environ.get("OMP_NUM_THREADS", "all")))
        except ImportError as e:
            say("(b) not measured: %s" % e)
        say("kernel against (a): %.1fx the torch path, %.1fx cdist + topk" % (ta[0] / t[0], tc[0] / t[0]))
    say("clock state after: " + clocks())
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "knn_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

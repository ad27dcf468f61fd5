"""Times farthest point sampling (``ops.fps``, dn_fps.hip) at four shapes -- 1 000 -> 250, 10 000 -> 1 000, 200 000 -> 2 000 and a batch of
16 x 10 000 -> 1 000 each -- on every route that accepts the shape: the one-launch resident kernel, the stepped route (one launch per
sample) and the package's torch route (``geometry._fps_torch``: the reference's loop with the index kept on the device), all on the same
device and on the same, already normalised, points.  Device events around windows of back-to-back calls after warm-up; the contenders
alternate window by window in one process; median [min .. max] of the windows.  The first contender of every shape is timed a second time
(same code) to show the spread a difference has to exceed.  Every kernel result is compared with the torch route's mask first.
Writes $DN_OUT_DIR/fps_timing.txt (bash tools/gpu_run.sh fps); the committed copy is profiles/fps_timing.txt."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import torch  # noqa: E402
from diffusion_net import _hip, geometry, ops  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
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


def alternate(contenders, reps):
    """contenders: [(label, fn, inner)].  One warm-up call each, then `reps` rounds of one window per contender, in turn."""
    for _, fn, _ in contenders:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in contenders]
    for _ in range(reps):
        for i, (_, fn, inner) in enumerate(contenders):
            ts[i].append(window(fn, inner))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return "; ".join(" ".join(l.split()) for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)) or "not reported"
    except Exception as e:      # noqa: BLE001
        return "not read (%s)" % e


def sphere_cloud(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, 3, generator=g)
    p = p / p.norm(dim=1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1.0 / 3.0)       # uniform in the unit ball
    return geometry.normalize_positions(p.to(dev))


def main():
    assert torch.cuda.is_available(), "fps_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    cap = _hip.FPS_RESIDENT_MAX_POINTS
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count,
                                          torch.__version__))
    say("clock state before (read, not set): " + clocks())
    say("resident capacity: %d points per cloud" % cap)
    say("times in ms per call: median [min .. max] over the windows; a window is `inner` back-to-back calls between two device events; the "
        "contenders of a shape take turns window by window after one warm-up call each; 'again' is the first contender a second time")
    for n, n_sample, batch, label, reps in ((1000, 250, 1, "1 000 -> 250", 9), (10000, 1000, 1, "10 000 -> 1 000", 7),
                                            (200000, 2000, 1, "200 000 -> 2 000", 3), (10000, 1000, 16, "16 x 10 000 -> 1 000 each", 3)):
        clouds = [sphere_cloud(n, 100 + c, dev) for c in range(batch)]
        packed = torch.cat(clouds)
        offsets = [n * c for c in range(batch + 1)]
        say("--- %s" % label)

        def kern(route):
            return ops.fps(packed, n_sample, offsets=offsets if batch > 1 else None, route=route)

        def torch_route():
            return [geometry._fps_torch(c, n_sample) for c in clouds]

        want = torch.cat(torch_route())
        contenders = []
        if n <= cap:
            contenders.append(("resident route (1 launch)", lambda: kern(1), 10 if n_sample <= 1000 and batch == 1 else 3))
        contenders.append(("stepped route (%d launches)" % (n_sample + 1), lambda: kern(2), 5 if n < 100000 and batch == 1 else 2))
        for name, fn, _ in contenders:
            mask = torch.zeros(packed.shape[0], dtype=torch.bool, device=dev).index_fill_(0, fn()[0].reshape(-1), True)
            say("%-38s mask equal to the torch route's: %s" % (name, bool(torch.equal(mask, want))))
        contenders.append(("torch route (about %d launches)" % (6 * n_sample * batch), torch_route, 1))
        contenders.append(("again: " + contenders[0][0], contenders[0][1], contenders[0][2]))
        res = alternate(contenders, reps)
        for (name, _, inner), t in zip(contenders, res):
            say("%-46s %10.3f  [%.3f .. %.3f]  (%d windows of %d)   %.2f us per sample" % (
                (name, ) + t + (reps, inner, 1e3 * t[0] / n_sample)))
        spread = abs(res[-1][0] - res[0][0])
        say("same-code spread of the first contender: %.3f ms (%.1f %%)" % (spread, 100 * spread / res[0][0]))
        for (name, _, _), t in zip(contenders[:-2], res[:-2]):
            say("%s against the torch route: %.1fx  (median difference %.3f ms against a spread of %.3f ms)" % (
                name, res[-2][0] / t[0], res[-2][0] - t[0], spread))
    say("clock state after: " + clocks())
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "fps_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

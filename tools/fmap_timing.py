"""Times one forward plus backward step of the functional map at the shape of the functional_correspondence experiment -- V = 5000 vertices per
shape, k_eig = 128 stored eigenpairs, K = n_fmap = 30, F = 128 features, one pair -- three ways on the same device tensors:
(a) ``fmaps.functional_map`` on the HIP route (``geometry.to_basis`` + ``ops.fmap_solve``, dn_fmap.hip);
(b) this package's vectorised torch route (projection without diag(mass), one batched ``torch.linalg.solve_ex`` over the K systems);
(c) the experiment script's way, restated here: ``evecs^T[:K] @ diag(mass)`` as a dense K x V by V x V product per shape, then a Python loop
    over the K rows of the map with ``torch.inverse`` of a K x K matrix and a ``bmm`` each.
A step is: the map from features that require grad, mean((C - C_gt)^2), backward to both feature tensors.  Times are host clock around windows
of back-to-back steps that end in a device synchronise (route (c) waits for the device inside every step, so device events alone would not
see what it costs), after warm-up, in one process; median [min .. max] of the windows.  Kernel launches per step are counted with
torch.profiler in a pass of its own.  Every route is checked against the formula in fp64 first.  A last section times the solve alone,
forward + backward on coefficients projected beforehand (HIP op against the torch route's batched solve; device events).
Writes $DN_OUT_DIR/fmap_timing.txt (bash tools/gpu_run.sh fmap)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffusion_net import fmaps  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
V, K_EIG, K, F, LAM = 5000, 128, 30, 128, 1e-3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def shape(seed, dev):
    """mass, a basis with Phi^T M Phi = I, sorted eigenvalues starting at 0, features"""
    rs = np.random.RandomState(seed)
    mass = rs.uniform(0.5, 1.5, V) / V
    q, _ = np.linalg.qr(rs.randn(V, K_EIG))
    evals = 100.0 * (np.arange(K_EIG) + 0.5 * (seed % 2) + 0.25 * rs.uniform(0.0, 1.0, K_EIG)) / K_EIG    # two interleaved jittered grids
    evals[0] = 0.0
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    return dict(mass=f32(mass), evecs=f32(q / np.sqrt(mass)[:, None]), evals=f32(evals), feat=f32(rs.randn(V, F)))


def route_hip(x, y, fx, fy):
    return fmaps.functional_map(fx, fy, x["mass"], y["mass"], x["evals"], y["evals"], x["evecs"], y["evecs"], n_fmap=K, lambda_param=LAM)


def route_torch(x, y, fx, fy):
    A = x["evecs"][:, :K].t() @ (fx * x["mass"][:, None])
    B = y["evecs"][:, :K].t() @ (fy * y["mass"][:, None])
    return fmaps._solve_torch(A, B, x["evals"][:K], y["evals"][:K], LAM)


def route_script(x, y, fx, fy):
    """The experiment's model and function, restated (dense diag(mass); a row loop of torch.inverse)."""
    tx, ty = x["evecs"].t()[:K] @ torch.diag(x["mass"]), y["evecs"].t()[:K] @ torch.diag(y["mass"])
    A, B = (tx @ fx)[None], (ty @ fy)[None]
    ex, ey = x["evals"][None, :K], y["evals"][None, :K]
    D = (ex[:, None, :] - ey[:, :, None]) ** 2
    At = A.transpose(1, 2)
    G, H = torch.bmm(A, At), torch.bmm(B, At)
    rows = []
    for i in range(K):
        Di = torch.diag_embed(D[:, i, :])
        rows.append(torch.bmm(torch.inverse(G + LAM * Di), H[:, i, :, None]).transpose(1, 2))
    return torch.cat(rows, dim=1)[0]


def make_step(route, x, y, c_gt):
    fx, fy = x["feat"].clone().requires_grad_(True), y["feat"].clone().requires_grad_(True)

    def step():
        fx.grad = fy.grad = None
        C = route(x, y, fx, fy)
        ((C - c_gt) ** 2).mean().backward()
        return C.detach(), fx.grad, fy.grad
    return step


def wall_time(step, inner, reps, warm=5):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            step()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts)


def launches(step, n=5):
    """device kernels per step, from torch.profiler (memory copies and memsets not counted)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                step()
            torch.cuda.synchronize()
        ks = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "mem" not in e.name.lower()]
        return "%.0f" % (len(ks) / n) if ks else "not counted (the profiler reported no device events)"
    except Exception as e:      # noqa: BLE001
        return "not counted (%s)" % e


def main():
    assert torch.cuda.is_available(), "fmap_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count,
                                          torch.__version__))
    say("one forward + backward step of the functional map: V = %d per shape, k_eig = %d, K = %d, F = %d, one pair, lam = %g" % (V, K_EIG, K, F, LAM))
    say("times in ms per step, host clock: median [min .. max] over windows of back-to-back steps ending in a device synchronise, after 5 warm-up steps")
    x, y = shape(1, dev), shape(2, dev)
    c_gt = torch.randn(K, K, generator=torch.Generator().manual_seed(3)).to(dev)
    # the formula in fp64 on the device, from fp64 projections
    fx64, fy64 = x["feat"].double().requires_grad_(True), y["feat"].double().requires_grad_(True)
    d = lambda s: {k: v.double() for k, v in s.items()}   # noqa: E731
    C64 = route_torch(d(x), d(y), fx64, fy64)
    ((C64 - c_gt.double()) ** 2).mean().backward()
    steps = {}
    for name, route in (("(a) HIP route", route_hip), ("(b) torch route", route_torch), ("(c) script's row loop", route_script)):
        steps[name] = make_step(route, x, y, c_gt)
        C, gx, gy = steps[name]()
        rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())   # noqa: E731
        say("%-22s against the fp64 formula, max error over max magnitude: C %.2e, d feat_x %.2e, d feat_y %.2e" % (
            name, rel(C, C64.detach()), rel(gx, fx64.grad), rel(gy, fy64.grad)))
    res = {}
    for rnd in range(2):                       # two alternating rounds of the three routes: the spread between rounds is the noise
        for name, step in steps.items():
            t = wall_time(step, 20, 15)
            res.setdefault(name, []).append(t)
            say("%-22s round %d: %8.3f  [%.3f .. %.3f]  (15 windows of 20 steps)" % (name, rnd + 1, *t))
    for name, step in steps.items():
        say("%-22s device kernels per step: %s" % (name, launches(step)))
    med = {name: min(t[0] for t in ts) for name, ts in res.items()}
    a = med["(a) HIP route"]
    say("(a) against (b): %.2fx; (a) against (c): %.2fx (ratios of the better round's medians; above 1: (a) is faster)" % (
        med["(b) torch route"] / a, med["(c) script's row loop"] / a))
    # the solve alone, on coefficients projected beforehand: what the two routes differ in once the projections are taken out of the step
    say("--- the solve alone (forward + backward on prepared coefficients [K, F]; device events, median [min .. max] of 15 windows of 50)")
    from diffusion_net import ops
    A0 = (x["evecs"][:, :K].t() @ (x["feat"] * x["mass"][:, None])).contiguous()
    B0 = (y["evecs"][:, :K].t() @ (y["feat"] * y["mass"][:, None])).contiguous()
    ex, ey, dC = x["evals"][:K].contiguous(), y["evals"][:K].contiguous(), torch.randn(K, K, generator=torch.Generator().manual_seed(4)).to(dev)
    for name, fn in (("ops.fmap_solve (HIP)", lambda a, b: ops.fmap_solve(a, b, ex, ey, LAM)),
                     ("fmaps._solve_torch", lambda a, b: fmaps._solve_torch(a, b, ex, ey, LAM))):
        a, b = A0.clone().requires_grad_(True), B0.clone().requires_grad_(True)

        def solve_step(fn=fn, a=a, b=b):
            a.grad = b.grad = None
            fn(a, b).backward(dC)
        for _ in range(5):
            solve_step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(15):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                solve_step()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 50)
        say("%-22s %8.3f  [%.3f .. %.3f]   device kernels per step: %s" % (name, statistics.median(ts), min(ts), max(ts), launches(solve_step)))
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "fmap_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

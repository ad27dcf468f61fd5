"""Measures the implicit diffusion (``diffusion_method="implicit_sparse"``: per-channel Jacobi-PCG on the device, dn_implicit.hip) on
``synthetic.sphere_mesh`` with diffusion times drawn as ``synthetic.randomize_times`` draws them, U(1e-3, 0.3) (needs a ROCm device):

  1. (no comparison with the ``"implicit_dense"`` torch route on the same device: ``torch.linalg.cholesky`` of that route raises
     hipErrorLaunchFailure on gfx950 at [1, 5, 300, 300])
  2. at sizes the dense form cannot reach, V = 10 000 and 16 x 10 000, C = 128: iterations to rtol = 1e-9 per channel (min / median / max),
     the whole solve (``ops.implicit_solve``, check=True: with its host reads), time per iteration and per launch, call to call, from two
     check=False runs of different lengths; the layer's forward plus backward; and, for orientation only, the spectral ``DiffusionFn`` forward
     plus backward on a batch of the same size at K = 128 (random eigenvectors: its time does not depend on their values)
  3. ``--one-solve``: one V = 10 000, C = 128 solve of 40 iterations and nothing else, for a kernel trace in a run of its own
     (rocprofv3 --kernel-trace --stats ... -- python tools/implicit_timing.py --one-solve); ``--stats FILE``: the share of every im_* kernel
     in that trace's kernel_stats.csv

-> $DN_OUT_DIR/implicit_timing.txt            python tools/implicit_timing.py"""
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
RTOL = 1e-9
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ts):
    return "%.2f ms [%.2f .. %.2f]" % (statistics.median(ts), min(ts), max(ts))


def timed(fn, n):
    """Device-event time of n calls of fn, in ms per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def windows(fns, reps, n):
    """Alternating windows: every function once per round, ``reps`` rounds of ``n`` calls."""
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            out[i].append(timed(fn, n))
    return out


def operator(V, copies, dev):
    """(L scipy fp32 block diagonal, torch sparse L [B, V, V], mass [B, V]) of ``copies`` sphere meshes of V vertices."""
    from diffusion_net import precompute as P, synthetic
    v, f = synthetic.sphere_mesh(V, seed=1)
    L = sp.csr_matrix(P.cotan_laplacian(v, f, 1e-10)).astype(np.float32)
    L.sort_indices()
    m = P.vertex_areas(v, f).astype(np.float32)
    coo = sp.coo_matrix(L)
    Lt = torch.sparse_coo_tensor(torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)), torch.from_numpy(coo.data), L.shape).coalesce().to(dev)
    mt = torch.from_numpy(m).to(dev)
    return L, m, torch.stack([Lt] * copies), torch.stack([mt] * copies)


def draw_times(C, seed=0):
    from diffusion_net import synthetic
    return synthetic.randomize_times({"diffusion_time": torch.zeros(C)}, seed=seed)["diffusion_time"]


def layer_step(lay, x, L, mass):
    def step():
        lay.diffusion_time.grad = None
        x.grad = None
        lay(x, L, mass, None, None).square().sum().backward()
    return step


def mesh_sizes(dev):
    from diffusion_net import layers, ops
    from diffusion_net.batch import MeshBatch
    C, K, V = 128, 128, 10000
    for copies in (1, 16):
        L, m, Lb, mb = operator(V, copies, dev)
        lay = layers.LearnedTimeDiffusion(C, method="implicit_sparse").to(dev)
        with torch.no_grad():
            lay.diffusion_time.copy_(draw_times(C))
        op = layers._implicit_operator_of(Lb, mb)
        t = lay.diffusion_time.detach()
        u = torch.randn(copies * V, C, device=dev)
        args = (op.rowptr, op.col, op.val, op.mass, t, u, op.sizes)
        x, info = ops.implicit_solve(*args, rtol=RTOL, return_info=True)
        its = info["iterations"].cpu().numpy()
        per_channel = its.max(axis=0)
        say("")
        say("== 2. %d x sphere_mesh(%d), C = %d: %d rows, %d entries of L, %d tiles" % (copies, V, C, copies * V, op.col.numel(), op.n_tiles))
        say("iterations to rtol = 1e-9 per channel: min %d, median %d, max %d   (residual <= %.2e; %d launches in that solve)"
            % (per_channel.min(), int(np.median(per_channel)), per_channel.max(), float(info["residual"].max()), info["launches"]))
        whole = windows([lambda: ops.implicit_solve(*args, rtol=RTOL)], 5, 2)[0]
        say("whole solve, ops.implicit_solve check=True (a host read every 16 iterations): %s" % spread(whole))
        n1, n2 = 10, 30
        short, long_ = windows([lambda: ops.implicit_solve(*args, rtol=RTOL, max_iter=n1, check=False),
                                lambda: ops.implicit_solve(*args, rtol=RTOL, max_iter=n2, check=False)], 7, 2)
        per_it = (statistics.median(long_) - statistics.median(short)) / (n2 - n1)
        moved = 11 * copies * V * C * 8
        say("one iteration (4 launches), from check=False runs of %d and %d iterations: %.1f us, %.1f us per launch call to call; the passes move"
            " about %.0f MB per iteration at least -> %.2f TB/s" % (n1, n2, 1e3 * per_it, 1e3 * per_it / 4, moved / 1e6, moved / (per_it * 1e-3) / 1e12))
        say("   (%d-iteration runs %s, %d-iteration runs %s; channels that finish early stop being stored)" % (n1, spread(short), n2, spread(long_)))
        xl = u.reshape(copies, V, C).clone().requires_grad_(True)
        step = layer_step(lay, xl, Lb, mb)
        step()
        both = windows([step], 5, 2)[0]
        say("LearnedTimeDiffusion('implicit_sparse') forward + backward: %s" % spread(both))
        # the spectral route on a batch of the same size, for orientation
        g = torch.Generator().manual_seed(0)
        evecs = [torch.randn(V, K, generator=g).to(dev) for _ in range(1)] * copies
        evals = [torch.linspace(0.0, 50.0, K).to(dev)] * copies
        mbatch = MeshBatch.from_operators([mb[0]] * copies, evals, evecs)
        xs = u.clone().requires_grad_(True)
        ts = t.clone().requires_grad_(True)

        def spectral():
            xs.grad = None
            ts.grad = None
            ops.DiffusionFn.apply(xs, ts, mbatch).square().sum().backward()
        spectral()
        spec = windows([spectral], 5, 5)[0]
        say("for orientation, the spectral DiffusionFn forward + backward on the same rows at K = %d: %s" % (K, spread(spec)))


def one_solve(dev):
    from diffusion_net import layers, ops
    L, m, Lb, mb = operator(10000, 1, dev)
    op = layers._implicit_operator_of(Lb, mb)
    u = torch.randn(10000, 128, device=dev)
    t = draw_times(128).to(dev)
    for _ in range(2):
        ops.implicit_solve(op.rowptr, op.col, op.val, op.mass, t, u, op.sizes, rtol=RTOL, max_iter=40, check=False)
    torch.cuda.synchronize()


def stats(path):
    """Shares from a rocprofv3 kernel_stats.csv (columns "Name", "Calls", "TotalDurationNs", ... as in profiles/r06_bench_kernel_stats.csv;
    names are demangled: "void (anonymous namespace)::im_product_kernel<false>((anonymous namespace)::ImArgs)")."""
    import re
    im = []
    for r in csv.DictReader(open(path)):
        hit = re.search(r"\bim_\w+(<[^>]*>)?", r["Name"])
        if hit:
            im.append((hit.group(0), int(r["Calls"]), float(r["TotalDurationNs"])))
    passes = ("im_product_kernel<false>", "im_update_kernel", "im_reduce_kernel", "im_pupdate_kernel")
    per_it = sum(d for n, _, d in im if n in passes)
    assert per_it > 0, "no im_* kernel in %s" % path
    out = ["== 3. kernel trace of 2 x 40 iterations at V = 10 000, C = 128 (rocprofv3 --kernel-trace --stats, a run of its own)"]
    for n, calls, d in sorted(im, key=lambda p: -p[2]):
        share = "%5.1f %% of the four passes of an iteration" % (100.0 * d / per_it) if n in passes else "(not part of an iteration)"
        out.append("%-28s %5d calls %10.1f us total %8.2f us per call   %s" % (n, calls, d / 1e3, d / 1e3 / calls, share))
    print("\n".join(out))
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "implicit_timing_trace.txt"), "w").write("\n".join(out) + "\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        return stats(sys.argv[2])
    assert torch.cuda.is_available(), "implicit_timing needs a ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    if len(sys.argv) > 1 and sys.argv[1] == "--one-solve":
        return one_solve(dev)
    say("implicit diffusion, Jacobi-PCG in fp64, rtol = 1e-9; %s" % torch.cuda.get_device_name(dev))
    mesh_sizes(dev)
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "implicit_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Measures the Laplacian eigenbasis of ``geometry.laplacian_eigenbasis`` (Chebyshev-filtered subspace iteration, dn_eigen.hip) against the
shift-invert ``eigsh`` of ``precompute.laplacian_eigenbasis`` on the same box, on ``synthetic.sphere_mesh`` at 10 000 and 2 000 vertices,
k_eig = 128 (needs a ROCm device):

  device route   end to end -- S built on the host and uploaded, the solve, the results on the device, a final synchronisation; host clock,
                 one warm-up, median [min .. max] of 5
  one product    ``dn_cheb_step_f64`` on a [V, 160] block: device events around windows of 20 back-to-back recurrence steps, warm-up first,
                 median [min .. max] per call, and the bytes a call moves at least (S once, Y, Z and out once) over that time
  shares         one more solve with a synchronisation around every block operation: products with S, tall dense products (torch), transfers,
                 and what is left -- the nb x nb eigh / Cholesky factorisations and the driver on the host.  The synchronisations make this
                 run slower than the end-to-end figure; the shares are of its own total.
  eigsh          ``precompute.laplacian_eigenbasis`` (SuperLU + ARPACK) with the threads the machine gives, median [min .. max] of 3

-> $DN_OUT_DIR/eigenbasis_timing.txt            python tools/eigen_timing.py   (bash tools/gpu_run.sh eigen)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
K = 128
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def spread(ts):
    return "%.1f ms [%.1f .. %.1f]" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def main():
    from diffusion_net import geometry, ops, precompute as P, synthetic
    assert torch.cuda.is_available(), "eigen_timing needs a ROCm device"
    dev = torch.device("cuda", torch.cuda.current_device())
    say("Laplacian eigenbasis, k_eig = %d, fp64, rtol = 1e-9; %s; %d host threads" % (K, torch.cuda.get_device_name(dev), torch.get_num_threads()))

    class Timed(geometry._TorchBlocks):
        def __init__(self, S, dev):
            super().__init__(S, dev)
            self.t = dict(products=0.0, dense=0.0, transfers=0.0)

    def timed(kind, name):
        plain = getattr(geometry._TorchBlocks, name)

        def fn(self, *a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = plain(self, *a, **k)
            torch.cuda.synchronize()
            self.t[kind] += time.perf_counter() - t0
            return r
        setattr(Timed, name, fn)
    for kind, names in (("products", ("step",)), ("dense", ("tmm", "mm", "solve_upper_right", "residuals", "finish")),
                        ("transfers", ("from_host", "to_host"))):
        for name in names:
            timed(kind, name)

    for V in (10000, 2000):
        v, f = synthetic.sphere_mesh(V, seed=1)
        L = P.cotan_laplacian(v, f, 1e-10)
        m = P.vertex_areas(v, f)
        m = m + P.EPS * m.mean()
        mass = torch.from_numpy(m).to(dev)
        say("")
        say("== sphere_mesh(%d): %d entries of L" % (V, L.nnz))
        ts, info = [], None
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evals, evecs, info = geometry.laplacian_eigenbasis(L, mass, K, dtype=torch.float64, return_info=True)
            torch.cuda.synchronize()
            if i:
                ts.append(time.perf_counter() - t0)
        say("device route, end to end: %s   (%d iterations, %d products with S, degrees %s, nb = %d)" % (
            spread(ts), info["iterations"], info["products"], info["degrees"], info["nb"]))
        t_dev = statistics.median(ts)
        # one product
        S, d, ub = P.scaled_operator(L, m)
        be = geometry._TorchBlocks(S, dev)
        nb = info["nb"]
        a, b = (torch.randn(V, nb, dtype=torch.float64, device=dev) for _ in range(2))
        for _ in range(5):
            ops.cheb_step(be.rowptr, be.col, be.val, a, b, 1e-4, -1.0, -1.0, out=b)
        per = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.normal_(); b.normal_()
            e0.record()
            for _ in range(10):
                ops.cheb_step(be.rowptr, be.col, be.val, a, b, 1e-4, -1.0, -1.0, out=b)
                ops.cheb_step(be.rowptr, be.col, be.val, b, a, 1e-4, -1.0, -1.0, out=a)
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / 20.0 * 1e-3)
        moved = S.nnz * 12 + (V + 1) * 4 + 3 * V * nb * 8
        say("one product, dn_cheb_step_f64 on [%d, %d] (%d entries of S): %.1f us [%.1f .. %.1f] per call; %.1f MB at least per call -> %.2f TB/s" % (
            V, nb, S.nnz, 1e6 * statistics.median(per), 1e6 * min(per), 1e6 * max(per), moved / 1e6, moved / statistics.median(per) / 1e12))
        say("   (Python call to call, launch overhead included; the gathered rows of Y are re-read from cache %.1f times over)" % (S.nnz / V))
        # shares
        tb = Timed(S, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.subspace_iterate(tb, V, d, ub, K)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        host = total - sum(tb.t.values())
        say("shares of a solve with a synchronisation around every block operation (%.1f ms): products with S %.0f %%, tall dense products %.0f %%, "
            "transfers %.0f %%, host factorisations and driver %.0f %%" % (
                1e3 * total, 100 * tb.t["products"] / total, 100 * tb.t["dense"] / total, 100 * tb.t["transfers"] / total, 100 * host / total))
        # eigsh
        te = []
        for _ in range(3):
            t0 = time.perf_counter()
            ev, _ = P.laplacian_eigenbasis(L, m, K)
            te.append(time.perf_counter() - t0)
        t_eigsh = statistics.median(te)
        say("eigsh (precompute.laplacian_eigenbasis, host): %s" % spread(te))
        say("eigenvalues of the two routes: max |difference| = %.2e lambda_k" % (np.abs(evals.cpu().numpy() - ev).max() / ev[-1]))
        say("device route / eigsh = %.3f%s" % (t_dev / t_eigsh, ("   -> the expected factor (less than half of eigsh at V = 10 000) is %s"
                                                               % ("MET" if t_dev < 0.5 * t_eigsh else "NOT MET")) if V == 10000 else ""))
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "eigenbasis_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

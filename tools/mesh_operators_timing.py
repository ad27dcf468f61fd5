"""Times the assembly of a triangle mesh's operators in front of the eigenproblem -- normals, frames, cotan Laplacian, lumped mass, gradient
operator -- on ``synthetic.sphere_mesh`` at 10 000 and 200 000 vertices, two ways on the same box:
(a) ``geometry.mesh_operators`` on fp32 device tensors (``ops.mesh_assemble`` + ``ops.mesh_frames_gradients``, dn_mesh.hip): five device tensors;
(b) the host functions it replaces (``precompute.vertex_normals``, ``tangent_frames``, ``cotan_laplacian``, ``vertex_areas``,
    ``gradient_operator``; numpy / scipy in fp64 on this box's threads), alone and with the upload of their five results as
    ``compute_operators`` does it (``_to_torch_sparse``).
Times are host clock around windows of back-to-back calls that end in a device synchronise, after warm-up, in one process, in alternating
rounds of the routes; median [min .. max] of the windows.  A second section times the device steps one by one with device events (face pass,
the two stable sorts with their run ranks, the two segment sums, the normalisation, the vertex pass): median of 20 repetitions each.  The
device route is checked against the host route first.  Writes $DN_OUT_DIR/mesh_operators_timing.txt (bash tools/gpu_run.sh mesh)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffusion_net import _hip, geometry, ops, precompute, synthetic  # noqa: E402

OUT = os.environ.get("DN_OUT_DIR", os.path.join(ROOT, "out"))
SIZES = (10_000, 200_000)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def host_functions(v64, f):
    n = precompute.vertex_normals(v64, f)
    frames = precompute.tangent_frames(n)
    L = precompute.cotan_laplacian(v64, f, denom_eps=1e-10)
    mass = precompute.vertex_areas(v64, f)
    Lc = L.tocoo()
    grad = precompute.gradient_operator(v64, frames, np.stack([Lc.row, Lc.col]))
    return frames, mass, L, grad


def host_with_upload(v64, f, dev):
    frames, mass, L, grad = host_functions(v64, f)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=torch.float32)   # noqa: E731
    sp = lambda m: precompute._to_torch_sparse(m, dev, torch.float32)   # noqa: E731
    return t(frames), t(mass), sp(L), sp(grad.real), sp(grad.imag)


def windows(fn, inner, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts)


def device_steps(tv, tf, reps=20):
    """The steps of ``ops._mesh_assemble_launch`` and of the vertex pass, one by one between device events (the same calls in the same order)."""
    L = _hip.lib()
    V, F = tv.shape[0], tf.shape[0]
    dev, st, m = tv.device, _hip.stream_of(tv), 9 * tf.shape[0]
    names = ("face pass", "sort of L's keys + run ranks", "segment sum (L, CSR)", "sort of the vertex keys", "segment sum (vertex records)",
             "normalisation (torch)", "vertex pass")
    acc = {k: [] for k in names}
    for _ in range(reps + 2):
        rowptr = torch.zeros(V + 1, dtype=torch.int32, device=dev)
        col = torch.empty(m, dtype=torch.int32, device=dev)
        lval = torch.empty(m, dtype=torch.float64, device=dev)
        vrec = torch.zeros(V, 4, dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _hip.workspace(dev, L.dn_mesh_workspace_bytes(V, F))
        Fe = (F + 1) // 2 * 2
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        _hip.check(L.dn_mesh_emit_f32(tv.data_ptr(), V, tf.data_ptr(), F, ws.data_ptr(), ws.numel(), status.data_ptr(), st), "emit")
        ev[1].record()
        key_l, val_l = ws[:72 * F].view(torch.int64), ws[72 * Fe:72 * Fe + 72 * F].view(torch.float64)
        key_v, val_v = ws[144 * Fe:144 * Fe + 24 * F].view(torch.int64), ws[168 * Fe:168 * Fe + 96 * F].view(torch.float64)
        skey, perm = torch.sort(key_l, stable=True)
        head = torch.ones(m, dtype=torch.bool, device=dev)
        torch.ne(skey[1:], skey[:-1], out=head[1:])
        rank = torch.cumsum(head, 0, dtype=torch.int64)
        ev[2].record()
        _hip.check(L.dn_segment_sum_f64_f64(skey.data_ptr(), perm.data_ptr(), val_l.data_ptr(), m, rank.data_ptr(), V, rowptr.data_ptr(), col.data_ptr(),
                                            lval.data_ptr(), count.data_ptr(), st), "sum")
        ev[3].record()
        skey_v, perm_v = torch.sort(key_v, stable=True)
        ev[4].record()
        _hip.check(L.dn_segment_sum4_f64_f64(skey_v.data_ptr(), perm_v.data_ptr(), val_v.data_ptr(), 3 * F, V, vrec.data_ptr(), st), "sum4")
        ev[5].record()
        nsum = vrec[:, 1:]
        normals = (nsum / torch.linalg.vector_norm(nsum, dim=1, keepdim=True)).contiguous()
        ev[6].record()
        ops._mesh_frames_gradients_launch(tv, rowptr, col, normals)
        ev[7].record()
        torch.cuda.synchronize()
        for i, k in enumerate(names):
            acc[k].append(ev[i].elapsed_time(ev[i + 1]))
    return [(k, statistics.median(v[2:])) for k, v in acc.items()], int(count.item())


def main():
    assert torch.cuda.is_available(), "mesh_operators_timing.py measures on a ROCm device; there is nothing to time without one"
    dev = torch.device("cuda:0")
    say("device: %s, %d CUs; torch %s; host threads: %d (torch), OMP_NUM_THREADS=%s" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count, torch.__version__, torch.get_num_threads(),
        os.environ.get("OMP_NUM_THREADS", "unset")))
    say("assembly of a mesh's operators in front of the eigenproblem (normals, frames, cotan Laplacian, mass, gradient operator), synthetic.sphere_mesh")
    say("times in ms per call, host clock: median [min .. max] over windows of back-to-back calls ending in a device synchronise, after 2 warm-up calls")
    for V in SIZES:
        v, f = synthetic.sphere_mesh(V)
        v32 = v.astype(np.float32)
        v64 = v32.astype(np.float64)
        tv, tf = torch.from_numpy(v32).to(dev), torch.from_numpy(f).to(dev)
        say("--- V = %d, F = %d" % (V, f.shape[0]))
        got = geometry.mesh_operators(tv, tf)
        ref = host_with_upload(v64, f, dev)
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())   # noqa: E731
        dense = lambda t: t.coalesce().values() if t.is_sparse else t   # noqa: E731
        say("device route against the host route, max difference over max magnitude (fp32 tensors): frames %.2e, mass %.2e, L %.2e, gradX %.2e, gradY %.2e; "
            "same pattern: %s" % (*(rel(dense(a), dense(b)) for a, b in zip(got, ref)), bool(torch.equal(got[2].indices(), ref[2].coalesce().indices()))))
        inner = 20 if V <= 20_000 else 3
        routes = (("(a) geometry.mesh_operators, device", lambda: geometry.mesh_operators(tv, tf), inner, 9),
                  ("(b) host functions alone", lambda: host_functions(v64, f), 1, 5),
                  ("(b) host functions + upload", lambda: host_with_upload(v64, f, dev), 1, 5))
        res = {}
        for rnd in range(2):                   # two alternating rounds of the routes: the spread between rounds is the noise
            for name, fn, n_in, reps in routes:
                t = windows(fn, n_in, reps)
                res.setdefault(name, []).append(t)
                say("%-38s round %d: %9.3f  [%.3f .. %.3f]  (%d windows of %d calls)" % (name, rnd + 1, *t, reps, n_in))
        med = {name: min(t[0] for t in ts) for name, ts in res.items()}
        a = med["(a) geometry.mesh_operators, device"]
        say("(b) alone over (a): %.2fx; (b) with upload over (a): %.2fx (ratios of the better round's medians; above 1: the device route is faster)" % (
            med["(b) host functions alone"] / a, med["(b) host functions + upload"] / a))
        steps, nnz = device_steps(tv, tf)
        say("device steps one by one, device events, median of 20 repetitions (nnz = %d):" % nnz)
        for k, t in steps:
            say("    %-32s %8.3f ms" % (k, t))
        say("    %-32s %8.3f ms  (route (a) adds: one host read of the status word and nnz, a finiteness check of the normals, a NaN check of"
            " the frames, the casts and the three sparse tensors)" % ("sum of the steps", sum(t for _, t in steps)))
        os.makedirs(OUT, exist_ok=True)        # (after every size: a run that is cut short leaves what it measured)
        open(os.path.join(OUT, "mesh_operators_timing.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

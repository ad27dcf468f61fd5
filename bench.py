#!/usr/bin/env python
"""bench.py -- DiffusionNet training-step throughput on MI355X (BASELINE.json metric).

One "step" = forward + NLL loss + backward (+ RCCL gradient all-reduce for N>1) + Adam update over
one ragged batch of synthetic meshes per GPU (weak scaling: every rank owns its own batch).
Workload (config.workload): BASELINE configs[1] shape (human-segmentation net: C_in=3, C_out=8,
C_width=128, K=128, N_block=4, per-face outputs, dropout on) at the north-star size
(>=10k-vertex meshes, batch of meshes).

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, ms_per_step (milliseconds per timed step), the
configuration.  A plain run sets up, warms up, times --steps steps and prints that line, nothing else.  With --full the line also holds
  roofline     -- dominant kernel family, algorithmic flops (or bytes) / hipEvent-measured duration
  parity       -- the product path against the reference's own outputs (committed fixtures), measured in this run
  cpu_baseline -- the CPU oracle (torch-CPU restatement of the reference) on a bounded sample
and the diffusion-block bandwidth, the all-reduce alone (N > 1) and short runs of the other BASELINE configs.
--dump-outputs DIR writes what the last timed step computed (loss, log-probabilities, updated parameters, gradients) as DIR/<name>.npy;
the inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "diffusion-net_amd"))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist
import torch.nn.functional as F

PEAK_MFMA_F32_TFLOPS = 157.3      # MI355X_MICROARCH.md: exact-f32 MFMA = f32 vector peak
PEAK_HBM_GBPS = 8000.0            # HBM3E spec (6.29 TB/s measured copy ceiling)
PEAK_MFMA_BF16_TFLOPS = 2500.0    # dense bf16 MFMA (no sparsity)
TRAFFIC_JSON = "r06_traffic.json"  # PMC FETCH/WRITE passes of the same kernels (tools/pmc_run.sh + tools/traffic_summary.py), committed under profiles/


def mesh_sizes(n_meshes, v_mean, rank):
    # ragged but deterministic: +-10 % around v_mean
    g = torch.Generator().manual_seed(1234 + rank)
    return [int(v_mean * (0.9 + 0.2 * torch.rand(1, generator=g).item())) for _ in range(n_meshes)]


def build_batch(sizes, K, device, seed0):
    from diffusion_net import synthetic
    from diffusion_net.batch import GatherPattern, MeshBatch
    meshes = [synthetic.make_mesh_operators(v, K, seed=seed0 + i) for i, v in enumerate(sizes)]
    mb = MeshBatch.from_operators([m["mass"] for m in meshes], [m["evals"] for m in meshes],
                                  [m["evecs"] for m in meshes], [m["gradX"] for m in meshes],
                                  [m["gradY"] for m in meshes], device=device)
    offs, faces = 0, []
    for m, v in zip(meshes, sizes):
        faces.append(m["faces"] + offs)
        offs += v
    faces = torch.cat(faces, 0).to(device)
    gather = GatherPattern(faces, sum(sizes))
    x = torch.cat([m["verts"] for m in meshes], 0).to(device)
    return meshes, mb, gather, x


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float32 (float64 kept), at most DUMP_BUDGET_BYTES in all.  The smaller arrays
    are written whole; an array beyond what is left of the budget is written as a fixed sample of its rows (seeded, sorted) with the row
    indices next to it as <name>_rows.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_BYTES - 4096 * 2 * len(arrays)          # (headroom for the .npy headers)
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())
    for i, (name, t) in enumerate(items):
        share = left // (len(items) - i)
        t = t.detach()
        t = t.double() if t.dtype == torch.float64 else t.float()
        if t.dim() > 0 and t.numel() * t.element_size() > share:
            row_bytes = (t.numel() // max(1, t.shape[0])) * t.element_size() + 8
            n_keep = max(1, min(t.shape[0], share // row_bytes))
            g = torch.Generator().manual_seed(0)
            rows = torch.randperm(t.shape[0], generator=g)[:n_keep].sort().values
            t = t[rows.to(t.device)]
            np.save(os.path.join(out_dir, name + "_rows.npy"), rows.double().numpy())
            left -= n_keep * 8
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
        left -= t.numel() * t.element_size()


def _import_reference():
    """The reference package itself, when its sources are reachable (dev container only; never on the GPU box)."""
    import types
    if not os.path.isdir("/root/reference/src/diffusion_net"):
        return None
    try:
        import importlib.util
        for name in ("potpourri3d", "robust_laplacian"):
            sys.modules.setdefault(name, types.ModuleType(name))
        spec = importlib.util.spec_from_file_location("ref_diffusion_net", "/root/reference/src/diffusion_net/__init__.py",
                                                      submodule_search_locations=["/root/reference/src/diffusion_net"])
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_diffusion_net"] = mod
        spec.loader.exec_module(mod)
        return mod
    except Exception:      # noqa: BLE001
        return None


def cpu_baseline(args, C_out, sizes):
    """The reference's training loop on the host CPU: one mesh per optimizer step (DataLoader(batch_size=None),
    human_segmentation_original.py:61), fwd + NLL + bwd + Adam, the first meshes of THIS benchmark batch.  Timed with the imported
    reference module when its sources are reachable (kind "reference"), else with the in-repo oracle restatement (kind "port");
    swept over thread counts, the best is reported with its core count."""
    import diffusion_net
    from diffusion_net import synthetic
    from oracle import diffusionnet_oracle as orc
    ref = _import_reference()
    n_sample = min(3, len(sizes))
    meshes = [synthetic.make_mesh_operators(v, args.keig, seed=i) for i, v in enumerate(sizes[:n_sample])]
    labels = [torch.randint(0, C_out, (m["faces"].shape[0],)) for m in meshes]
    lsm = lambda t: F.log_softmax(t, dim=-1)
    torch.manual_seed(0)
    sd = synthetic.randomize_times(diffusion_net.layers.DiffusionNet(3, C_out, C_width=args.cwidth, N_block=args.blocks, outputs_at="faces").state_dict(), seed=0)
    if ref is not None:
        model = ref.layers.DiffusionNet(3, C_out, C_width=args.cwidth, N_block=args.blocks, outputs_at="faces", dropout=True, last_activation=lsm)
        model.load_state_dict(sd)
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def step(i):
            m = meshes[i % n_sample]
            opt.zero_grad()
            out = model(m["verts"], m["mass"], L=None, evals=m["evals"], evecs=m["evecs"], gradX=m["gradX"], gradY=m["gradY"], faces=m["faces"])
            F.nll_loss(out, labels[i % n_sample]).backward()
            opt.step()
    else:
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(params.values()), lr=1e-3)

        def step(i):
            m = meshes[i % n_sample]
            V = m["verts"].shape[0]
            opt.zero_grad()
            masks = [[torch.bernoulli(torch.full((V, args.cwidth), 0.5)) for _ in range(2)] for _ in range(args.blocks)]
            p = {k: (orc.clamp_time(v) if k.endswith("diffusion_time") else v) for k, v in params.items()}
            out = orc.net_forward(p, m["verts"], m["mass"], m["evals"], m["evecs"], m["gradX"], m["gradY"], faces=m["faces"],
                                  outputs_at="faces", last_activation=lsm, keep_masks=masks)
            F.nll_loss(out, labels[i % n_sample]).backward()
            opt.step()
    ncpu = os.cpu_count() or 1
    sweep, best = {}, None
    prev_threads = torch.get_num_threads()
    for nt in sorted({min(8, ncpu), min(16, ncpu), min(32, ncpu), min(64, ncpu)}):   # beyond 64 threads the fp32 CPU path only gets slower
        torch.set_num_threads(nt)
        tw = time.perf_counter()
        step(0)                                              # warm-up (thread pool, allocator)
        tw = time.perf_counter() - tw
        if tw > 8.0:                                         # hopelessly oversubscribed: one step is the sample
            sweep[str(nt)] = round(sizes[0] / tw, 1)
            continue
        t0, n, v = time.perf_counter(), 0, 0
        while n < 2 * n_sample and (time.perf_counter() - t0 < 6.0 or n < n_sample):
            step(n)
            v += sizes[n % n_sample]
            n += 1
        rate = v / (time.perf_counter() - t0)
        sweep[str(nt)] = round(rate, 1)
        if best is None or rate > best[0]:
            best = (rate, nt, n)
    torch.set_num_threads(prev_threads)
    return {"value": best[0], "unit": "vertices/s", "cores": best[1], "kind": "reference" if ref is not None else "port",
            "sample": "%d train steps, one mesh per step as the reference's loop, over the first %d meshes (%s vertices) of the benchmark batch, "
                      "fp32, same net/config; best of thread counts %s (vertices/s per count: %s); host has %d logical CPUs"
                      % (best[2], n_sample, "/".join(str(s_) for s_ in sizes[:n_sample]), sorted(int(k) for k in sweep), sweep, ncpu)}


def torch_rocm_baseline(args, C_out, sizes, device):
    """SURVEY 8d's optional second baseline: the SAME restatement the CPU baseline times (oracle/, plain torch ops), but with its tensors on
    the MI355X -- i.e. what stock PyTorch-ROCm (rocBLAS GEMMs, rocSPARSE COO products, elementwise kernels, autograd) makes of this
    network on this GPU, in the reference's one-mesh-per-step loop.  Baseline only; returns None if an op is missing on this build."""
    try:
        import diffusion_net
        from diffusion_net import synthetic
        from oracle import diffusionnet_oracle as orc
        n_sample = min(3, len(sizes))
        meshes = [{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in synthetic.make_mesh_operators(vv, args.keig, seed=i).items()}
                  for i, vv in enumerate(sizes[:n_sample])]
        labels = [torch.randint(0, C_out, (m["faces"].shape[0],), device=device) for m in meshes]
        lsm = lambda t: F.log_softmax(t, dim=-1)
        sd = synthetic.randomize_times(diffusion_net.layers.DiffusionNet(3, C_out, C_width=args.cwidth, N_block=args.blocks, outputs_at="faces").state_dict(), seed=0)
        params = {k: v.clone().to(device).requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.Adam(list(params.values()), lr=1e-3)

        def step(i):
            m = meshes[i % n_sample]
            V = m["verts"].shape[0]
            opt.zero_grad()
            masks = [[torch.bernoulli(torch.full((V, args.cwidth), 0.5, device=device)) for _ in range(2)] for _ in range(args.blocks)]
            p = {k: (orc.clamp_time(v) if k.endswith("diffusion_time") else v) for k, v in params.items()}
            out = orc.net_forward(p, m["verts"], m["mass"], m["evals"], m["evecs"], m["gradX"], m["gradY"], faces=m["faces"],
                                  outputs_at="faces", last_activation=lsm, keep_masks=masks)
            F.nll_loss(out, labels[i % n_sample]).backward()
            opt.step()
        for i in range(3):
            step(i)
        torch.cuda.synchronize()
        t0, n, v = time.perf_counter(), 0, 0
        while n < 30 and time.perf_counter() - t0 < 5.0:
            step(n)
            v += sizes[n % n_sample]
            n += 1
        torch.cuda.synchronize()
        return {"value": v / (time.perf_counter() - t0), "unit": "vertices/s", "kind": "port on the GPU (stock PyTorch-ROCm ops, no code of this library)",
                "sample": "%d train steps, one mesh per step, first %d meshes of the benchmark batch, fp32, same net/config" % (n, n_sample)}
    except Exception as e:      # noqa: BLE001
        return {"value": None, "unit": "vertices/s", "kind": "unavailable: %s" % repr(e)[:160]}


def parity_in_run(device):
    """Measured in THIS run, on this GPU, through the product path: the two C_width = 128 / K = 128 fixtures generated by the imported
    reference (tests/golden/make_golden.py) -- a one-block net with the faces head and the shipped human_seg_xyz_4x128 checkpoint
    (4 blocks, trained weights) -- forward rel-max and worst gradient rel-L2 against the reference's own fp32 outputs.  No oracle code is
    involved: the fixtures are arrays.  (The fp64-bracket margins of the large shapes are measured by the GPU test tier and written to
    gpurun_out/parity_margins_cuda.json; the round's copy is committed under profiles/.)"""
    import diffusion_net
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    # (the tolerances of tests/parity_cases.py: FWD_TOL / GRAD_TOL for synthetic weights; the trained-checkpoint fixture is judged by the fp64 bracket)
    out = {"tolerance_fwd_rel_max": 1e-5, "tolerance_grad_rel_l2": 2e-5, "trained_checkpoint_gradient_floor_inside_the_fp64_bracket": 2e-4, "cases": []}
    for name in ("faces_v500_c128_k128", "ckpt_human_seg_xyz_v600"):
        try:
            meta, params, inputs, masks, expect = helpers.load_golden(name)
            model = diffusion_net.layers.DiffusionNet(last_activation=helpers.activation_of(meta), **meta["ctor"])
            model.load_state_dict(params, strict=True)
            model.train(False)
            model.to(device)
            dv = lambda t: None if t is None else t.to(device)
            x = inputs["x_in"].to(device).requires_grad_(True)
            o = model(x, dv(inputs["mass"]), L=None, evals=dv(inputs["evals"]), evecs=dv(inputs["evecs"]), gradX=dv(inputs["gradX"]),
                      gradY=dv(inputs["gradY"]), edges=dv(inputs["edges"]), faces=dv(inputs["faces"]))
            (o * expect["loss_w"].to(device)).sum().backward()
            got = {"x_in": x.grad.cpu(), **{k: p.grad.cpu() for k, p in model.named_parameters()}}
            eg = {k: helpers.rel_l2(v, expect["grads"][k]) for k, v in got.items()}
            wk = max(eg, key=eg.get)
            case = {"fixture": name, "blocks": meta["ctor"].get("N_block", 4), "vertices": meta["V"],
                    "fwd_rel_max_vs_reference": helpers.rel_max(o.detach().cpu(), expect["out"]),
                    "worst_gradient_rel_l2_vs_reference": eg[wk], "worst_gradient": wk}
            if "out64" in expect:      # trained weights: the fp32 reference is itself ~1e-5 from the fp64 evaluation of the same module --
                o64, g64 = expect["out64"], expect["grads64"]          # the yard-stick is the distance to fp64, next to the reference's own
                case["fwd_rel_max_vs_reference_fp64"] = helpers.rel_max(o.detach().cpu().double(), o64)
                case["reference_fp32_fwd_rel_max_vs_reference_fp64"] = helpers.rel_max(expect["out"].double(), o64)
                ratios = {k: helpers.rel_l2(v.double(), g64[k]) / max(helpers.rel_l2(expect["grads"][k].double(), g64[k]), 1e-12) for k, v in got.items()}
                wr = max(ratios, key=ratios.get)
                case["worst_gradient_distance_to_fp64_over_reference_fp32s"] = ratios[wr]
                case["worst_gradient_vs_fp64"] = {"tensor": wr, "new": helpers.rel_l2(got[wr].double(), g64[wr]),
                                                  "reference_fp32": helpers.rel_l2(expect["grads"][wr].double(), g64[wr])}
                case["criterion"] = "distance to fp64 <= max(tolerance, 2 x the fp32 reference's own distance to fp64) (SURVEY 7)"
                case["note"] = ("the forward margin against fp64 depends on the summation order inside the MFMA: the host emulator build of the same "
                                "kernels (k-ordered fmaf chains) lands at 1.49e-5 from fp64 on this fixture -- beyond the fp32 reference's own 1.15e-5 -- "
                                "where the device measured 4.6e-6 in round 5; both pass only through the bracket, neither is within 1e-5 of the fp32 reference")
            out["cases"].append(case)
        except Exception as e:      # noqa: BLE001
            out["cases"].append({"fixture": name, "error": repr(e)[:200]})
    return out


def kernel_family_report(lib):
    """Per-KERNEL timing from the library's hipEvent brackets (this rank, timed region) and the roofline object of the kernel with the
    largest share of kernel time.  Since round 5 every bracket kind is one kernel as rocprofv3 names it (the round-4 `tngemm_kernel` bucket
    lumped the projection, the weight-gradient and the dA kernels: it out-weighed the actual dominant kernel) -- except the
    `rowgemm_kernel<*,N>` kinds (instantiations of one kernel template) and `small` (everything under ~30 us)."""
    fam = []
    buf = (ctypes.c_double * 4)()
    for k in range(16):
        if not lib.dn_prof_kind_name(k):     # kinds are numbered densely; an empty name ends the list
            break
        lib.dn_prof_read(k, buf)
        ms, n, fl, by = buf[0], buf[1], buf[2], buf[3]
        if n > 0:
            fam.append({"kernel": lib.dn_prof_kind_name(k).decode(), "ms_total": ms, "launches": int(n),
                        "avg_us": 1e3 * ms / n, "tflops": fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0,
                        "gbps": by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0,
                        "flops_per_launch": fl / n, "bytes_per_launch": by / n})
    if not fam:          # nothing went through the library's brackets (the timed region replayed graphs)
        return [], None
    dom = max((f for f in fam if f["kernel"] != "small"), key=lambda f: f["ms_total"], default=max(fam, key=lambda f: f["ms_total"]))
    # Binding roof of a family = the lower of the two roofs at its arithmetic intensity.  The GEMM families run on
    # split-bf16 MFMA (6 bf16 MFMAs per fp32 product: effective fp32 peak = 2.5 PF / 6); the sparse family is HBM-bound.
    def bind(f):
        # (the chained forward kernel runs on the 2-term fp16 split: 3 MFMAs per fp32 product)
        eff_peak = PEAK_MFMA_BF16_TFLOPS / 3.0 if "chain" in f["kernel"] else (
            PEAK_MFMA_BF16_TFLOPS / 6.0 if ("gemm" in f["kernel"] or "diffuse" in f["kernel"] or "backproject" in f["kernel"]) else PEAK_MFMA_F32_TFLOPS)
        ai = f["flops_per_launch"] / max(f["bytes_per_launch"], 1.0)
        ridge = eff_peak * 1e12 / (PEAK_HBM_GBPS * 1e9)
        if f["flops_per_launch"] > 0 and ai > ridge:
            return {"bound": "mfma", "achieved": f["tflops"], "peak": eff_peak, "unit": "TFLOP/s", "frac": f["tflops"] / eff_peak}
        return {"bound": "hbm", "achieved": f["gbps"], "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": f["gbps"] / PEAK_HBM_GBPS}
    roof = bind(dom)
    roof["traffic"] = None
    roof["arithmetic_intensity_flop_per_byte"] = dom["flops_per_launch"] / max(dom["bytes_per_launch"], 1.0)
    roof["effective_fp32_tflops"] = dom["tflops"]
    # HBM bytes per launch of that family from the committed FETCH_SIZE / WRITE_SIZE PMC passes (separate rocprofv3
    # --pmc runs of the same workload, gfx950 x2 read correction applied; tools/traffic_summary.py)
    try:
        tj = TRAFFIC_JSON if os.path.exists(os.path.join(ROOT, "profiles", TRAFFIC_JSON)) else "r05_traffic.json"
        tr = json.load(open(os.path.join(ROOT, "profiles", tj)))
        # (the PMC workload also runs the inference forward -- another instantiation of the same kernel, a fraction of the traffic: the member
        # with the largest traffic is the training-step kernel this line is about)
        ent = tr[dom["kernel"]]
        roof["traffic"] = max([m["hbm_bytes_per_launch"] for m in ent.get("members", {}).values()] or [ent["hbm_bytes_per_launch"]])
        roof["traffic_source"] = ("NOT measured in this run: read from profiles/%s -- separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; "
                                  "(2*FETCH_SIZE+WRITE_SIZE)*1024 B per launch, gfx950 read correction) over tools/microbench.py at this batch shape; "
                                  "algorithmic bytes per launch = %.4g" % (tj, dom["bytes_per_launch"]))
    except Exception:
        pass
    roof.update({"kernel": dom["kernel"], "avg_launch_us": dom["avg_us"], "launches": dom["launches"],
                 "share_of_kernel_time": dom["ms_total"] / sum(f["ms_total"] for f in fam)})

    return fam, roof


def run_other_config(args, device, lib, world, rank):
    """The other BASELINE.json configs through the same timing contract (1 GPU; they are parity-test shapes, reported for reference):
      cfg2  human_segmentation_original as the script runs it: ONE ~7k-vertex mesh per step through the reference-signature forward,
            operators moved to the device every step, torch Adam, F.nll_loss (human_segmentation_original.py:105-148)
      cfg3  classification_shrec11 shape: 64 ragged ~2k-vertex meshes per step, C_width=64 (the script's), K=128, global-mean pooling,
            30 classes, label-smoothing loss, packed batch
      cfg4  one 200 000-vertex mesh, C_width=K=256, inference (no_grad, eval) through the reference-signature forward"""
    import diffusion_net
    from diffusion_net import synthetic
    assert world == 1, "the alternative configs are single-GPU workloads"
    lsm = lambda t: F.log_softmax(t, dim=-1)
    torch.manual_seed(0)
    cfg = args.config
    if cfg == "cfg2":
        V, K, C = 7000, 128, 128
        meshes = [synthetic.make_mesh_operators(V + 17 * i, K, seed=i) for i in range(8)]
        labels = [torch.randint(0, 8, (m["faces"].shape[0],)) for m in meshes]
        model = diffusion_net.layers.DiffusionNet(3, 8, C_width=C, N_block=4, outputs_at="faces", dropout=True, last_activation=lsm).to(device)
        model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=0))
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        sizes = [m["verts"].shape[0] for m in meshes]
        if args.graph:
            # one captured step per mesh (operators device-resident, as the op cache keeps them anyway); per step: copy features + labels, replay
            from diffusion_net.batch import GatherPattern, MeshBatch
            from diffusion_net.dist import FlatParams
            from diffusion_net.graphs import GraphedTrainStep
            flat = FlatParams(model)
            opt = torch.optim.Adam([flat.master], lr=1e-3, capturable=True)
            gsteps = []
            for m, lab in zip(meshes, labels):
                mb_i = MeshBatch.from_operators([m["mass"]], [m["evals"]], [m["evecs"]], [m["gradX"]], [m["gradY"]], device=device)
                gsteps.append(GraphedTrainStep(model, flat, opt, mb_i, GatherPattern(m["faces"].to(device), m["verts"].shape[0]),
                                               m["verts"].to(device), lab.to(device)))

            def step(i):
                m, lab = meshes[i % 8], labels[i % 8]
                return gsteps[i % 8].step(m["verts"].to(device, non_blocking=True), lab.to(device, non_blocking=True)), sizes[i % 8]
        else:
            def step(i):
                m, lab = meshes[i % 8], labels[i % 8]
                d = {k: m[k].to(device) for k in ("verts", "faces", "mass", "evals", "evecs", "gradX", "gradY")}
                opt.zero_grad()
                preds = model(d["verts"], d["mass"], L=None, evals=d["evals"], evecs=d["evecs"], gradX=d["gradX"], gradY=d["gradY"], faces=d["faces"])
                loss = F.nll_loss(preds, lab.to(device))
                loss.backward()
                opt.step()
                return loss, sizes[i % 8]
        desc = ("HIP-graph replay of the human_segmentation_original step: one ~%d-vertex mesh per step, features and labels copied in, operators resident, "
                "C_width=128 K=128 N_block=4, dropout on (device-side seed), Adam" % V) if args.graph else (
                "unmodified human_segmentation_original train loop: one ~%d-vertex mesh per step through DiffusionNet.forward(x, mass, L, evals, evecs, "
                "gradX, gradY, faces), operators re-sent to the device every step (operator cache hits by content; forward and backward replayed from "
                "automatically captured HIP graphs: %s), C_width=128 K=128 N_block=4, dropout on, torch Adam + F.nll_loss" % (V, "on" if diffusion_net.autograph.enabled else "off"))
        Cw = C
    elif cfg == "cfg3":
        K, C, n = 128, 64, 64
        g = torch.Generator().manual_seed(3)
        sizes = [int(1500 + 1000 * torch.rand(1, generator=g).item()) for _ in range(n)]
        from diffusion_net.batch import MeshBatch
        ms = [synthetic.make_mesh_operators(v, K, seed=100 + i) for i, v in enumerate(sizes)]
        mb = MeshBatch.from_operators([m["mass"] for m in ms], [m["evals"] for m in ms], [m["evecs"] for m in ms], [m["gradX"] for m in ms],
                                      [m["gradY"] for m in ms], device=device)
        x = torch.cat([m["verts"] for m in ms], 0).to(device)
        lab = torch.randint(0, 30, (n,), device=device)
        model = diffusion_net.layers.DiffusionNet(3, 30, C_width=C, N_block=4, outputs_at="global_mean", dropout=False, last_activation=lsm).to(device)
        model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=0))
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        if args.graph:
            from diffusion_net.dist import FlatParams
            from diffusion_net.graphs import GraphedTrainStep
            flat = FlatParams(model)
            opt = torch.optim.Adam([flat.master], lr=1e-3, capturable=True)
            gs = GraphedTrainStep(model, flat, opt, mb, None, x, lab, smoothing=0.2)

        def step(i):
            if args.graph:
                return gs.step(), sum(sizes)
            opt.zero_grad()
            preds = model.forward_packed(x, mb)
            loss = diffusion_net.utils.label_smoothing_log_loss(preds, lab, 0.2)
            loss.backward()
            opt.step()
            return loss, sum(sizes)
        desc = ("classification_shrec11 shape: packed batch of %d ragged meshes (1500..2500 vertices, %d in total) per step, C_in=3 C_out=30 C_width=64 K=128 "
                "N_block=4 outputs_at=global_mean, label-smoothing loss 0.2, torch Adam%s" % (n, sum(sizes), ", step replayed from a captured HIP graph" if args.graph else ""))
        Cw = C
    else:
        V, K, C = 200000, 256, 256
        m = synthetic.make_mesh_operators(V, K, seed=4)
        d = {k: m[k].to(device) for k in ("verts", "mass", "evals", "evecs", "gradX", "gradY")}
        model = diffusion_net.layers.DiffusionNet(3, 16, C_width=C, N_block=4, dropout=True).to(device).eval()
        model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=1))

        def step(i):
            with torch.no_grad():
                out = model(d["verts"], d["mass"], evals=d["evals"], evecs=d["evecs"], gradX=d["gradX"], gradY=d["gradY"])
            return out.sum(), V
        desc = "inference (eval, no_grad) on one %d-vertex mesh through the reference-signature forward, C_in=3 C_out=16 C_width=256 K=256 N_block=4" % V
        Cw = C
    # cfg2: every one of the 8 meshes seen 4 times (automatic graph capture at the 3rd); cfg4 is above the capture threshold (device-bound)
    for i in range(max(args.warmup, 32 if cfg == "cfg2" else 1)):
        step(i)
    torch.cuda.synchronize()
    lib.dn_prof_reset()
    lib.dn_prof_enable(1)
    t0, verts = time.perf_counter(), 0
    for i in range(args.steps):
        loss, v = step(i)
        verts += v
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    lib.dn_prof_enable(0)
    assert torch.isfinite(loss).item()
    # a replayed graph bypasses the library's host-side event brackets (cfg2: the automatic capture of diffusion_net.autograph replays too)
    graphed = args.graph or (cfg == "cfg2" and diffusion_net.autograph.enabled and diffusion_net.autograph.stats["replays_fwd"] > 0)
    fam, roof = ([], None) if graphed else kernel_family_report(lib)
    print(json.dumps({
        "engine": _engine_note(),
        "metric": "vertices/sec %s, C_width=%d K=%d" % ("fwd" if cfg == "cfg4" else "fwd+bwd", Cw, K),
        "value": verts / elapsed, "unit": "vertices/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic", "config": {"workload": desc, "baseline_config": cfg, "parallelism": "dp1"},
        "roofline": roof, "kernel_families": fam}))


def _engine_note():
    from diffusion_net import _hip
    return ("split-bf16 MFMA only (library option f16=0)" if _hip.get_option("f16") == 0 else
            "row products (gradient features, MLP, input gradients, backward back-projection) on 2-term split-fp16 MFMA with producer-side "
            "power-of-two scales; projections, forward back-projection and all parameter-gradient sums on 3-term split-bf16 MFMA" +
            ("" if _hip.get_option("spectral_grad") == 0 else
             "; spectral-gradient forward (option spectral_grad=%d: %s): xd, gx, gy = [evecs | gradX evecs | gradY evecs] ys inside the chained forward "
             "kernel on the 2-term engine, gradX evecs / gradY evecs accumulated in fp64 once per mesh" %
             (_hip.get_option("spectral_grad"), "inference at every size, training up to 65536 rows" if _hip.get_option("spectral_grad") == 1 else "every size")))


def run_epoch_mode(args, device, lib, world, rank):
    """The headline train step over CHANGING batches (the static-batch replay is not what an epoch looks like -- the reference's
    loop visits a different mesh every step, human_segmentation_original.py:105-120): `--epoch N` packs N distinct batches of `--meshes`
    meshes each (drawn as sliding windows from a pool of meshes + N synthetic meshes, so that the operators, the vertex counts and every
    device pointer differ from batch to batch) and cycles them through diffusion_net.graphs.GraphedEpoch: one captured step per packed
    batch, one shared memory pool, one host call per step after a batch's first visit.  Same JSON contract; value = vertices of the timed
    steps / time."""
    import diffusion_net
    from diffusion_net import synthetic
    from diffusion_net.batch import GatherPattern, MeshBatch
    from diffusion_net.dist import FlatParams
    from diffusion_net.graphs import GraphedEpoch
    C_in, C_out = 3, 8
    n_b, n_m = args.epoch, args.meshes or 16
    verts = args.verts or 10000
    torch.manual_seed(0)
    model = diffusion_net.layers.DiffusionNet(C_in, C_out, C_width=args.cwidth, N_block=args.blocks, outputs_at="faces", dropout=True,
                                              last_activation=lambda t: F.log_softmax(t, dim=-1))
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=0))
    model.to(device).train()
    flat = FlatParams(model)
    try:
        opt = torch.optim.Adam([flat.master], lr=1e-3, capturable=True, fused=True)
    except (TypeError, RuntimeError):
        opt = torch.optim.Adam([flat.master], lr=1e-3, capturable=True)
    n_pool = n_m + n_b
    sizes = mesh_sizes(n_pool, verts, rank)
    pool = [synthetic.make_mesh_operators(v, args.keig, seed=7000 * rank + i) for i, v in enumerate(sizes)]
    stride = max(1, n_pool // n_b)
    batches = []
    for b in range(n_b):
        ms = [pool[(b * stride + j) % n_pool] for j in range(n_m)]
        mb = MeshBatch.from_operators([m["mass"] for m in ms], [m["evals"] for m in ms], [m["evecs"] for m in ms], [m["gradX"] for m in ms],
                                      [m["gradY"] for m in ms], device=device)
        offs, faces = 0, []
        for m in ms:
            faces.append(m["faces"] + offs)
            offs += m["verts"].shape[0]
        gather = GatherPattern(torch.cat(faces, 0).to(device), offs)
        x = torch.cat([m["verts"] for m in ms], 0).to(device)
        labels = torch.randint(0, C_out, (gather.n_out,), device=device)
        batches.append((mb, gather, x, labels, offs))
    ge = GraphedEpoch(model, flat, opt, all_reduce=False if world == 1 else "eager")

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    for i in range(max(args.warmup, n_b)):          # every batch visited (captured) at least once before the timed region
        ge.step(*batches[i % n_b][:4])
    fence()
    t0 = time.perf_counter()
    v = 0
    for i in range(args.steps):
        loss = ge.step(*batches[i % n_b][:4])
        v += batches[i % n_b][4]
    fence()
    elapsed = time.perf_counter() - t0
    assert torch.isfinite(loss).item()
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        vt = torch.tensor([v], device=device, dtype=torch.float64)
        dist.all_reduce(vt, op=dist.ReduceOp.SUM)
        v = float(vt.item())
    if rank == 0:
        print(json.dumps({
            "metric": "vertices/sec fwd+bwd, C_width=%d K=%d" % (args.cwidth, args.keig), "value": v / elapsed, "unit": "vertices/s",
            "n_gpus": world, "steps": args.steps, "warmup": max(args.warmup, n_b), "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "train step (fwd+NLL+bwd+Adam) cycling %d DISTINCT packed batches of %d meshes x ~%d vertices (sliding windows over a pool of %d "
                                   "synthetic meshes: operators, vertex counts %d..%d and every device pointer differ per batch), DiffusionNet C_in=3 C_out=8 "
                                   "C_width=%d K=%d N_block=%d outputs_at=faces dropout=on" % (n_b, n_m, verts, n_pool, min(b[4] for b in batches),
                                                                                             max(b[4] for b in batches), args.cwidth, args.keig, args.blocks),
                       "baseline_config": "headline", "parallelism": "dp%d" % world,
                       "step_mode": "HIP-graph replay over changing batches: one captured step per packed batch, shared memory pool "
                                    "(diffusion_net.graphs.GraphedEpoch: %s)" % ge.stats}}))
    if world > 1:
        dist.destroy_process_group()


def other_configs_brief(args):
    """Short runs of the other BASELINE.json configs, each in its own process (its own model, graphs and allocator state), summarised for the
    headline line's `configs` object.  cfg5 here is the single-GPU shard shape; its multi-GPU form is `--gpus N --config cfg5`."""
    import subprocess
    out = {}
    runs = (("cfg2", ["--config", "cfg2", "--steps", "40", "--warmup", "8"]),
            ("cfg2_graph", ["--config", "cfg2", "--graph", "--steps", "40", "--warmup", "8"]),
            ("cfg3", ["--config", "cfg3", "--graph", "--steps", "20", "--warmup", "3"]),
            ("cfg4", ["--config", "cfg4", "--steps", "5", "--warmup", "1"]),
            ("cfg5", ["--config", "cfg5", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-other-configs"]),
            ("epoch_mode", ["--epoch", "8", "--steps", "24", "--warmup", "8", "--no-cpu-baseline", "--no-other-configs"]))
    for name, extra in runs:
        t0 = time.perf_counter()
        try:
            lib_flags = [f for kv in args.lib_opt for f in ("--lib-opt", kv)]
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra + lib_flags, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[name] = {"error": (r.stderr or r.stdout)[-300:]}
                continue
            d = json.loads(line[-1])
            out[name] = {"value": d["value"], "unit": d["unit"], "metric": d["metric"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                         "workload": d["config"]["workload"], "wall_s": round(time.perf_counter() - t0, 1)}
        except Exception as e:      # noqa: BLE001
            out[name] = {"error": repr(e)[:300]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--meshes", type=int, default=None, help="meshes per GPU per step (default 16; cfg5: 8)")
    ap.add_argument("--verts", type=int, default=None, help="mean vertices per mesh (default 10000; cfg5: 15000)")
    ap.add_argument("--cwidth", type=int, default=128)
    ap.add_argument("--keig", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--streams", type=int, default=1, help="split the per-GPU batch into this many sub-batches run on separate HIP streams")
    ap.add_argument("--full", action="store_true", help="headline: after the timed steps also measure and report the roofline / kernel families, "
                                                        "the diffusion block, in-run parity, the all-reduce alone (N > 1), the CPU and "
                                                        "PyTorch-ROCm baselines and the other configs (off: only the timed steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="headline / cfg5: write what the last timed step computed (loss, "
                                                                         "log-probabilities, updated parameters, gradients) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU and PyTorch-ROCm baselines")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full, headline at 1 GPU: do not append the short runs of cfg2..cfg5 (`configs` object)")
    ap.add_argument("--graph", action="store_true", help="cfg2/cfg3: replay a captured HIP graph of the step (diffusion_net.graphs) instead of enqueueing ~150 launches per step "
                                                         "(the headline step is replayed from a graph by default; see --eager)")
    ap.add_argument("--graph-collectives", action="store_true", help="N > 1: capture the bucketed RCCL all-reduce inside the step graph instead of issuing one flat all-reduce from the host after the replay")
    ap.add_argument("--eager", action="store_true", help="headline: enqueue the ~190 launches of every step from the host instead of replaying the captured HIP graph")
    ap.add_argument("--epoch", type=int, default=0, help="headline: cycle this many DISTINCT packed batches (graph replay over changing batches: one captured step per "
                                                     "batch, diffusion_net.graphs.GraphedEpoch) instead of replaying one static batch")
    ap.add_argument("--lib-opt", action="append", default=[], metavar="NAME=VALUE",
                    help="tuning option of the library for this run (include/diffnet_hip.h: dn_set_option), e.g. chain=0, diffuse=0; repeatable")
    ap.add_argument("--config", default="headline", choices=["headline", "cfg2", "cfg3", "cfg4", "cfg5"],
                    help="headline: BASELINE metric workload (default, what the driver runs); cfg2/cfg3/cfg4: the other BASELINE.json configs, same JSON contract; "
                         "cfg5: the headline step at the rna_mesh_segmentation shape (8 meshes x ~15k vertices per GPU, 260 classes at the vertices; works with --gpus N)")
    args = ap.parse_args()
    if args.dump_outputs and (args.config not in ("headline", "cfg5") or args.epoch > 0):
        ap.error("--dump-outputs is implemented for the headline step (and cfg5), not for --config %s / --epoch" % args.config)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU of this node over RCCL, same arguments
        import socket
        import subprocess
        s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "--gpus %d but the launcher started %d ranks" % (args.gpus, world)
    if os.environ.get("DN_BENCH_LAUNCH_CHECK"):   # tests/test_dist_gloo.py: the launcher leg alone (runs without a GPU)
        print(json.dumps({"rank": rank, "local": local, "local_rank": local, "world": world, "master": os.environ.get("MASTER_ADDR")}), flush=True)
        return
    assert torch.cuda.is_available(), "bench.py needs a ROCm device (no CPU path)"
    # TEST HOOK (tests/test_gpu_parity.py on the 1-GPU boxes): every rank on GPU 0, collectives over gloo -- exercises the N-rank logic
    # (sharding, graph replay + host all-reduce, agreement flags, max-over-ranks timing) where N GPUs are not available; never a result
    shared_gpu = os.environ.get("DN_BENCH_TEST_SHARED_GPU") == "1"
    if shared_gpu:
        local = 0
    assert torch.cuda.device_count() >= (local + 1), "rank %d has no GPU (visible devices: %d)" % (rank, torch.cuda.device_count())
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
            assert dist.get_backend() == "nccl"
        assert dist.get_world_size() == args.gpus

    import diffusion_net
    from diffusion_net import _hip, synthetic
    from diffusion_net.dist import FlatParams
    for kv in args.lib_opt:                    # applied when the library is bound (and to every sub-run: they get the same flags)
        k_, v_ = kv.split("=", 1)
        _hip.default_options[k_] = int(v_)
    if _hip.default_options.get("spectral_grad") == 2:   # "always": k_eig = 256 batches carry the packed operands too (off by default: DESIGN.md)
        from diffusion_net import batch as _batch
        _batch.spectral_grad_wide = True
    if not os.path.exists(_hip.LIB_PATH):      # fresh checkout: compile the HIP sources once (rank 0), never a fallback
        if rank == 0:
            import __graft_entry__
            __graft_entry__.build()
        if world > 1:
            dist.barrier()
    lib = _hip.lib()

    if args.config not in ("headline", "cfg5"):
        return run_other_config(args, device, lib, world, rank)
    if args.epoch > 0:
        return run_epoch_mode(args, device, lib, world, rank)
    C_in, C_out = 3, 8
    at_faces = True
    if args.config == "cfg5":                  # rna_mesh_segmentation.py:69-75: C_out = 260 classes, outputs_at = 'vertices', ~15k-vertex meshes
        C_out, at_faces = 260, False
        args.meshes, args.verts = args.meshes or 8, args.verts or 15000
    args.meshes, args.verts = args.meshes or 16, args.verts or 10000
    torch.manual_seed(0)                       # identical replicas on every rank
    model = diffusion_net.layers.DiffusionNet(C_in, C_out, C_width=args.cwidth, N_block=args.blocks, outputs_at="faces" if at_faces else "vertices",
                                              dropout=True, last_activation=lambda t: F.log_softmax(t, dim=-1))   # as human_segmentation_original.py:69-75
    model.load_state_dict(synthetic.randomize_times(model.state_dict(), seed=0))
    model.to(device).train()
    nsub = max(1, min(args.streams, args.meshes))
    flat = FlatParams(model, direct_sinks=(nsub == 1))   # concurrent backward streams need autograd's ordered accumulation
    try:                                       # one fused update kernel over the flat parameter buffer
        opt = torch.optim.Adam([flat.master], lr=1e-3, fused=True)
    except (TypeError, RuntimeError):
        opt = torch.optim.Adam([flat.master], lr=1e-3)

    sizes = mesh_sizes(args.meshes, args.verts, rank)
    shard_note = None
    if args.config == "cfg5":
        # ONE ragged dataset for the whole job (the rna_mesh_segmentation shape: ~15k-vertex meshes, here 0.6..1.4 x --verts), split over the ranks
        # with the package's greedy longest-processing-time sharding (diffusion_net.dist.shard_by_cost; cost = vertices): the designed
        # multi-GPU path end to end.  Ranks hold different mesh counts; the imbalance is reported next to the rate.
        from diffusion_net.dist import shard_by_cost
        g = torch.Generator().manual_seed(4321)
        all_sizes = [int(args.verts * (0.6 + 0.8 * torch.rand(1, generator=g).item())) for _ in range(args.meshes * world)]
        mine = shard_by_cost(all_sizes, world)[rank]
        sizes = [all_sizes[i] for i in mine]
        per_rank = [sum(all_sizes[i] for i in part) for part in shard_by_cost(all_sizes, world)]
        shard_note = {"dataset_meshes": len(all_sizes), "dataset_vertices": sum(all_sizes), "meshes_per_rank": [len(p_) for p_ in shard_by_cost(all_sizes, world)],
                      "vertices_per_rank": per_rank, "load_imbalance_max_over_mean": max(per_rank) / (sum(per_rank) / len(per_rank))}
        args.meshes = len(sizes)
    subs = []
    for j in range(nsub):
        sub_sizes = sizes[j::nsub]
        _, mb_j, gather_j, x_j = build_batch(sub_sizes, args.keig, device, seed0=1000 * rank + 100 * j)
        if not at_faces:
            gather_j = None
        labels_j = torch.randint(0, C_out, (gather_j.n_out if at_faces else sum(sub_sizes),), device=device)
        subs.append((mb_j, gather_j, x_j, labels_j, sum(sub_sizes)))
    mb = subs[0][0]
    v_step = sum(sizes)
    streams = [torch.cuda.Stream(device) for _ in range(nsub)] if nsub > 1 else [None]

    gs, step_mode = None, "eager launches"
    if not args.eager and nsub == 1:
        # the whole step (zero grads + fwd + loss + bwd [+ bucketed RCCL all-reduce] + Adam) captured once into a HIP graph and replayed:
        # one host call per step instead of ~190 launches (the host cannot enqueue them as fast as the GPU retires them)
        from diffusion_net.graphs import GraphedTrainStep
        ok, why = 1, ""
        try:
            try:
                opt_g = torch.optim.Adam([flat.master], lr=1e-3, capturable=True, fused=True)
            except (TypeError, RuntimeError):
                opt_g = torch.optim.Adam([flat.master], lr=1e-3, capturable=True)
            mb_j, gather_j, x_j, labels_j, _ = subs[0]
            # N > 1: forward + backward from the graph, then one flat RCCL all-reduce and the update from the host (--graph-collectives
            # captures the bucketed, overlapped all-reduce too; never needed for 1.85 MB of gradients)
            ar_mode = False if world == 1 else ("captured" if args.graph_collectives else "eager")
            gs = GraphedTrainStep(model, flat, opt_g, mb_j, gather_j, x_j, labels_j, all_reduce=ar_mode)
            torch.cuda.synchronize()
        except Exception as e:                 # never silently: the mode is reported in the bench line
            ok, why = 0, repr(e)[:200]
        try:
            if not ok:
                torch.cuda.synchronize()       # (a capture that died half-way can leave the stream unusable: found out here, not later)
            if world > 1:                      # all ranks replay, or none does
                t = torch.tensor([ok], device=device, dtype=torch.int32)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                ok = int(t.item())
        except Exception as e2:
            raise RuntimeError("HIP-graph capture of the step failed (%s) and the device could not be used afterwards (%s): "
                               "re-run with --eager" % (why, repr(e2)[:200]))
        if ok:
            opt, step_mode = opt_g, ("HIP-graph replay" if world == 1 else ("HIP-graph replay incl. the bucketed RCCL all-reduce" if args.graph_collectives
                                                                         else "HIP-graph replay of forward+backward, then one flat RCCL all-reduce and Adam from the host"))
        else:
            if gs is not None:
                gs.release()
            for blk in model.blocks:
                blk._graph_seed = None
            gs, step_mode = None, "eager launches (graph capture failed: %s)" % why

    last_preds = []                            # eager steps: the log-probabilities of the last step (a graph keeps its own: gs.preds)

    def step():
        if gs is not None:
            return gs.step()
        flat.zero_grad()
        if nsub == 1:
            mb_j, gather_j, x_j, labels_j, _ = subs[0]
            preds, loss = model.forward_packed_loss(x_j, mb_j, gather_j, labels_j)     # per-face log-softmax + NLL: one kernel each way
            last_preds[:] = [preds]
            loss.backward()
        else:
            # sub-batches on separate streams: the store phase of one overlaps the MFMA phase of the other;
            # gradients of all sub-batches accumulate into the same flat bucket (mean over the whole batch)
            cur = torch.cuda.current_stream(device)
            losses = []
            last_preds.clear()
            for st, (mb_j, gather_j, x_j, labels_j, v_j) in zip(streams, subs):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    preds_j, loss_j = model.forward_packed_loss(x_j, mb_j, gather_j, labels_j)
                    last_preds.append(preds_j)
                    losses.append(loss_j * (1.0 / nsub))
            for st, l in zip(streams, losses):
                with torch.cuda.stream(st):
                    l.backward()
            for st in streams:
                cur.wait_stream(st)
            loss = losses[0]
        flat.all_reduce_mean()
        opt.step()
        return loss

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    lib.dn_prof_reset()
    lib.dn_prof_enable(1 if args.full else 0)  # --full: the library's event brackets (eager launches only) feed kernel_families
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    fence()
    elapsed = time.perf_counter() - t0
    lib.dn_prof_enable(0)
    if args.dump_outputs and rank == 0:        # before anything else runs on the model: the last timed step's results as a caller gets them
        dump_outputs(args.dump_outputs, {"loss": loss.reshape(1), "log_probs": gs.preds if gs is not None else torch.cat(last_preds, 0),
                                         "params": flat.master, "grads": flat.grad})
    multi, v_all = None, float(v_step)
    if world > 1:
        mine = torch.tensor([elapsed], device=device, dtype=torch.float64)
        t = mine.clone()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        vt = torch.tensor([v_step], device=device, dtype=torch.float64)
        dist.all_reduce(vt, op=dist.ReduceOp.SUM)
        v_all = float(vt.item())
    if world > 1 and args.full:
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)                       # every rank's own clock over the same K steps: a straggler shows here, not only in the MAX
        # the gradient all-reduce by itself (outside the timed region): the flat bucket as the step sends it, K times between two fences --
        # so that the first real N-GPU run says how much of its step is the collective and how much is the ranks waiting for each other
        fence()
        ta = time.perf_counter()
        for _ in range(max(args.steps, 5)):
            flat.all_reduce_mean()
        fence()
        ar_ms = 1e3 * (time.perf_counter() - ta) / max(args.steps, 5)
        flat.zero_grad()
        multi = {"per_rank_ms_per_step": [1e3 * float(e.item()) / args.steps for e in every], "max_over_ranks_ms_per_step": 1e3 * elapsed / args.steps,
                 "all_reduce_alone_ms": ar_ms, "all_reduce_bytes": int(flat.grad.numel() * 4),
                 "all_reduce_in_step": "host call after the replayed graph (no overlap)" if (gs is not None and not args.graph_collectives)
                                       else ("captured with the step, per-block buckets overlapped with the backward" if gs is not None else
                                             "per-block buckets launched from inside backward (eager)"),
                 "backend": dist.get_backend()}
    assert torch.isfinite(loss).item()

    Cw, K = args.cwidth, args.keig
    fam, roof, diff = [], None, None
    if args.full:
        eager_ms = None
        if gs is not None:      # the library's per-launch event brackets are host-side: time the same launches in a short eager pass
            lib.dn_prof_reset()
            lib.dn_prof_enable(1)
            te = time.perf_counter()
            for _ in range(min(args.steps, 5)):
                gs._body()
                gs._tail()
            fence()
            eager_ms = 1e3 * (time.perf_counter() - te) / min(args.steps, 5)
            lib.dn_prof_enable(0)
        fam, roof = kernel_family_report(lib)
        if roof is not None:
            fam_ms = sum(f["ms_total"] for f in fam) / (min(args.steps, 5) if gs is not None else args.steps)
            roof["timing"] = ("HIP events around every launch of %d eager steps run right after the timed graph replays (the event brackets are "
                              "host-side; a replayed graph bypasses them); profiles/ holds the rocprofv3 kernel trace of the replays themselves"
                              % min(args.steps, 5)) if gs is not None else "HIP events around every launch of the timed steps"
            # the brackets inflate: event records sit between the launches and the eager pass has host gaps the replay does not
            roof["families_ms_per_step"] = fam_ms
            roof["bracket_inflation_vs_timed_step"] = fam_ms / (1e3 * elapsed / args.steps)
            # real inter-kernel idle of the TIMED (replayed) step = step time - sum of kernel time.  The sum here is the library's own kernels from the
            # bracketed eager pass (torch's fill / Adam kernels, ~0.1 ms, are not bracketed; a bracket also counts the launch ramp), so the
            # difference is an upper bound of the idle only when positive; rocprofv3's per-kernel durations of the replays are the reference
            # (profiles/r0N_step_kernels.txt: the profiler itself inserts ~10 us between kernels, which the unprofiled replay does not have)
            roof["timed_step_ms_minus_bracketed_kernel_ms"] = 1e3 * elapsed / args.steps - fam_ms
            if eager_ms is not None:
                roof["eager_pass_ms_per_step"] = eager_ms

        # ---- diffusion block (to_basis + exp(-lambda t) + from_basis) on the same batch: HBM GB/s of BASELINE.json
        from diffusion_net import ops
        v_sub0 = subs[0][4]
        sizes = sizes[0::nsub]
        tt = torch.full((Cw,), 0.05, device=device)
        bytes_diff = sum(4.0 * (v * (2 * Cw + 2 * K + 1) + 2 * K * Cw + K + Cw) for v in sizes)
        flops_diff = sum(4.0 * v * K * Cw for v in sizes)

        def time_diffusion(n_rot):
            # n_rot input buffers touched in turn (the eigenbasis itself is one 81 MB array: it is re-read from HBM only when the inputs and
            # outputs streaming past it evict it from the 256 MiB Infinity Cache, as in the network)
            xs_ = [torch.randn(v_sub0, Cw, device=device) for _ in range(n_rot)]
            with torch.no_grad():
                for i in range(3):
                    ops.DiffusionFn.apply(xs_[i % n_rot], tt, mb)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                reps = 24
                keep = []
                for i in range(reps):
                    keep.append(ops.DiffusionFn.apply(xs_[i % n_rot], tt, mb))
                    if len(keep) > n_rot:
                        keep.pop(0)
                e1.record()
                torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps
        t_diff = time_diffusion(8)        # 8 inputs + 8 live outputs x 81 MB = 1.3 GB in rotation: HBM
        t_diff_cached = time_diffusion(1)

        def time_diffusion_bwd(n_rot):
            # the gradient of the same operator (dn_diffusion_bwd_f32: d_x = add + M Phi (coef * Phi^T d_xd), d_time), called as ops.DiffusionFn.backward calls it
            Lb = _hip.lib()
            gs_ = [torch.randn(v_sub0, Cw, device=device) for _ in range(n_rot)]
            adds = [torch.randn(v_sub0, Cw, device=device) for _ in range(n_rot)]
            outs = [torch.empty(v_sub0, Cw, device=device) for _ in range(n_rot)]
            xs_sp = torch.randn(mb.n_mesh, K, Cw, device=device)
            d_t = torch.empty(Cw, device=device)
            nws = Lb.dn_diffusion_workspace_bytes(mb.ref(), Cw)
            ws_ = torch.empty(nws + 4096, dtype=torch.uint8, device=device)
            st_ = torch.cuda.current_stream(device).cuda_stream

            def call(i):
                _hip.check(Lb.dn_diffusion_bwd_f32(mb.ref(), gs_[i % n_rot].data_ptr(), xs_sp.data_ptr(), tt.data_ptr(), Cw, adds[i % n_rot].data_ptr(),
                                                   outs[i % n_rot].data_ptr(), d_t.data_ptr(), ws_.data_ptr(), nws, st_), "dn_diffusion_bwd_f32")
            for i in range(3):
                call(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(24):
                call(i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / 24
        t_dbwd = time_diffusion_bwd(6)     # 6 x (d_xd, addend, d_x) x 81 MB = 1.5 GB in rotation
        bytes_dbwd = sum(4.0 * (v * (3 * Cw + 2 * K + 1) + 3 * K * Cw + K + Cw) for v in sizes)   # read d_xd, Phi twice, the addend, mass; write d_x; 3 x (K, C)
        diff = {"ms": t_diff * 1e3, "gbps": bytes_diff / t_diff / 1e9, "frac_hbm_8TBs": bytes_diff / t_diff / 1e9 / PEAK_HBM_GBPS,
                "frac_of_measured_copy_6p3TBs": bytes_diff / t_diff / 1e9 / 6300.0,
                "buffers": "8 rotating input / output sets (1.3 GB): operands come from HBM as inside the network; one re-used set (Infinity-Cache assisted): "
                           "%.3f ms = %.3f of 8 TB/s" % (t_diff_cached * 1e3, bytes_diff / t_diff_cached / 1e9 / PEAK_HBM_GBPS),
                "copy_calibration": "hand-written float4 nontemporal copy on 2 GiB of rotating buffers: 6.2-6.36 TB/s = 0.79 of 8 TB/s; hipMemcpy D2D 5.3 TB/s "
                                    "(tools/kbench --ops copyk, profiles/r03_copy_calibration.txt)",
                "backward": {"ms": t_dbwd * 1e3, "gbps": bytes_dbwd / t_dbwd / 1e9, "frac_hbm_8TBs": bytes_dbwd / t_dbwd / 1e9 / PEAK_HBM_GBPS,
                             "what": "dn_diffusion_bwd_f32 with an addend (the block's residual gradient), 6 rotating operand sets; algorithmic bytes "
                                     "4 [V (3C + 2K + 1) + 3KC + K + C] per mesh"},
                "launches": "projection (split-V, k-major bf16 planes) + per-mesh partial sum with exp(-lambda t) + direct back-projection (dn_diffuse.hip: backproject_kernel)"
                            if _hip.get_option("diffuse") == 2 else ("one persistent launch (dn_diffuse.hip: diffuse_kernel)" if _hip.get_option("diffuse") == 1 else
                                                                      "projection + per-mesh partial sum + wave-specialised row GEMM"),
                "tflops": flops_diff / t_diff / 1e12, "frac_mfma_f32": flops_diff / t_diff / 1e12 / PEAK_MFMA_F32_TFLOPS,
                "frac_mfma_bf16x3": flops_diff / t_diff / 1e12 / (PEAK_MFMA_BF16_TFLOPS / 6.0),
                "note": "arithmetic intensity KC/(2(K+C)) = %.0f flop/B; ridge 19.7 (f32 MFMA) / 52 (split-bf16 MFMA, used) -> HBM-bound" % (K * Cw / (2.0 * (K + Cw)))}

    if rank == 0:
        res = {
            "metric": "vertices/sec fwd+bwd, C_width=%d K=%d" % (Cw, K),
            "value": v_all * args.steps / elapsed, "unit": "vertices/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "arithmetic": "fp32 storage, accumulation and epilogues; dense products on split MFMA with fp32-level accuracy: " + _engine_note() +
                          (" (measured in this run against the reference's own outputs: see \"parity\")" if args.full and world == 1 else ""),
            "config": {"workload": "train step (fwd+NLL+bwd+Adam%s) on a ragged batch of %d meshes x ~%d vertices per GPU, "
                                   "DiffusionNet C_in=3 C_out=%d C_width=%d K=%d N_block=%d outputs_at=%s dropout=on"
                                   % ("+RCCL all-reduce" if world > 1 else "", args.meshes, args.verts, C_out, Cw, K, args.blocks, "faces" if at_faces else "vertices"),
                       "baseline_config": args.config, "meshes_per_gpu": args.meshes, "verts_per_gpu_step": v_step, "parallelism": "dp%d" % world,
                       "streams_per_gpu": nsub, "step_mode": step_mode, **({"sharding": shard_note} if shard_note else {}),
                       **({"TEST_ONLY": "all ranks share GPU 0, gloo collectives (DN_BENCH_TEST_SHARED_GPU)"} if shared_gpu else {})},
        }
        if args.full:
            res.update({"roofline": roof, "kernel_families": fam, "diffusion_block": diff})
        if multi is not None:
            res["multi_gpu"] = multi
        if args.full and world == 1:
            res["parity"] = parity_in_run(device)
        if args.full and not args.no_cpu_baseline and world == 1 and args.config == "headline":   # reported at N = 1 only (the other ranks would sit idle behind it)
            res["cpu_baseline"] = cpu_baseline(args, C_out, mesh_sizes(args.meshes, args.verts, 0))
            res["torch_rocm_baseline"] = torch_rocm_baseline(args, C_out, mesh_sizes(args.meshes, args.verts, 0), device)
        if args.full and world == 1 and args.config == "headline" and not args.no_other_configs:
            del gs, model, flat, subs, mb            # hand the GPU's memory back before the other configs' processes start
            torch.cuda.empty_cache()
            res["configs"] = other_configs_brief(args)
            em = res["configs"].pop("epoch_mode", None)
            if em is not None:        # the same step over 8 distinct packed batches (one captured graph per batch), next to the static-batch replay
                if "value" in em:
                    em["ratio_to_static_batch_replay"] = em["value"] / res["value"]
                res["epoch_mode"] = em
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

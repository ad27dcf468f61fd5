"""Golden vectors for ``diffusion_net.fmaps`` from the *reference itself* (dev container only; needs /root/reference): seeded inputs and the
outputs of the reference experiment's own ``compute_correspondence`` (experiments/functional_correspondence/fmaps_model.py) in fp32 and in
fp64, and from fp64 autograd the gradients of mean((C - C_gt)^2) with respect to both feature tensors.  (The file carries the ``geom_``
prefix of the fixtures of single functions: every other .npz in this folder is taken for a whole-net golden case.)

Inputs: bases with Phi^T M Phi = I (a QR factor scaled by mass^-1/2); eigenvalues sorted in [0, 100], the first exactly 0 on both shapes
(so D_0 has a zero and row 0 of the map rests on G), the others on two interleaved jittered grids, so that no two eigenvalues of the two
shapes come closer than a quarter of the grid step and the K systems stay well conditioned; lam = 1e-3.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fmap_golden.py            # writes geom_fmap_ref.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fmap_golden.py --check    # regenerates and compares with the committed file
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

LAM = 1e-3
# name: (V, K, F, rank of the features (0: full), seed)
CASES = {
    "k1_f1": (70, 1, 1, 0, 31),
    "k5_f3": (70, 5, 3, 0, 32),
    "k30_f128": (40, 30, 128, 0, 33),
    "k30_f16": (40, 30, 16, 0, 34),          # F < K: G is singular
    "k30_f128_rank8": (40, 30, 128, 8, 35),
    "k31_f40": (40, 31, 40, 0, 36),
    "k64_f70": (80, 64, 70, 0, 37),
    "k65_f20": (80, 65, 20, 0, 38),          # past the kernel's K: torch route
}


def make_inputs(V, K, F, rank, seed):
    """-> dict of fp32 arrays: feat_[xy] [V, F], mass_[xy] [V], evecs_[xy] [V, K], evals_[xy] [K], c_gt [K, K]."""
    rs = np.random.RandomState(seed)
    out = {}
    for s, shift in (("x", 0.0), ("y", 0.5)):
        mass = rs.uniform(0.5, 1.5, V) / V
        q, _ = np.linalg.qr(rs.randn(V, K))
        out["mass_" + s] = mass.astype(np.float32)
        out["evecs_" + s] = (q / np.sqrt(mass)[:, None]).astype(np.float32)
        evals = 100.0 * (np.arange(K) + shift + 0.25 * rs.uniform(0.0, 1.0, K)) / K
        evals[0] = 0.0
        out["evals_" + s] = evals.astype(np.float32)
        feat = rs.randn(V, rank) @ rs.randn(rank, F) / np.sqrt(rank) if rank else rs.randn(V, F)
        out["feat_" + s] = feat.astype(np.float32)
    out["c_gt"] = rs.randn(K, K).astype(np.float32)
    return out


def generate():
    import_reference()
    sys.path.insert(0, "/root/reference/experiments/functional_correspondence")
    import fmaps_model
    sys.path.pop(0)
    assert fmaps_model.__file__.startswith("/root/reference"), fmaps_model.__file__
    out = {"cases": np.array(sorted(CASES)), "lam": np.array(LAM, dtype=np.float64)}
    for name, (V, K, F, rank, seed) in CASES.items():
        inp = make_inputs(V, K, F, rank, seed)
        for key, v in inp.items():
            out[name + "/" + key] = v
        res = {}
        for dt in (torch.float32, torch.float64):
            t = {key: torch.from_numpy(v).to(dt) for key, v in inp.items()}
            fx, fy = t["feat_x"].requires_grad_(True), t["feat_y"].requires_grad_(True)
            trans = [t["evecs_" + s].t() @ torch.diag(t["mass_" + s]) for s in "xy"]       # fmaps_model.py:79
            C = fmaps_model.compute_correspondence(fx, fy, t["evals_x"], t["evals_y"], trans[0], trans[1], lambda_param=LAM)
            assert tuple(C.shape) == (1, K, K)
            res[dt] = C.detach()[0].numpy()
            if dt == torch.float64:
                ((C[0] - t["c_gt"]) ** 2).mean().backward()
                out[name + "/grad_feat_x_f64"], out[name + "/grad_feat_y_f64"] = fx.grad.numpy(), fy.grad.numpy()
        out[name + "/C_f32"], out[name + "/C_f64"] = res[torch.float32], res[torch.float64]
    return out


if __name__ == "__main__":
    out = generate()
    path = os.path.join(HERE, "geom_fmap_ref.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key, v in out.items():
            assert old[key].dtype == v.dtype and np.array_equal(old[key], v), key
        print("geom_fmap_ref.npz regenerates bit-exactly (%d arrays)" % len(out))
    else:
        np.savez_compressed(path, **out)
        print("wrote geom_fmap_ref.npz (%d bytes)" % os.path.getsize(path), {key: getattr(v, "shape", None) for key, v in out.items() if "/C_f64" in key})

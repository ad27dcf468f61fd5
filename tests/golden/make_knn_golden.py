"""Golden vectors for ``diffusion_net.geometry.find_knn`` from the *reference itself* (dev container only; needs /root/reference):
seeded inputs and the outputs of the reference's own ``find_knn`` for ``method='brute'`` and ``method='cpu_kd'``.  (The file carries the
``geom_`` prefix of the fixtures of single geometry functions: every other .npz in this folder is taken for a whole-net golden case.)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_knn_golden.py            # writes geom_knn_ref.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_knn_golden.py --check    # regenerates and compares with the committed file
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

# name: (N, M, D, k, largest, omit_diagonal, methods, seed)
CASES = {
    "d30_k1": (120, 90, 30, 1, False, False, ("brute", "cpu_kd"), 11),
    "d30_k8": (120, 90, 30, 8, False, False, ("brute", "cpu_kd"), 11),
    "d3_k30_omit": (120, 120, 3, 30, False, True, ("brute", "cpu_kd"), 12),
    "d30_k3_largest": (120, 90, 30, 3, True, False, ("brute",), 13),
}


def generate():
    ref = import_reference()
    out = {"cases": np.array(sorted(CASES))}
    for name, (N, M, D, k, largest, omit, methods, seed) in CASES.items():
        rs = np.random.RandomState(seed)
        src = rs.randn(N, D).astype(np.float32)
        tgt = src.copy() if omit else rs.randn(M, D).astype(np.float32)
        out[name + "/src"], out[name + "/tgt"] = src, tgt
        out[name + "/k_largest_omit"] = np.array([k, int(largest), int(omit)], dtype=np.int64)
        for method in methods:
            vals, inds = ref.geometry.find_knn(torch.from_numpy(src), torch.from_numpy(tgt), k, largest=largest, omit_diagonal=omit,
                                               method=method)
            out["%s/%s_values" % (name, method)] = vals.numpy()
            out["%s/%s_indices" % (name, method)] = inds.numpy()
    return out


if __name__ == "__main__":
    out = generate()
    path = os.path.join(HERE, "geom_knn_ref.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key, v in out.items():
            assert old[key].dtype == v.dtype and np.array_equal(old[key], v), key
        print("geom_knn_ref.npz regenerates bit-exactly (%d arrays)" % len(out))
    else:
        np.savez_compressed(path, **out)
        print("wrote geom_knn_ref.npz", {key: getattr(v, "shape", None) for key, v in out.items()})

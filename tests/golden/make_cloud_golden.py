"""Golden vectors for the point-cloud operators from the *reference itself* (development machine only: needs the reference checkout
that make_golden.import_reference finds): seeded clouds and the outputs of the reference's own ``vertex_normals``, ``build_tangent_frames`` and ``build_grad_point_cloud`` -- twice per case: as the
reference runs (fp32 points: ``ref32/``) and on the same points in fp64 (``ref64/``: the truth the kernel tests compare with).  The file also
records how far the reference's fp32 run is from its fp64 run (``dev_normals``: normals up to sign, largest component difference;
``dev_grad``: gradient entries, as a share of the largest entry of their row), which is the yardstick of the host-route parity test.
(The file carries the ``geom_`` prefix of the fixtures of single geometry functions: every other .npz here is a whole-net golden case.)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cloud_golden.py            # writes geom_cloud_ref.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cloud_golden.py --check    # regenerates and compares with the committed file
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

# name: (N, k, seed, axes, noise)
CASES = {
    "sphere300_k30": (300, 30, 3, (1.0, 1.0, 1.0), 0.0),
    "ellipsoid64_k30_noise": (64, 30, 3, (1.0, 0.7, 0.5), 0.01),
    "sphere100_k3": (100, 3, 3, (1.0, 1.0, 1.0), 0.0),
}


def sample(N, seed, axes=(1.0, 1.0, 1.0), noise=0.0):
    """N points of the ellipsoid with these axes (directions uniform on the sphere), optional Gaussian noise, rounded to fp32."""
    rs = np.random.RandomState(seed)
    p = rs.randn(N, 3)
    p = p / np.linalg.norm(p, axis=1, keepdims=True) * np.asarray(axes)
    if noise:
        p = p + noise * rs.randn(N, 3)
    return p.astype(np.float32)


def run_reference(ref, pts, k):
    """The reference's three functions on these points, in the dtype of ``pts``."""
    verts = torch.from_numpy(pts)
    faces = torch.zeros(0, 3, dtype=torch.int64)
    normals = ref.geometry.vertex_normals(verts, faces, n_neighbors_cloud=k)
    frames = ref.geometry.build_tangent_frames(verts, faces, normals=normals)
    grad = ref.geometry.build_grad_point_cloud(verts, frames, n_neighbors_cloud=k).tocsc()
    grad.sort_indices()
    _, nbr = ref.geometry.find_knn(verts, verts, k, omit_diagonal=True, method="cpu_kd")
    assert normals.dtype == verts.dtype and frames.dtype == verts.dtype
    return dict(normals=normals.numpy(), frames=frames.numpy(), nbr=nbr.numpy().astype(np.int64), grad_data=grad.data.astype(np.complex128),
                grad_indices=grad.indices.astype(np.int32), grad_indptr=grad.indptr.astype(np.int32))


def generate():
    ref = import_reference()
    out = {"cases": np.array(sorted(CASES))}
    for name, (N, k, seed, axes, noise) in CASES.items():
        pts = sample(N, seed, axes, noise)
        r32, r64 = run_reference(ref, pts, k), run_reference(ref, pts.astype(np.float64), k)
        assert np.array_equal(np.sort(r32["nbr"], axis=1), np.sort(r64["nbr"], axis=1)), name
        assert np.array_equal(r32["grad_indices"], r64["grad_indices"]) and np.array_equal(r32["grad_indptr"], r64["grad_indptr"]), name
        out[name + "/pts"], out[name + "/k"] = pts, np.array(k, dtype=np.int64)
        for tag, r in (("ref32", r32), ("ref64", r64)):
            for key, v in r.items():
                out["%s/%s/%s" % (name, tag, key)] = v
        s = np.sign(np.einsum("ij,ij->i", r32["normals"].astype(np.float64), r64["normals"]))
        out[name + "/dev_normals"] = np.array(np.abs(s[:, None] * r32["normals"] - r64["normals"]).max())
        # CSC of an [N, N] matrix: entry e lies in row grad_indices[e]; the Y part flips with the normal
        rows = r64["grad_indices"]
        d32 = r32["grad_data"].real + 1j * s[rows] * r32["grad_data"].imag
        top = np.zeros(N)
        np.maximum.at(top, rows, np.maximum(np.abs(r64["grad_data"].real), np.abs(r64["grad_data"].imag)))
        diff = np.maximum(np.abs(d32.real - r64["grad_data"].real), np.abs(d32.imag - r64["grad_data"].imag))
        out[name + "/dev_grad"] = np.array((diff / top[rows]).max())
    return out


if __name__ == "__main__":
    out = generate()
    path = os.path.join(HERE, "geom_cloud_ref.npz")
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(out), (sorted(old.files), sorted(out))
        for key, v in out.items():
            assert old[key].dtype == v.dtype and np.array_equal(old[key], v), key
        print("geom_cloud_ref.npz regenerates bit-exactly (%d arrays)" % len(out))
    else:
        np.savez_compressed(path, **out)
        print("wrote geom_cloud_ref.npz", {key: (getattr(v, "shape", None) if v.ndim else v.item()) for key, v in out.items() if key != "cases"})

"""CPU tier: the host routes of the point-cloud operators (``vertex_normals``, ``build_tangent_frames``, ``build_grad_point_cloud``,
``cloud_operators`` on host tensors) against the reference's recorded outputs (tests/golden/geom_cloud_ref.npz), and the point-cloud branch
of ``compute_operators`` / ``get_operators``."""
import inspect
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cloud_cases
import diffusion_net
import helpers
from diffusion_net import geometry, precompute

NO_FACES = torch.zeros(0, 3, dtype=torch.long)


def test_the_reference_names_exist_with_its_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(geometry.neighborhood_normal) == ["points"]
    assert sig(geometry.vertex_normals) == ["verts", "faces", "n_neighbors_cloud"]
    assert sig(geometry.build_tangent_frames) == ["verts", "faces", "normals"]
    assert sig(geometry.build_grad_point_cloud) == ["verts", "frames", "n_neighbors_cloud"]
    assert sig(geometry.cloud_operators) == ["verts", "n_neighbors_cloud", "normals"]
    assert inspect.signature(geometry.vertex_normals).parameters["n_neighbors_cloud"].default == 30
    assert sig(geometry.compute_operators) == ["verts", "faces", "k_eig", "normals", "laplacian"]
    assert inspect.signature(geometry.compute_operators).parameters["laplacian"].kind is inspect.Parameter.KEYWORD_ONLY
    from diffusion_net import _hip, ops
    assert "dn_cloud_operators_f32" in _hip.EXPORTED_SYMBOLS and callable(ops.cloud_operators)


def _grad_dev(got, ref, s):
    """Largest difference of the entries of two complex operators, as a share of the largest entry of their row of ``ref``; ``s``: the sign
    of the normal of ``got`` relative to ``ref`` per row (the Y part flips with it)."""
    S = sp.diags(s)
    worst = 0.0
    for a, b in ((sp.csr_matrix(got.real), sp.csr_matrix(ref.real)), (S @ sp.csr_matrix(got.imag), sp.csr_matrix(ref.imag))):
        top = np.maximum(cloud_cases._row_top(sp.csr_matrix(ref.real)), cloud_cases._row_top(sp.csr_matrix(ref.imag)))
        worst = max(worst, float((cloud_cases._row_top(sp.csr_matrix(a - b)) / top).max()))
    return worst


@pytest.mark.parametrize("name", sorted(cloud_cases.golden()))
def test_host_fp32_route_matches_the_reference_as_it_runs(name):
    """Both sides are fp32 LAPACK calls, possibly of different builds: entries within 4 x the distance of the reference's own fp32 run from
    its fp64 run (recorded in the fixture).  Normals up to sign."""
    pts, k, _, ref32, dev_normals, dev_grad = cloud_cases.golden()[name]
    verts = torch.from_numpy(pts)
    normals = geometry.vertex_normals(verts, NO_FACES, n_neighbors_cloud=k)
    assert normals.dtype == torch.float32 and tuple(normals.shape) == (len(pts), 3)
    s = np.sign(np.einsum("ij,ij->i", normals.numpy().astype(np.float64), ref32["normals"].astype(np.float64)))
    e_n = float(np.abs(s[:, None] * normals.numpy().astype(np.float64) - ref32["normals"]).max())
    frames = geometry.build_tangent_frames(verts, NO_FACES, normals=torch.from_numpy(ref32["normals"]))
    e_f = float((frames - torch.from_numpy(ref32["frames"])).abs().max())
    grad = geometry.build_grad_point_cloud(verts, torch.from_numpy(ref32["frames"]), n_neighbors_cloud=k)
    assert sp.isspmatrix_csc(grad) and grad.dtype == np.complex128 and grad.shape == (len(pts), len(pts))
    e_g = _grad_dev(grad, ref32["gx"] + 1j * ref32["gy"], np.ones(len(pts)))
    helpers.record_margin("cloud_host_fp32_" + name, "cpu", normals_share_of_bound=e_n / (4 * dev_normals), frames_err=e_f,
                          grad_share_of_bound=e_g / (4 * dev_grad), reference_fp32_vs_fp64_normals=dev_normals, reference_fp32_vs_fp64_grad=dev_grad)
    print("host fp32 %s: normals %.3e (bound %.3e), frames %.3e, gradient %.3e (bound %.3e)" % (name, e_n, 4 * dev_normals, e_f, e_g, 4 * dev_grad))
    assert e_n <= 4 * dev_normals
    assert e_f <= 2.0 ** -23            # the same fp32 formula on the same normals: at most a rounding apart
    assert e_g <= 4 * dev_grad


@pytest.mark.parametrize("name", sorted(cloud_cases.golden()))
def test_host_fp64_route_is_the_references_fp64_run(name):
    """The truth of the kernel tests that are not in the fixture is this route: two fp64 LAPACK runs of the same arithmetic, 1e-12 apart at
    most at the singular gaps the checker demands (1e-16 / 1e-3, with room)."""
    pts, k, ref64, _, _, _ = cloud_cases.golden()[name]
    truth = cloud_cases.truth_from_host_route(pts, k)
    cloud_cases.assert_conditions(pts, k, ref64)
    assert np.array_equal(np.sort(truth["nbr"], axis=1), np.sort(ref64["nbr"], axis=1))
    s = np.sign(np.einsum("ij,ij->i", truth["normals"], ref64["normals"]))
    assert float(np.abs(s[:, None] * truth["normals"] - ref64["normals"]).max()) <= 1e-12
    sf = np.stack([np.ones(len(pts)), s, s], axis=1)[:, :, None]
    assert float(np.abs(sf * truth["frames"] - ref64["frames"]).max()) <= 1e-12
    assert _grad_dev(truth["gx"] + 1j * truth["gy"], ref64["gx"] + 1j * ref64["gy"], s) <= 1e-12


def test_mesh_branches_delegate_to_the_host_code():
    from diffusion_net import synthetic
    verts, faces = synthetic.sphere_mesh(120, seed=2)
    vt, ft = torch.from_numpy(verts).float(), torch.from_numpy(faces)
    want = precompute.vertex_normals(vt.numpy().astype(np.float64), faces.astype(np.int64))
    got = geometry.vertex_normals(vt, ft)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want.astype(np.float32))
    frames = geometry.build_tangent_frames(vt.double(), ft)
    assert float(np.abs(frames.numpy() - precompute.tangent_frames(want)).max()) <= 1e-15
    with pytest.raises(ValueError, match="laplacian= is for point clouds"):
        geometry.compute_operators(vt, ft, 4, laplacian=(sp.identity(120), np.ones(120)))


def test_neighborhood_normal_is_numpy_in_numpy_out():
    rs = np.random.RandomState(0)
    P = rs.randn(5, 30, 3).astype(np.float32)
    n = geometry.neighborhood_normal(P)
    assert isinstance(n, np.ndarray) and n.dtype == np.float32 and n.shape == (5, 3)
    lam, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", P.astype(np.float64), P.astype(np.float64)))
    assert float(np.abs(np.abs(np.einsum("ni,ni->n", n, vec[:, :, 0])) - 1).max()) < 1e-5


def _graph_laplacian(pts, k=8):
    """A symmetric kNN-graph Laplacian with unit masses scaled to the cloud: all the tests need of an (L, mass)."""
    v = torch.from_numpy(np.asarray(pts, dtype=np.float64))
    nbr = geometry.find_knn(v, v, k, omit_diagonal=True, method="cpu_kd").indices.numpy()
    n = len(pts)
    A = sp.coo_matrix((np.ones(n * k), (np.repeat(np.arange(n), k), nbr.reshape(-1))), shape=(n, n)).tocsr()
    A = ((A + A.T) > 0).astype(np.float64)
    return (sp.diags(np.asarray(A.sum(axis=1)).reshape(-1)) - A).tocsr(), np.full(n, 4 * np.pi / n)


def test_compute_operators_on_a_cloud_needs_a_laplacian(monkeypatch):
    monkeypatch.setitem(sys.modules, "robust_laplacian", None)        # as on a machine without the wheel
    verts = torch.from_numpy(cloud_cases.sample(80, 5))
    with pytest.raises(ImportError, match=r"laplacian=\(L, massvec\).*robust_laplacian"):
        geometry.compute_operators(verts, NO_FACES, 8)


def test_compute_operators_on_a_cloud_and_the_cache_round_trip(tmp_path):
    pts = cloud_cases.sample(120, 5)
    verts = torch.from_numpy(pts)
    L, mass = _graph_laplacian(pts)
    out = geometry.compute_operators(verts, NO_FACES, 8, laplacian=(L, mass))
    frames, massvec, Lt, evals, evecs, gX, gY = out
    assert tuple(frames.shape) == (120, 3, 3) and tuple(massvec.shape) == (120,) and tuple(evals.shape) == (8,) and tuple(evecs.shape) == (120, 8)
    for t in out:
        assert t.dtype == torch.float32 and not t.is_cuda
    for m in (Lt, gX, gY):
        assert m.is_sparse and m.is_coalesced() and tuple(m.shape) == (120, 120)
    assert gX._nnz() == 120 * 31 and float(evals[0]) < 1e-6 and bool((evals[1:] > 0).all())
    f2, gX2, gY2 = geometry.cloud_operators(verts, 30)
    assert torch.equal(frames, f2) and torch.equal(gX.to_dense(), gX2.to_dense()) and torch.equal(gY.to_dense(), gY2.to_dense())
    calls = []
    lap = lambda v: (calls.append(v.dtype), (L, sp.diags(mass)))[1]                        # the callable form, M as a diagonal matrix
    again = geometry.compute_operators(verts, NO_FACES, 8, laplacian=lap)
    for i in (0, 1, 2, 5, 6):
        assert torch.equal(out[i].to_dense(), again[i].to_dense())
    assert torch.allclose(evals, again[3], atol=1e-5)          # (the Lanczos start vector is random: eigenpairs repeat to its tolerance)
    for e in (evecs, again[4]):                                # ... and are orthonormal in the mass the caller gave
        assert torch.allclose(e.T @ (massvec[:, None] * e), torch.eye(8), atol=1e-4)
    assert calls == [np.float64]
    none = geometry.compute_operators(verts, NO_FACES, 0, laplacian=(L, mass))             # k_eig = 0 works
    assert tuple(none[3].shape) == (0,) and tuple(none[4].shape) == (120, 0)
    # the cache: a miss writes the reference's file layout, a hit reads it back (no Laplacian is needed for a hit)
    first = geometry.get_operators(verts, NO_FACES, k_eig=8, op_cache_dir=str(tmp_path), laplacian=(L, mass))
    files = list(tmp_path.glob("*.npz"))
    assert len(files) == 1 and files[0].name == "%s_0.npz" % diffusion_net.utils.hash_arrays((pts, NO_FACES.numpy()))
    z = np.load(files[0])
    assert {"verts", "frames", "faces", "k_eig", "mass", "L_data", "L_indices", "L_indptr", "L_shape", "evals", "evecs", "gradX_data",
            "gradX_indices", "gradX_indptr", "gradX_shape", "gradY_data", "gradY_indices", "gradY_indptr", "gradY_shape"} == set(z.files)
    assert z["faces"].shape == (0, 3) and z["gradX_data"].dtype == np.float32
    hit = geometry.get_operators(verts, NO_FACES, k_eig=8, op_cache_dir=str(tmp_path))
    for b, c in zip(first, hit):                               # inputs and payload are fp32: the round trip is exact
        assert b.dtype == c.dtype and torch.equal(b.to_dense(), c.to_dense())
    for i in (0, 1, 2, 5, 6):
        assert torch.equal(out[i].to_dense(), first[i].to_dense())
    lists = geometry.get_all_operators([verts, verts], [NO_FACES, NO_FACES], 8, op_cache_dir=str(tmp_path))
    assert len(lists) == 7 and all(len(col) == 2 for col in lists) and torch.equal(lists[0][1], frames)

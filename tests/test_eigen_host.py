"""CPU tier, no device and no emulator: the numpy route of the filtered subspace iteration (``precompute.laplacian_eigenbasis_subspace``)
checked against its inputs and against shift-invert ``eigsh``, the ``eigensolver=`` keyword of ``compute_operators_with`` / ``get_operators`` /
``get_all_operators``, the error paths and the names.  Bodies and criteria in eigen_cases.py."""
import inspect

import numpy as np
import pytest
import torch

import eigen_cases as ec
import diffusion_net
from diffusion_net import geometry, precompute


def test_names_and_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(geometry.laplacian_eigenbasis) == ["L", "massvec", "k_eig", "rtol", "seed", "max_iter", "dtype", "return_info"]
    assert sig(precompute.laplacian_eigenbasis_subspace) == ["L", "massvec", "k_eig", "rtol", "seed", "max_iter", "return_info"]
    for fn in (geometry.laplacian_eigenbasis, precompute.laplacian_eigenbasis_subspace):
        p = inspect.signature(fn).parameters
        assert p["rtol"].default == 1e-9 and p["seed"].default == 0 and p["max_iter"].default == 100 and p["return_info"].default is False
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("rtol", "seed", "max_iter", "return_info"))
    for fn in (geometry.compute_operators_with, geometry.get_operators, geometry.get_all_operators):
        p = inspect.signature(fn).parameters["eigensolver"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    # compute_operators keeps the parameter list it has had; compute_operators_with is the same function plus the keyword
    assert sig(geometry.compute_operators_with) == sig(geometry.compute_operators) + ["eigensolver"]
    assert sig(diffusion_net.ops.cheb_step) == ["rowptr", "col", "val", "Y", "Z", "alpha", "beta", "gamma", "out"]
    assert diffusion_net.laplacian_eigenbasis is geometry.laplacian_eigenbasis
    from diffusion_net import _hip, torchlib  # noqa: F401
    assert "dn_cheb_step_f64" in _hip.EXPORTED_SYMBOLS and "dn_cheb_rows_per_workgroup" in _hip.EXPORTED_SYMBOLS
    assert callable(torch.ops.diffusion_net.cheb_step)


def test_fake_kernel_of_the_custom_operator():
    """``torch.ops.diffusion_net.cheb_step`` on meta tensors: the shape and dtype of the result without a launch."""
    from diffusion_net import torchlib  # noqa: F401
    m = lambda *s, dtype=torch.float64: torch.empty(*s, dtype=dtype, device="meta")
    out = torch.ops.diffusion_net.cheb_step(m(11, dtype=torch.int32), m(30, dtype=torch.int32), m(30), m(10, 7), None, 1.0, 0.0, 0.0)
    assert out.device.type == "meta" and tuple(out.shape) == (10, 7) and out.dtype == torch.float64


@pytest.mark.parametrize("name", list(ec.SOLVER_CASES))
def test_numpy_route(name):
    ec.run_solver(name, "cpu", "numpy")


def test_block_width_and_dense_threshold():
    assert [precompute.subspace_block_width(k) for k in (1, 8, 64, 65, 128)] == [17, 24, 80, 82, 160]
    L, m = ec.pencil("sphere40")
    for k, route in ((4, "numpy"), (5, "dense")):            # nb = 20: 2 nb = 40 = V is the last size the iteration takes
        evals, evecs, info = precompute.laplacian_eigenbasis_subspace(L, m, k, return_info=True)
        assert info["route"] == route and evals.shape == (k,) and evecs.shape == (40, k)
    with pytest.raises(ValueError):
        precompute.laplacian_eigenbasis_subspace(L, m, 41)


def test_k_zero_returns_empties():
    L, m = ec.pencil("sphere40")
    evals, evecs = precompute.laplacian_eigenbasis_subspace(L, m, 0)
    assert evals.shape == (0,) and evecs.shape == (40, 0)
    evals, evecs, info = geometry.laplacian_eigenbasis(L, torch.from_numpy(np.array(m)), 0, return_info=True)
    assert tuple(evals.shape) == (0,) and tuple(evecs.shape) == (40, 0) and info["iterations"] == 0


def test_seed_and_repeatability():
    """The same seed gives the same bits; another seed another block and the same eigenvalues to the tolerance."""
    a = ec.solve_numpy("sphere300_k16")
    b = ec.solve_numpy("sphere300_k16")
    c = ec.solve_numpy("sphere300_k16", seed=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], c[1])
    assert float((a[0] - c[0]).abs().max()) <= 2 * ec.RTOL * float(a[0][-1])


def test_max_iter_reached_raises():
    L, m = ec.pencil("sphere300")
    with pytest.raises(RuntimeError, match=r"1 iterations did not reach rtol.*residual"):
        precompute.laplacian_eigenbasis_subspace(L, m, 16, max_iter=1)


def test_failed_cholesky_raises(monkeypatch):
    """A Gram matrix without a Cholesky factor is a ``RuntimeError`` that names the iteration and the residual -- the factorisation itself
    on an indefinite matrix, and the driver when its fifth factorisation (the first of iteration 2) fails.  A non-finite operator is refused."""
    import scipy.linalg
    with pytest.raises(RuntimeError, match="Cholesky-QR failed in iteration 3"):
        precompute._cholesky_upper(np.array([[1.0, 2.0], [2.0, 1.0]]), "in iteration 3 (residual 0.001)")
    L, m = ec.pencil("sphere300")
    real, calls = scipy.linalg.cholesky, []

    def failing(a, *args, **kw):
        calls.append(1)
        if len(calls) == 5:
            raise scipy.linalg.LinAlgError("5-th leading minor of the array is not positive definite")
        return real(a, *args, **kw)
    monkeypatch.setattr(scipy.linalg, "cholesky", failing)
    with pytest.raises(RuntimeError, match=r"Cholesky-QR failed in iteration 2 \(residual [0-9.e+-]+\)"):
        precompute.laplacian_eigenbasis_subspace(L, m, 16)
    monkeypatch.undo()
    bad = L.copy()
    bad.data = bad.data.copy()
    bad.data[5] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        precompute.laplacian_eigenbasis_subspace(bad, m, 16)


def test_torch_sparse_and_output_dtype():
    """``geometry.laplacian_eigenbasis`` takes a torch sparse L; results in the mass's dtype unless ``dtype`` says otherwise."""
    L, m = ec.pencil("sphere300")
    Lt = precompute._to_torch_sparse(L, "cpu", torch.float64)
    m32 = torch.from_numpy(np.array(m)).float()
    ev32, U32 = geometry.laplacian_eigenbasis(Lt, m32, 16)
    assert ev32.dtype == U32.dtype == torch.float32 and tuple(U32.shape) == (300, 16)
    ev64, _ = geometry.laplacian_eigenbasis(L, torch.from_numpy(np.array(m)), 16)
    assert ev64.dtype == torch.float64
    ref = np.clip(ec.eigsh_reference("sphere300_k16")[0][:16], 0.0, np.inf)
    assert np.abs(ev64.numpy() - ref).max() <= 2 * ec.RTOL * ref[-1]
    # the fp32 run solved the pencil of the fp32-rounded mass -- every eigenvalue moves by at most 2^-24 / (1 - 2^-24) of itself (a diagonal
    # congruence: Ostrowski) -- to 2 rtol lambda_k, and rounded the result to fp32: 3 x 2^-24 lambda_k covers the three
    assert np.abs(ev32.double().numpy() - ref).max() <= 3 * 2.0 ** -24 * ref[-1]


def test_compute_operators_with_the_subspace_solver():
    ec.run_compute_operators("cpu")


def test_point_cloud_branches_take_the_keyword():
    """Both point-cloud branches: ``laplacian="delaunay"`` and a caller's pair."""
    import cloud_cases
    pts = torch.from_numpy(cloud_cases.sample(500, ec.MESH_SEED).astype(np.float64))
    faces = torch.zeros(0, 3, dtype=torch.long)
    ref = geometry.compute_operators(pts, faces, 30, laplacian="delaunay")
    got = geometry.compute_operators_with(pts, faces, 30, laplacian="delaunay", eigensolver="subspace")
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    lam, lam_ref = got[3].numpy(), ref[3].numpy()
    assert np.abs(lam - lam_ref).max() <= 2 * ec.RTOL * lam_ref[-1] and got[4].shape == ref[4].shape
    L, m = ec.pencil("cloud500")
    got = geometry.compute_operators_with(pts, faces, 30, laplacian=(L, np.array(m)), eigensolver="subspace")
    ref = np.clip(ec.eigsh_reference("cloud500_k30")[0][:30], 0.0, np.inf)
    assert np.abs(got[3].numpy() - ref).max() <= 2 * ec.RTOL * ref[-1]


def test_cache_round_trip_and_bad_values(tmp_path, monkeypatch):
    ec.run_cache_round_trip("cpu", tmp_path, monkeypatch)

"""CPU tier: the numpy route of the point-cloud Laplacian (``precompute.point_cloud_laplacian_host``) -- the oracle of the kernel tests --
against ``scipy.spatial.Delaunay`` and its algebraic invariants, and ``compute_operators(..., laplacian="delaunay")`` on host tensors."""
import functools
import inspect

import numpy as np
import pytest
import scipy.spatial
import torch

import cloud_lap_cases
import helpers
from diffusion_net import geometry, precompute

NO_FACES = torch.zeros(0, 3, dtype=torch.long)


@functools.lru_cache(maxsize=None)
def host_run(n, k, seed, kind):
    """The numpy route on a case, with the table and the frames it made for itself (fp64)."""
    pts = cloud_lap_cases.sample(n, seed, kind).astype(np.float64)
    t = torch.from_numpy(pts)
    nbr = geometry.find_knn(t, t, k, omit_diagonal=True, method="cpu_kd").indices.numpy()
    frames = precompute.tangent_frames(precompute.neighborhood_normal(pts[nbr] - pts[:, None, :]))
    L, mass, parts = precompute.point_cloud_laplacian_from_table(pts, nbr, frames, with_parts=True)
    return pts, nbr, frames, L, mass, parts


def test_names_and_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(precompute.point_cloud_laplacian_host) == ["v64", "n_neighbors", "frames"]
    assert sig(geometry.point_cloud_laplacian) == ["verts", "n_neighbors", "frames"]
    assert inspect.signature(geometry.point_cloud_laplacian).parameters["n_neighbors"].default == 30
    from diffusion_net import _hip, ops
    for name in ("dn_cloud_star_f32", "dn_cloud_laplacian_emit_f32", "dn_segment_sum_f64_f32", "dn_cloud_laplacian_workspace_bytes"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert callable(ops.cloud_laplacian)


@pytest.mark.parametrize("n,k,seed,kind", cloud_lap_cases.CASES)
def test_stars_are_the_delaunay_triangles_at_the_centre(n, k, seed, kind):
    """On every point: the oracle's star == the triangles of scipy's (Qhull's) Delaunay triangulation of {0} u projected neighbours that
    hold vertex 0, as sets.  The input's decision margins are asserted first, as in the kernel tests."""
    pts, nbr, frames, _, _, parts = host_run(n, k, seed, kind)
    m_in, m_cr = cloud_lap_cases.decision_margins(pts, nbr, frames)
    assert m_in >= cloud_lap_cases.INCIRCLE_MARGIN and m_cr >= cloud_lap_cases.CROSS_MARGIN, (m_in, m_cr)
    X, Y, _ = precompute.cloud_project(pts, nbr, frames)
    stars = cloud_lap_cases.stars_of(parts["partner"])
    for i in range(n):
        P = np.concatenate([np.zeros((1, 2)), np.stack([X[i], Y[i]], axis=1)])
        want = {frozenset(int(v) - 1 for v in s if v != 0) for s in scipy.spatial.Delaunay(P).simplices if 0 in s}
        assert stars[i] == want, "point %d: %s != %s" % (i, sorted(map(sorted, stars[i])), sorted(map(sorted, want)))


@pytest.mark.parametrize("n,k,seed,kind", cloud_lap_cases.CASES)
def test_host_laplacian_is_symmetric_with_zero_row_sums_and_psd(n, k, seed, kind):
    _, _, _, L, mass, _ = host_run(n, k, seed, kind)
    D = L.toarray()
    assert np.array_equal(D, D.T)                       # every term stands under (i, j) and (j, i): the route sums one copy and mirrors it
    absrow = np.abs(D).sum(axis=1)
    assert (np.abs(D.sum(axis=1)) <= 1e-12 * absrow).all()
    lam = float(np.linalg.eigvalsh(D).min())
    assert lam >= -1e-12 * float(absrow.max()), lam
    assert (mass >= 0).all() and mass.sum() > 0
    helpers.record_margin("cloud_lap_host_n%d_k%d_%s" % (n, k, kind), "cpu", rowsum_rel=float((np.abs(D.sum(axis=1)) / absrow).max()),
                          min_eig_rel=lam / float(absrow.max()))


def test_public_host_function_is_the_table_route():
    n, k, seed, kind = cloud_lap_cases.CASES[2]
    pts, nbr, frames, L, mass, _ = host_run(n, k, seed, kind)
    L2, mass2 = precompute.point_cloud_laplacian_host(pts, k)
    assert (L != L2).nnz == 0 and np.array_equal(mass, mass2)
    L3, _ = precompute.point_cloud_laplacian_host(torch.from_numpy(pts), k, frames=torch.from_numpy(frames))
    assert (L != L3).nnz == 0
    Lt, mt = geometry.point_cloud_laplacian(torch.from_numpy(pts), k)                    # host tensors, fp64: the same numbers as tensors
    assert Lt.is_sparse and Lt.is_coalesced() and Lt.dtype == torch.float64 and mt.dtype == torch.float64
    assert np.array_equal(Lt.to_dense().numpy(), L.toarray()) and np.array_equal(mt.numpy(), mass)


@functools.lru_cache(maxsize=None)
def sphere_operators():
    pts = cloud_lap_cases.sample(1500, 0)
    return pts, geometry.compute_operators(torch.from_numpy(pts), NO_FACES, 10, laplacian="delaunay")


def test_delaunay_operators_of_a_sphere_have_its_spectrum_and_area():
    """Unit sphere, 1500 points, 30 neighbours: the Laplace-Beltrami spectrum is l (l + 1) with multiplicity 2 l + 1, the area 4 pi.
    Measured with this code on this sample: evals[1:4] = 1.9825 .. 2.0179 (largest deviation from 2: 0.90 %), evals[4:9] = 5.9026 .. 6.0446
    (from 6: 1.62 %), mass sum 0.571 % below 4 pi (flat triangles inscribed in the sphere).  Asserted at twice the measured deviations:
    1.8 %, 3.3 % and 1.15 %."""
    pts, out = sphere_operators()
    frames, massvec, L, evals, evecs, gX, gY = out
    assert len(out) == 7
    for t, shape in zip(out, ((1500, 3, 3), (1500,), (1500, 1500), (10,), (1500, 10), (1500, 1500), (1500, 1500))):
        assert t.dtype == torch.float32 and not t.is_cuda and tuple(t.shape) == shape
    assert L.is_sparse and L.is_coalesced()
    ev = evals.double().numpy()
    d2, d6 = float(np.abs(ev[1:4] / 2.0 - 1.0).max()), float(np.abs(ev[4:9] / 6.0 - 1.0).max())
    dm = float(massvec.double().sum() / (4 * np.pi) - 1.0)
    print("sphere 1500: evals[1:4] %.4f .. %.4f (dev %.3e), evals[4:9] %.4f .. %.4f (dev %.3e), mass sum / 4 pi - 1 = %.3e" % (
        ev[1:4].min(), ev[1:4].max(), d2, ev[4:9].min(), ev[4:9].max(), d6, dm))
    helpers.record_margin("cloud_lap_sphere_n1500_k30", "cpu", dev_evals_2=d2, dev_evals_6=d6, dev_mass=dm)
    assert ev[0] < 1e-4
    assert d2 <= 0.018 and d6 <= 0.033 and abs(dm) <= 0.0115
    assert torch.allclose(evecs.T.double() @ (massvec.double()[:, None] * evecs.double()), torch.eye(10, dtype=torch.float64), atol=1e-4)


def test_callable_form_gives_the_same_laplacian_as_delaunay():
    """fp64 host tensors: ``"delaunay"`` works on the frames and the table of ``cloud_operators``, the callable makes its own from the
    fp64 positions -- the same arithmetic, so the same L and (up to the EPS x mean that only the named form adds) the same mass."""
    pts = cloud_lap_cases.sample(300, 3).astype(np.float64)
    verts = torch.from_numpy(pts)
    named = geometry.compute_operators(verts, NO_FACES, 6, laplacian="delaunay")
    called = geometry.compute_operators(verts, NO_FACES, 6, laplacian=precompute.point_cloud_laplacian_host)
    assert named[2].dtype == torch.float64
    assert torch.equal(named[2].to_dense(), called[2].to_dense())
    mass = called[1]
    assert torch.allclose(named[1], mass + precompute.EPS * mass.mean(), rtol=1e-14, atol=0)
    assert torch.allclose(named[3], called[3], rtol=1e-6, atol=1e-9)
    for i in (0, 5, 6):
        assert torch.equal(named[i].to_dense(), called[i].to_dense())


def test_delaunay_passes_through_get_operators_and_rejects_other_names(tmp_path):
    pts = cloud_lap_cases.sample(120, 5)
    verts = torch.from_numpy(pts)
    out = geometry.compute_operators(verts, NO_FACES, 4, laplacian="delaunay")
    first = geometry.get_operators(verts, NO_FACES, k_eig=4, op_cache_dir=str(tmp_path), laplacian="delaunay")
    for i in (0, 1, 2, 5, 6):
        assert torch.equal(out[i].to_dense(), first[i].to_dense())
    lists = geometry.get_all_operators([verts, verts], [NO_FACES, NO_FACES], 4, laplacian="delaunay")
    assert len(lists) == 7 and torch.equal(lists[2][1].to_dense(), out[2].to_dense())
    with pytest.raises(ValueError, match="delaunay"):
        geometry.compute_operators(verts, NO_FACES, 4, laplacian="tufted")

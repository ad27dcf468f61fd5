"""CPU tier: the yardstick of the mesh-operator tests and its bounds.  The fp64 host route of ``precompute`` with its faces shuffled and
rotated -- the same terms summed in other orders -- must pass the bounds of mesh_cases.py that the kernels are held to; no test vertex may
sit on the frame's branch; and the ``assembly=`` keyword on host tensors without a device is the host route."""
import inspect

import numpy as np
import pytest
import torch

import helpers
import mesh_cases
from diffusion_net import geometry, precompute

ALL = mesh_cases.CASES + mesh_cases.DEGENERATE + mesh_cases.FALLBACK


def test_names_and_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(geometry.mesh_operators) == ["verts", "faces", "normals"]
    assert sig(geometry.compute_operators_via) == sig(geometry.compute_operators_with) + ["assembly"]
    for fn in (geometry.compute_operators_via, geometry.get_operators, geometry.get_all_operators):
        p = inspect.signature(fn).parameters["assembly"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    from diffusion_net import _hip, ops, torchlib  # noqa: F401
    for name in ("dn_mesh_workspace_bytes", "dn_mesh_emit_f32", "dn_segment_sum_f64_f64", "dn_segment_sum4_f64_f64", "dn_mesh_frames_gradients_f64"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert callable(ops.mesh_assemble) and callable(ops.mesh_frames_gradients) and callable(ops._mesh_assemble_launch)
    assert callable(torch.ops.diffusion_net.mesh_assemble) and callable(torch.ops.diffusion_net.mesh_frames_gradients)


@pytest.mark.parametrize("name", ALL)
def test_no_vertex_sits_on_the_branch_of_the_frame(name):
    host, _, _ = mesh_cases.reference(name)
    if host["V"]:
        gap = float(np.abs(np.abs(host["normals"][:, 0]) - 0.9).min())
        assert gap >= mesh_cases.BRANCH_MARGIN, "a normal of %s is %.3e from |n_x| = 0.9 (change the mesh, not the margin)" % (name, gap)


@pytest.mark.parametrize("name", ALL)
def test_shuffled_host_route_passes_the_bounds(name):
    """Other summation orders of the same fp64 terms: faces permuted, every face rotated (its orientation kept).  The same checks the
    kernels get, at the same bounds -- with the normals of the shuffled route itself, which differ from the first route's by their own
    round-off: the frames and gradients are held to the bounds ``geometry.mesh_operators`` gets for the device's normals."""
    host, _, b = mesh_cases.reference(name)
    v, f = mesh_cases.mesh(name)
    rs = np.random.RandomState(11)
    fs = f[rs.permutation(len(f))]
    fs = np.stack([np.roll(row, int(s)) for row, s in zip(fs, rs.randint(0, 3, len(fs)))]) if len(fs) else fs
    # (a vertex without a finite normal gets the jitter-and-fixed-direction rule, which is no function of round-off: those cases keep the
    # first route's normals, as ``geometry.mesh_operators`` does)
    other = mesh_cases.host_route(v, fs, normals=host["normals"] if name in mesh_cases.FALLBACK else None)
    L, g = other["L"], other["grad"]
    got = dict(rowptr=L.indptr, col=L.indices, L=L.data, mass=other["mass"], raw_normals=other["raw_normals"], frames=other["frames"],
               gx=np.ascontiguousarray(g.data.real), gy=np.ascontiguousarray(g.data.imag))
    assert np.array_equal(L.indptr, host["L"].indptr) and np.array_equal(L.indices, host["L"].indices)
    rows = np.repeat(np.arange(host["V"]), np.diff(L.indptr))
    rowsum = mesh_cases.share(np.abs(np.bincount(rows, weights=L.data, minlength=host["V"])), np.bincount(rows, weights=b["L"], minlength=host["V"]))
    shares = mesh_cases.compare(got, host, b)
    print("shuffled host route %s: shares of the bounds %s, row sums %.3f" % (name, {k: round(s, 4) for k, s in shares.items()}, rowsum))
    helpers.record_margin("mesh_host_shuffled_" + name, "cpu", rowsum_share_of_bound=rowsum, **{k + "_share_of_bound": s for k, s in shares.items()})
    assert rowsum <= 1.0
    for k, s in shares.items():
        assert s <= 1.0, (k, s)


def test_bounds_are_not_vacuous():
    """The L bound of a well-shaped mesh is a few hundred u of the entry, the mass bound below 1e-14 relative: a kernel that summed in
    fp32, or dropped a term, misses them by orders of magnitude."""
    host, b, _ = mesh_cases.reference("sphere1500")
    rel = b["L"] / np.abs(host["L"].data)
    assert np.median(rel) < 1e-12 and (b["mass"] / host["mass"]).max() < 1e-14
    assert (b["L"] < 2.0 ** -24 * np.abs(host["L"].data)).mean() > 0.9


def test_right_triangle_keeps_its_explicit_zero():
    host, _, _ = mesh_cases.reference("right_triangle")
    L = host["L"]
    assert L.nnz == 9 and L[1, 2] == 0 and L[2, 1] == 0 and (host["grad"].toarray()[1, 2] != 0)


def test_mesh_operators_on_host_tensors_is_the_host_route():
    v, f = mesh_cases.mesh("sphere200")
    tv, tf = torch.from_numpy(np.array(v)).double(), torch.from_numpy(np.array(f))
    frames, mass, L, gX, gY = geometry.mesh_operators(tv, tf)
    ref = geometry.compute_operators(tv, tf, 4)
    assert torch.equal(frames, ref[0]) and torch.equal(L.to_dense(), ref[2].to_dense())
    assert torch.equal(gX.to_dense(), ref[5].to_dense()) and torch.equal(gY.to_dense(), ref[6].to_dense())
    assert torch.allclose(mass + precompute.EPS * mass.mean(), ref[1], rtol=1e-15, atol=0)


def test_device_assembly_of_host_tensors_is_the_host_route():
    v, f = mesh_cases.sphere300()
    tv, tf = torch.from_numpy(np.array(v)), torch.from_numpy(np.array(f))
    got = geometry.compute_operators_via(tv, tf, 8, assembly="device")
    ref = geometry.compute_operators(tv, tf, 8)
    for i in (0, 1, 2, 5, 6):                                    # (eigsh starts from a random vector: its pairs repeat to its tolerance only)
        a, b = (got[i].to_dense(), ref[i].to_dense()) if got[i].is_sparse else (got[i], ref[i])
        assert torch.equal(a, b), i
    assert torch.allclose(got[3], ref[3], rtol=1e-5, atol=1e-6) and got[4].shape == ref[4].shape


def test_cache_round_trip_and_bad_values_on_host_tensors(tmp_path):
    mesh_cases.run_cache_round_trip("cpu", tmp_path)

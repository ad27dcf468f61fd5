"""CPU tier (no library): the fp32 model of fps_cases.py against the reference's recorded masks (tests/golden/geom_fps_ref.npz), the host
routes of ``geometry.farthest_point_sampling`` / ``farthest_point_samples``, and the torch vector helpers against the reference's outputs."""
import os

import numpy as np
import pytest
import torch

import diffusion_net
import fps_cases


def test_model_equals_the_reference_mask_on_every_fixture_case():
    ran = 0
    for name, raw, normalized, n_sample, mask, _ in fps_cases.golden_cases():
        order, radii, md = fps_cases.model(normalized, n_sample)
        assert np.array_equal(fps_cases.mask_of(order, len(raw)), mask), name
        assert np.isinf(radii[0]) and bool((radii[1:] <= radii[:-1]).all())
        ran += 1
    assert ran == 4


def test_public_function_on_host_tensors_equals_the_fixture():
    for name, raw, normalized, n_sample, mask, _ in fps_cases.golden_cases():
        got = diffusion_net.geometry.farthest_point_sampling(torch.from_numpy(raw), n_sample)
        assert got.dtype == torch.bool and tuple(got.shape) == (len(raw),)
        assert np.array_equal(got.numpy(), mask), name
        assert torch.equal(diffusion_net.geometry.normalize_positions(torch.from_numpy(raw)), torch.from_numpy(normalized)), name


def test_batched_form_on_host_tensors_equals_the_single_calls():
    cases = list(fps_cases.golden_cases())
    got = diffusion_net.farthest_point_samples([torch.from_numpy(c[1]) for c in cases], 30)
    assert len(got) == len(cases)
    for g, c in zip(got, cases):
        assert torch.equal(g, diffusion_net.farthest_point_sampling(torch.from_numpy(c[1]), 30))
    assert diffusion_net.farthest_point_samples([], 3) == []


def test_vector_helpers_equal_the_reference():
    z = np.load(os.path.join(fps_cases.GOLDEN, "geom_fps_ref.npz"))
    G = diffusion_net.geometry
    verts, faces, a, b = (torch.from_numpy(z["helpers/" + k]) for k in ("verts", "faces", "a", "b"))
    unit = G.normalize(b)
    got = {"norm": G.norm(a), "norm2": G.norm2(a), "normalize": unit, "dot": G.dot(a, b), "cross": G.cross(a, b),
           "project_to_tangent": G.project_to_tangent(a, unit), "face_coords": G.face_coords(verts, faces),
           "face_area": G.face_area(verts, faces), "face_normals": G.face_normals(verts, faces),
           "face_normals_raw": G.face_normals(verts, faces, normalized=False)}
    for name, v in got.items():
        assert fps_cases.same_bits(v.numpy(), z["helpers/" + name]), name
    assert G.norm(a, highdim=True).shape == (30,) and G.normalize(torch.ones(2, 7), highdim=True).shape == (2, 7)
    assert torch.equal(G.normalize(a, divide_eps=0.5), a / (a.norm(dim=-1) + 0.5).unsqueeze(-1))
    with pytest.raises(ValueError, match="single vector"):
        G.normalize(torch.ones(3))
    with pytest.raises(ValueError, match="large last dimension"):
        G.normalize(torch.ones(2, 7))


def test_more_samples_than_points_is_a_value_error():
    with pytest.raises(ValueError, match="not enough points to sample"):
        diffusion_net.geometry.farthest_point_sampling(torch.randn(10, 3), 11)
    with pytest.raises(ValueError, match="not enough points to sample"):
        diffusion_net.farthest_point_samples([torch.randn(10, 3), torch.randn(5, 3)], 6)


def test_no_sample_still_sets_the_centremost_point():
    pts = torch.from_numpy(fps_cases.cloud(50, 3))
    got = diffusion_net.farthest_point_sampling(pts, 0)
    assert int(got.sum()) == 1 and torch.equal(got, diffusion_net.farthest_point_sampling(pts, 1))
    centre = diffusion_net.geometry.normalize_positions(pts).pow(2).sum(-1).argmin()
    assert bool(got[centre])


@pytest.mark.parametrize("dtype,D", [(torch.float64, 3), (torch.float32, 2), (torch.float32, 5), (torch.float64, 5)])
def test_torch_route_for_other_dtypes_and_dimensions(dtype, D):
    """fp64 and D != 3 against a straightforward fp64 restatement (clouds without near-ties at this precision: the gap is asserted)."""
    g = torch.Generator().manual_seed(5)
    pts = torch.randn(120, D, generator=g, dtype=torch.float64).to(dtype)
    got = diffusion_net.geometry.farthest_point_sampling(pts, 25)
    assert got.dtype == torch.bool and int(got.sum()) == 25
    p = diffusion_net.geometry.normalize_positions(pts).double().numpy()
    i = int(np.argmin((p * p).sum(-1)))
    md = np.full(120, np.inf)
    want = np.zeros(120, dtype=bool)
    for _ in range(25):
        want[i] = True
        md = np.minimum(md, ((p - p[i]) ** 2).sum(-1))
        top = np.sort(md)[-2:]
        assert top[1] - top[0] > 1e-5 * top[1]
        i = int(np.argmax(md))
    assert np.array_equal(got.numpy(), want)


def test_names_resolve_on_the_package():
    assert diffusion_net.farthest_point_sampling is diffusion_net.geometry.farthest_point_sampling
    assert diffusion_net.farthest_point_samples is diffusion_net.geometry.farthest_point_samples
    for name in ("norm", "norm2", "normalize", "dot", "cross", "project_to_tangent", "face_coords", "face_area", "face_normals"):
        assert callable(getattr(diffusion_net.geometry, name)), name


def test_fake_kernel_of_the_registered_operator():
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fps)
    o, r = torch.ops.diffusion_net.fps(torch.empty(50, 3, device="meta"), 7)
    assert o.shape == (7,) and o.dtype == torch.int64 and r.shape == (7,) and r.dtype == torch.float32

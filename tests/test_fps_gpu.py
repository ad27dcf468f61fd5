"""GPU tier: farthest point sampling (dn_fps.hip) on the device -- the shared cases of fps_cases.py bit for bit against the fp32 model,
``geometry.farthest_point_sampling`` / ``farthest_point_samples`` on device tensors (kernel route, torch route past the kernel's limits),
the registered operator under ``torch.compile``, both routes captured in a graph, and one workload-shaped run per route."""
import os

import numpy as np
import pytest
import torch

import fps_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.lib()                      # raises if libdiffnet_hip.so is missing: no fallback
    assert lib.dn_fps_resident_max_points() == fps_cases.RESIDENT_MAX
    return torch.device("cuda:0")


@pytest.mark.parametrize("n", fps_cases.resident_sizes(True))
def test_resident_size(dev, n):
    fps_cases.run_resident_size(dev, n)


def test_resident_rejects_past_capacity(dev):
    fps_cases.run_resident_rejects_past_capacity(dev)


@pytest.mark.parametrize("n", fps_cases.STEPPED_SIZES)
def test_stepped_size(dev, n):
    fps_cases.run_stepped_size(dev, n)


def test_routes_agree(dev):
    fps_cases.run_routes_agree(dev)


@pytest.mark.parametrize("route", [0, 2])
@pytest.mark.parametrize("sizes,n_sample", [((1, 64, 65, 1000), 1), ((300, 257, 1000), 200)])
def test_batch(dev, sizes, n_sample, route):
    fps_cases.run_batch(dev, list(sizes), n_sample, route)


def test_no_clouds(dev):
    fps_cases.run_no_clouds(dev)


def test_start(dev):
    fps_cases.run_start(dev)


def test_reference_fixture(dev):
    fps_cases.run_reference_fixture(dev)


def test_exact_ties(dev):
    fps_cases.run_exact_ties(dev)


def test_properties(dev):
    fps_cases.run_properties(dev)


def test_non_finite(dev):
    fps_cases.run_non_finite(dev)


def test_public_function_is_the_model_on_the_devices_own_normalisation(dev):
    """Device tensors: the mask equals the model applied to the device's normalised points, bit for bit in the order behind it; and on the
    gap-checked fixture clouds it equals the reference's mask (the device's normalisation may round a coordinate differently; the
    fixture's generator asserts winner / runner-up gaps of 1e-4, far above what that can move)."""
    import diffusion_net
    checked = 0
    for name, raw, normalized, n_sample, mask, gap_checked in fps_cases.golden_cases():
        pts = torch.from_numpy(raw).to(dev)
        got = diffusion_net.geometry.farthest_point_sampling(pts, n_sample)
        assert got.is_cuda and got.dtype == torch.bool
        own = diffusion_net.geometry.normalize_positions(pts).cpu().numpy()
        assert np.array_equal(got.cpu().numpy(), fps_cases.mask_of(fps_cases.model(own, n_sample)[0], len(raw))), name
        if gap_checked:
            assert np.array_equal(got.cpu().numpy(), mask), name
            checked += 1
    assert checked == 2
    pts = torch.from_numpy(fps_cases.cloud(300, 90)).to(dev)
    assert torch.equal(diffusion_net.farthest_point_sampling(pts, 0), diffusion_net.farthest_point_sampling(pts, 1))
    with pytest.raises(ValueError, match="not enough points to sample"):
        diffusion_net.farthest_point_sampling(pts, 301)


def test_batched_form_equals_the_single_calls(dev):
    import diffusion_net
    clouds = [torch.from_numpy(fps_cases.cloud(n, 91 + n) * 2.0 - 0.5).to(dev) for n in (130, 1000, 257)]
    masks = diffusion_net.farthest_point_samples(clouds, 60)
    assert len(masks) == 3
    for pts, mask in zip(clouds, masks):
        assert mask.is_cuda and torch.equal(mask, diffusion_net.farthest_point_sampling(pts, 60)) and int(mask.sum()) == 60


def test_torch_route_past_the_kernel_limits(dev):
    """fp64, D != 3 and requires_grad: the loop in torch on the device, equal to the same loop on the host at clouds without near-ties."""
    import diffusion_net
    g = torch.Generator().manual_seed(33)
    for dtype, D in ((torch.float64, 3), (torch.float32, 2), (torch.float32, 5)):
        pts = torch.randn(150, D, generator=g, dtype=torch.float64).to(dtype)
        got = diffusion_net.farthest_point_sampling(pts.to(dev), 20)
        assert got.is_cuda and int(got.sum()) == 20
        if dtype == torch.float64:
            assert torch.equal(got.cpu(), diffusion_net.farthest_point_sampling(pts, 20))
    pts = torch.from_numpy(fps_cases.golden_cases().__next__()[1]).to(dev)
    a = pts.clone().requires_grad_(True)
    assert torch.equal(diffusion_net.farthest_point_sampling(a, 32), diffusion_net.farthest_point_sampling(pts, 32))


def test_registered_operator_under_torch_compile(dev):
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fps)
    pts = torch.from_numpy(fps_cases.cloud(700, 95)).to(dev)

    def f(p):
        o, r = torch.ops.diffusion_net.fps(p * 1.0, 30)
        return o + 0, r + 0.0

    eager = f(pts)
    compiled = torch.compile(f, fullgraph=True)(pts)
    assert torch.equal(compiled[0], eager[0]) and torch.equal(compiled[1], eager[1])
    want = fps_cases.model(pts.cpu().numpy(), 30)
    assert fps_cases.same_bits(eager[0].cpu().numpy(), want[0]) and fps_cases.same_bits(eager[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("route", [1, 2])
def test_graph_capture_and_replay(dev, route):
    """A captured call replays twice with the eager bits, on other points the second time (nothing synchronises, nothing is memset)."""
    from diffusion_net import ops
    a = torch.from_numpy(fps_cases.cloud(1500, 96)).to(dev)
    b = torch.from_numpy(fps_cases.cloud(1500, 97)).to(dev)
    eager_a, eager_b = ops.fps(a, 40, route=route, return_min_dist=True), ops.fps(b, 40, route=route, return_min_dist=True)
    buf = a.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fps(buf, 40, route=route, return_min_dist=True)       # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.fps(buf, 40, route=route, return_min_dist=True)
    for src, eager in ((a, eager_a), (b, eager_b)):
        buf.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(out, eager):
            assert torch.equal(u, v)


@pytest.mark.parametrize("route", [1, 2])
def test_workload_shape(dev, route):
    """10 000 -> 1 000 through each route against the model."""
    fps_cases.check_single(dev, fps_cases.cloud(10000, 98, "sphere"), 1000, route)

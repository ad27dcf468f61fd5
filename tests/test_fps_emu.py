"""CPU tier (emulator build of the same kernel source, dn_fps.hip): farthest point sampling through the C ABI and ``ops.fps`` on host
buffers, bit for bit against the fp32 model -- every instantiation of the resident kernel on both sides of its size, the stepped route's
slice map, both routes on one input, batches, the tie rule, non-finite input, the error returns.  Bodies in fps_cases.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fps_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-net_amd", "csrc")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libdiffnet_emu.so")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not (os.path.exists(HOSTCXX) and shutil.which("make")), reason="host clang++/make not available")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", CSRC, "-j8", "emu"], check=True, capture_output=True)
    from diffusion_net import _hip
    _hip._use_library_for_tests(EMU_SO, True)
    yield "cpu"
    _hip._use_library_for_tests(None, False)


@pytest.mark.parametrize("n", fps_cases.resident_sizes(False))
def test_resident_size_on_emulator(emu, n):
    fps_cases.run_resident_size(emu, n)


def test_resident_rejects_past_capacity_on_emulator(emu):
    fps_cases.run_resident_rejects_past_capacity(emu)


@pytest.mark.parametrize("n", fps_cases.STEPPED_SIZES)
def test_stepped_size_on_emulator(emu, n):
    fps_cases.run_stepped_size(emu, n)


def test_routes_agree_on_emulator(emu):
    fps_cases.run_routes_agree(emu)


@pytest.mark.parametrize("route", [0, 2])
@pytest.mark.parametrize("sizes,n_sample", [((1, 64, 65, 1000), 1), ((300, 257, 1000), 200)])
def test_batch_on_emulator(emu, sizes, n_sample, route):
    fps_cases.run_batch(emu, list(sizes), n_sample, route)


def test_no_clouds_on_emulator(emu):
    fps_cases.run_no_clouds(emu)


def test_start_on_emulator(emu):
    fps_cases.run_start(emu)


def test_reference_fixture_on_emulator(emu):
    fps_cases.run_reference_fixture(emu)


def test_exact_ties_on_emulator(emu):
    fps_cases.run_exact_ties(emu)


def test_properties_on_emulator(emu):
    fps_cases.run_properties(emu)


def test_non_finite_on_emulator(emu):
    fps_cases.run_non_finite(emu)


def test_abi_errors_on_emulator(emu):
    fps_cases.run_abi_errors()


def test_public_functions_take_the_kernel_route_on_emulator(emu):
    """While the emulator library is bound, host fp32 [V, 3] tensors go through ``ops.fps``: the mask equals the model on the function's own
    normalised points, and the batched form equals the single calls."""
    import diffusion_net
    clouds = [torch.from_numpy(fps_cases.cloud(n, 80 + n) * 3.0 + 1.0) for n in (130, 600)]
    masks = diffusion_net.farthest_point_samples(clouds, 25)
    for pts, mask in zip(clouds, masks):
        one = diffusion_net.farthest_point_sampling(pts, 25)
        want = fps_cases.model(diffusion_net.geometry.normalize_positions(pts).numpy(), 25)[0]
        assert np.array_equal(one.numpy(), fps_cases.mask_of(want, len(pts))) and torch.equal(one, mask)
    assert torch.equal(diffusion_net.farthest_point_sampling(clouds[0], 0), diffusion_net.farthest_point_sampling(clouds[0], 1))

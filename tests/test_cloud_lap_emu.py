"""CPU tier (emulator build of the same kernel source, dn_cloud_lap.hip): the local-Delaunay Laplacian and mass of a point cloud through the
C ABI, ``ops.cloud_laplacian`` and ``geometry.point_cloud_laplacian`` on host buffers -- the lane-group map, the pivot and its check, the
fixed emission offsets, the run sums after the stable sort, the status word, the error returns.  Bodies in cloud_lap_cases.py."""
import os
import shutil
import subprocess

import pytest

import cloud_lap_cases

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


@pytest.mark.parametrize("n,k,seed,kind", cloud_lap_cases.CASES)
def test_case_on_emulator(emu, n, k, seed, kind):
    cloud_lap_cases.run_case(emu, n, k, seed, kind)


def test_one_neighbour_gives_no_triangle_on_emulator(emu):
    cloud_lap_cases.run_k1(emu)


def test_two_neighbours_on_emulator(emu):
    cloud_lap_cases.run_k2(emu)


def test_given_frames_on_emulator(emu):
    cloud_lap_cases.run_given_frames(emu)


@pytest.mark.parametrize("name", cloud_lap_cases.DEGENERATE)
def test_degenerate_input_on_emulator(emu, name):
    cloud_lap_cases.run_degenerate(emu, name)


def test_own_and_out_of_range_indices_on_emulator(emu):
    cloud_lap_cases.run_bad_indices(emu)


def test_ops_validation_on_emulator(emu):
    cloud_lap_cases.run_ops_validation(emu)


def test_sparse_laplacian_equals_the_raw_csr_on_emulator(emu):
    cloud_lap_cases.run_sparse_equals_raw(emu)


def test_abi_errors_on_emulator(emu):
    cloud_lap_cases.run_abi_errors()


def test_custom_operator_is_registered_with_a_fake_kernel(emu):
    import torch
    from diffusion_net import torchlib  # noqa: F401
    t, nbr, fr = cloud_lap_cases.inputs(emu, cloud_lap_cases.sample(40, 1), 6)
    got = torch.ops.diffusion_net.cloud_laplacian(t, nbr, fr)
    want = cloud_lap_cases.run(t, nbr, fr)
    for a, key in zip(got, ("partner", "rowptr", "col", "val", "mass")):
        assert torch.equal(a, torch.from_numpy(want[key])), key
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    with FakeTensorMode(shape_env=ShapeEnv(), allow_non_fake_inputs=False) as mode:
        fake = torch.ops.diffusion_net.cloud_laplacian(mode.from_tensor(t), mode.from_tensor(nbr), mode.from_tensor(fr))
    assert tuple(fake[0].shape) == (40, 6) and fake[0].dtype == torch.int32 and tuple(fake[1].shape) == (41,)
    assert fake[2].dtype == torch.int32 and fake[3].dtype == torch.float32 and fake[2].dim() == 1 and tuple(fake[4].shape) == (40,)

"""CPU tier (emulator build of the same kernel source, dn_cloud.hip): normals, tangent frames and gradient stencils of a point cloud through
the C ABI, ``ops.cloud_operators`` and ``geometry.cloud_operators`` on host buffers -- the lane-group map, the Jacobi eigen-solve, the sign
rule, rank-deficient neighbourhoods, the status word, the error returns.  Bodies in cloud_cases.py."""
import os
import shutil
import subprocess

import pytest

import cloud_cases

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


@pytest.mark.parametrize("N,k,seed,axes,noise", cloud_cases.CASES)
def test_case_on_emulator(emu, N, k, seed, axes, noise):
    cloud_cases.run_case(emu, N, k, seed, axes, noise)


def test_reference_fixture_on_emulator(emu):
    cloud_cases.run_reference_fixture(emu)


def test_single_point_is_rejected_on_emulator(emu):
    cloud_cases.run_single_point_is_rejected(emu)


def test_given_normals_on_emulator(emu):
    cloud_cases.run_given_normals(emu)


def test_sparse_operators_equal_the_raw_rows_on_emulator(emu):
    cloud_cases.run_sparse_equals_raw(emu)


def test_collinear_and_coincident_points_on_emulator(emu):
    cloud_cases.run_collinear(emu)


def test_duplicate_points_on_emulator(emu):
    cloud_cases.run_duplicates(emu)


def test_own_and_out_of_range_indices_on_emulator(emu):
    cloud_cases.run_bad_indices(emu)


def test_ops_validation_on_emulator(emu):
    cloud_cases.run_ops_validation(emu)


def test_abi_errors_on_emulator(emu):
    cloud_cases.run_abi_errors()

"""CPU tier (emulator build of the same kernel source, dn_knn.hip): the exact k-nearest-neighbour search through the C ABI and ``ops.knn`` on
host buffers -- tile and slice maps, the k = 1 path, list insertion, the merge kernel, the tie rule, the error returns.  Bodies in knn_cases.py."""
import os
import shutil
import subprocess

import pytest

import knn_cases

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


@pytest.mark.parametrize("N,M,D,k,flags", knn_cases.CASES)
def test_case_on_emulator(emu, N, M, D, k, flags):
    knn_cases.run_case(emu, N, M, D, k, flags)


@pytest.mark.parametrize("D,k,largest", [(3, 30, False), (30, 30, False), (30, 3, True), (30, 1, False)])
def test_split_and_merge_on_emulator(emu, D, k, largest):
    knn_cases.run_splits(emu, D, k, largest)


def test_exact_ties_on_emulator(emu):
    knn_cases.run_exact_ties(emu)


def test_duplicates_on_emulator(emu):
    knn_cases.run_duplicates(emu)


def test_reference_fixture_on_emulator(emu):
    knn_cases.run_reference_fixture(emu)


def test_abi_errors_on_emulator(emu):
    knn_cases.run_abi_errors()

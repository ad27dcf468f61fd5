"""CPU tier (emulator build of the same kernel source, dn_knn_grid.hip): the cell-grid k-nearest-neighbour search through the C ABI and
``ops.knn_grid`` on host buffers -- cell keys, shells, the closing rule, the scan fallback, the (key, index) insertion, the error returns --
against ``ops.knn`` bit for bit and against fp64 brute force.  Bodies in knn_grid_cases.py; shapes stay at or below 1 500 points."""
import os
import shutil
import subprocess

import pytest

import knn_grid_cases

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


@pytest.mark.parametrize("N,M,D,k,flags", knn_grid_cases.CASES)
def test_case_on_emulator(emu, N, M, D, k, flags):
    knn_grid_cases.run_case(emu, N, M, D, k, flags)


def test_exact_ties_on_emulator(emu):
    knn_grid_cases.run_exact_ties(emu)


def test_duplicates_zero_extent_and_collinear_on_emulator(emu):
    knn_grid_cases.run_duplicates(emu)


def test_clusters_and_outlier_close_without_a_scan_on_emulator(emu):
    knn_grid_cases.run_clusters(emu)


def test_cross_query_scans_on_emulator(emu):
    knn_grid_cases.run_cross(emu)


def test_second_run_gives_the_same_bits_on_emulator(emu):
    knn_grid_cases.run_repeat(emu)


def test_non_finite_input_returns_valid_indices_on_emulator(emu):
    knn_grid_cases.run_non_finite(emu)


def test_pipeline_routes_agree_on_emulator(emu, monkeypatch):
    knn_grid_cases.run_pipeline(emu, monkeypatch)


def test_abi_errors_on_emulator(emu):
    knn_grid_cases.run_abi_errors()

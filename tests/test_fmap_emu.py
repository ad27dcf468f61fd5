"""CPU tier (emulator build of the same kernel source, dn_fmap.hip): the regularised spectral solve of the functional-map layer through the C
ABI and ``ops.fmap_solve`` on host buffers -- the gram tiles, the packed Cholesky, both substitutions, the closed-form backward, the NaN rule
of a singular row, the error returns.  Bodies in fmap_cases.py."""
import os
import shutil
import subprocess

import pytest

import fmap_cases

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


@pytest.mark.parametrize("K,F,P", fmap_cases.CASES)
def test_case_on_emulator(emu, K, F, P):
    fmap_cases.run_case(emu, K, F, P)


def test_determinism_on_emulator(emu):
    fmap_cases.run_determinism(emu)


def test_singular_row_on_emulator(emu):
    fmap_cases.run_singular_row(emu)


def test_limits_and_errors_on_emulator(emu):
    fmap_cases.run_limits(emu)


def test_reference_fixture_on_emulator(emu):
    """torch projections on the host, the solve on the emulated kernels."""
    fmap_cases.run_reference_fixture(emu, "ops", names=("k1_f1", "k5_f3", "k30_f128", "k30_f16", "k30_f128_rank8", "k31_f40", "k64_f70"))


def test_abi_errors_on_emulator(emu):
    fmap_cases.run_abi_errors()

"""CPU tier (emulator build of the same kernel sources): the CSR gathers on an operator with long, empty and hub rows -- ``spmm_kernel`` as an
isolated op against fp64, packing and the norm word, the gather forms of the chained forward, ``sg_grad_kernel``, a cloud's operators through
forward + backward, and the isolation of a non-finite value inside its mesh.  Bodies and criteria in sparse_cases.py.

DN_SP_COOP -- the cooperative index fetch of ``spmm_kernel`` -- is compiled out of the emulator build (its shuffles sit in a loop whose trip
count differs between the row groups of a wave): the cases whose route is cooperative run the every-lane-loads form here, and only
test_sparse_gpu.py reaches the shuffles.  The generator and the case table are checked with no library at all."""
import os
import shutil
import subprocess

import pytest

import sparse_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-net_amd", "csrc")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libdiffnet_emu.so")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"

needs_emulator = pytest.mark.skipif(not (os.path.exists(HOSTCXX) and shutil.which("make")), reason="host clang++/make not available")
case_id = lambda c: "%d%s" % (c[0], "-misaligned" if c[1] else "")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", CSRC, "-j8", "emu"], check=True, capture_output=True)
    from diffusion_net import _hip
    _hip._use_library_for_tests(EMU_SO, True)
    yield "cpu"
    _hip._use_library_for_tests(None, False)


def test_generator_places_every_feature():
    sparse_cases.check_operator()


def test_case_table_reaches_every_instantiation():
    sparse_cases.check_case_table()


@needs_emulator
@pytest.mark.parametrize("case", sparse_cases.CASES, ids=case_id)
def test_gather_on_emulator(emu, case):
    sparse_cases.run_case(emu, *case)


@needs_emulator
def test_packing_on_emulator(emu):
    sparse_cases.run_packing(emu)


@needs_emulator
def test_norm_word_on_emulator(emu):
    sparse_cases.run_norm_word(emu)


@needs_emulator
def test_determinism_on_emulator(emu):
    sparse_cases.run_determinism(emu)


# (the C = K = 256 form takes minutes through forward + backward here: its gather runs in the saved-gather test below, the rest on the device)
@needs_emulator
@pytest.mark.parametrize("form", [f for f in sparse_cases.FORMS if f != "c256_rolling"])
def test_chain_vs_unfused_on_emulator(emu, form):
    sparse_cases.run_chain_form(emu, form)


@needs_emulator
def test_spectral_vs_gather_on_emulator(emu):
    sparse_cases.run_spectral_form(emu)


@needs_emulator
@pytest.mark.parametrize("form", list(sparse_cases.FORMS))
def test_saved_gather_is_spmm_bit_for_bit_on_emulator(emu, form):
    sparse_cases.run_saved_gather_bitwise(emu, form)


@needs_emulator
def test_cloud_forward_backward_on_emulator(emu):
    sparse_cases.run_cloud_backward(emu)


# (planted in mesh 0, which entry 0 of the pattern points into; the device tier plants it in either mesh)
@needs_emulator
@pytest.mark.parametrize("route", list(sparse_cases.ISOLATION_ROUTES))
def test_nan_stays_in_its_mesh_on_emulator(emu, route):
    sparse_cases.run_nan_isolation(emu, route, 0)

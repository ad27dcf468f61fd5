"""CPU tier (emulator build of the same kernel source, dn_mesh.hip): the operators of a triangle mesh through the C ABI, ``ops.mesh_assemble``,
``ops.mesh_frames_gradients``, ``geometry.mesh_operators`` and ``compute_operators_via(..., assembly="device")`` on host buffers -- the
face pass and its staged stores, the run sums after the stable sort, the vertex pass, the status words, the error returns.  Bodies and
bounds in mesh_cases.py."""
import os
import shutil
import subprocess

import pytest

import mesh_cases

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


@pytest.mark.parametrize("name", mesh_cases.CASES + mesh_cases.DEGENERATE + mesh_cases.FALLBACK)
def test_case_on_emulator(emu, name):
    mesh_cases.check(emu, name)


@pytest.mark.parametrize("name", mesh_cases.CASES + mesh_cases.DEGENERATE + mesh_cases.FALLBACK)
def test_mesh_operators_on_emulator(emu, name):
    mesh_cases.check_mesh_operators(emu, name)


def test_empty_inputs_on_emulator(emu):
    mesh_cases.run_empty(emu)


def test_out_of_range_indices_on_emulator(emu):
    mesh_cases.run_bad_indices(emu)


def test_ops_validation_on_emulator(emu):
    mesh_cases.run_ops_validation(emu)


def test_abi_errors_on_emulator(emu):
    mesh_cases.run_abi_errors()


def test_custom_operators_are_registered_with_fake_kernels(emu):
    mesh_cases.run_library_ops(emu)


@pytest.mark.parametrize("eigensolver", [None, "subspace"])
def test_compute_operators_with_device_assembly_on_emulator(emu, eigensolver, monkeypatch):
    from diffusion_net import ops
    calls = []
    real = ops.mesh_assemble
    monkeypatch.setattr(ops, "mesh_assemble", lambda *a: calls.append(1) or real(*a))
    mesh_cases.run_compute_operators(emu, eigensolver)
    assert calls                                                 # the kernels assembled it, not the host route


def test_cache_round_trip_and_bad_values_on_emulator(emu, tmp_path):
    mesh_cases.run_cache_round_trip(emu, tmp_path)

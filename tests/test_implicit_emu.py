"""CPU tier (emulator build of the same kernel source, dn_implicit.hip): the per-channel conjugate-gradient solve through the C ABI,
``ops.implicit_solve``, ``ops.ImplicitDiffusionFn``, the custom operator, ``LearnedTimeDiffusion`` and ``DiffusionNet`` with
``"implicit_sparse"`` on host buffers, against the fp64 dense solve.  Bodies and criteria in implicit_cases.py."""
import os
import shutil
import subprocess

import pytest

import implicit_cases as ic

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


@pytest.mark.parametrize("name", ic.FAMILIES)
def test_families_on_emulator(emu, name):
    ic.run_family(name, emu)


@pytest.mark.parametrize("C", ic.WIDTHS)
def test_widths_on_emulator(emu, C):
    ic.run_family("small", emu, C)


def test_one_vertex_on_emulator(emu):
    ic.run_family("v1", emu)


@pytest.mark.parametrize("name", ["sphere300", "sphere300_mass6", "graph200", "ragged"])
def test_iteration_counts_match_the_numpy_route_on_emulator(emu, name):
    ic.run_iteration_counts(name, emu)


def test_call_forms_on_emulator(emu):
    ic.run_call_forms(emu)


def test_max_iter_reached_raises_on_emulator(emu):
    ic.run_max_iter_raises(emu)


def test_isolation_on_emulator(emu):
    ic.run_isolation(emu)


@pytest.mark.parametrize("name,C", [("sphere300", 5), ("sphere300_mass6", 5), ("graph200", 5), ("small", 65)])
def test_backward_on_emulator(emu, name, C):
    ic.run_backward(name, emu, C)


def test_custom_operator_on_emulator(emu):
    ic.run_custom_operator(emu)


def test_refused_calls_on_emulator(emu):
    ic.run_refused_calls(emu)


def test_op_errors_on_emulator(emu):
    ic.run_op_errors(emu)


def test_layer_on_emulator(emu):
    ic.run_layer(emu)


def test_network_on_emulator(emu):
    ic.run_network(emu)

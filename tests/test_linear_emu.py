"""CPU tier (emulator build of the same kernel sources): every route of the nn.Linear entry points and ``hks_kernel`` off its tile sizes, as
isolated ops against fp64 -- condition-scaled error, the magnitude words bit for bit, misaligned operands.  The case table itself is
checked against a restatement of the dispatch with no library at all.  Bodies in linear_cases.py."""
import os
import shutil
import subprocess

import pytest

import linear_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-net_amd", "csrc")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libdiffnet_emu.so")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"

needs_emulator = pytest.mark.skipif(not (os.path.exists(HOSTCXX) and shutil.which("make")), reason="host clang++/make not available")
case_id = lambda c: "%dx%d-%d-%d%s" % (c[0][0], c[0][1], c[1], c[2], c[3] and "-" + c[3])


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", CSRC, "-j8", "emu"], check=True, capture_output=True)
    from diffusion_net import _hip
    _hip._use_library_for_tests(EMU_SO, True)
    yield "cpu"
    _hip._use_library_for_tests(None, False)


def test_case_table_reaches_every_route_and_both_sides_of_every_bound():
    linear_cases.check_case_table()


@needs_emulator
@pytest.mark.parametrize("case", linear_cases.CASES, ids=case_id)
def test_route_on_emulator(emu, case):
    linear_cases.run_case(emu, *case)


@needs_emulator
@pytest.mark.parametrize("log2_scale", linear_cases.WORD_SCALES)
@pytest.mark.parametrize("where", linear_cases.WORD_PLACES)
@pytest.mark.parametrize("sizes,thin,wide", linear_cases.WORD_WIDTHS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
@pytest.mark.parametrize("passname", ["fwd", "bwd"])
def test_magnitude_word_on_emulator(emu, passname, sizes, thin, wide, where, log2_scale):
    linear_cases.run_word(emu, passname, sizes, thin, wide, where, log2_scale)


@needs_emulator
def test_unaligned_out_on_emulator(emu):
    linear_cases.run_unaligned_out(emu)


@needs_emulator
def test_exact_workspace_many_chunks_on_emulator(emu):
    linear_cases.run_exact_workspace_many_chunks(emu)


@needs_emulator
@pytest.mark.parametrize("B,V,K,S,per_batch", linear_cases.HKS_CASES)
def test_hks_on_emulator(emu, B, V, K, S, per_batch):
    linear_cases.run_hks(emu, B, V, K, S, per_batch)

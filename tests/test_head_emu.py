"""CPU tier (emulator build of the same kernel sources): the fused head of dn_head.hip, the mass-weighted mean and the content checksum as
isolated ops -- condition-scaled error against fp64 in every instantiation, non-finite and extreme inputs against torch, determinism, the
checksum against its integer model.  The case table and the gather pattern are checked with no library at all.  Bodies and criteria in
head_cases.py.

The three striding cases take 45 of this file's 65 seconds, so the 66 000-row stride of the eight-lane groups runs in test_head_gpu.py
only, and the determinism of a striding call is checked here on the backward's stride, on the device also on the forward's."""
import os
import shutil
import subprocess

import pytest

import head_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-net_amd", "csrc")
EMU_SO = os.path.join(ROOT, "tests", "emu", "_build", "libdiffnet_emu.so")
HOSTCXX = "/opt/rocm/lib/llvm/bin/clang++"

needs_emulator = pytest.mark.skipif(not (os.path.exists(HOSTCXX) and shutil.which("make")), reason="host clang++/make not available")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", CSRC, "-j8", "emu"], check=True, capture_output=True)
    from diffusion_net import _hip
    _hip._use_library_for_tests(EMU_SO, True)
    yield "cpu"
    _hip._use_library_for_tests(None, False)


def test_case_table_reaches_every_instantiation_and_both_sides_of_every_boundary():
    head_cases.check_case_table()


def test_pattern_places_every_feature():
    head_cases.check_pattern()


def test_checksum_model_is_position_and_salt_dependent():
    a = head_cases.checksum_model([1, 2, 3], 5)
    assert a != head_cases.checksum_model([2, 1, 3], 5) and a != head_cases.checksum_model([1, 2, 3], 9) and a[0] != a[1]
    assert head_cases.checksum_model([], 5) == (0, 0) and all(0 <= v < 2 ** 64 for v in a)


@needs_emulator
@pytest.mark.parametrize("case", head_cases.CASES + head_cases.STRIDE_CASES, ids=head_cases.case_id)
def test_head_on_emulator(emu, case):
    head_cases.run_case(emu, case)


@needs_emulator
@pytest.mark.parametrize("route", ["head", "head_faces", "nll"])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_masked_class_on_emulator(emu, C, route):
    head_cases.run_masked_class(emu, C, route)


@needs_emulator
def test_nll_of_log_zero_on_emulator(emu):
    head_cases.run_nll_of_log_zero(emu)


@needs_emulator
@pytest.mark.parametrize("target", [0, 1, 2])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_extreme_row_on_emulator(emu, C, target):
    head_cases.run_extreme_row(emu, C, target)


@needs_emulator
@pytest.mark.parametrize("lsm", [True, False], ids=["logit", "given"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_target_masked_on_emulator(emu, C, smoothing, lsm):
    head_cases.run_target_masked(emu, C, smoothing, lsm)


@needs_emulator
@pytest.mark.parametrize("gather", ["none", "faces"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_poisoned_logit_on_emulator(emu, C, value, gather):
    head_cases.run_poison(emu, C, value, gather)


@needs_emulator
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_nan_in_ignored_row_on_emulator(emu, C):
    head_cases.run_nan_in_ignored_row(emu, C)


@needs_emulator
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_all_rows_ignored_on_emulator(emu, C):
    head_cases.run_all_ignored(emu, C)


@needs_emulator
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("gather", ["none", "faces"])
def test_single_class_on_emulator(emu, gather, smoothing):
    head_cases.run_single_class(emu, gather, smoothing)


@needs_emulator
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_denormal_logits_on_emulator(emu, C):
    head_cases.run_denormal(emu, C)


@needs_emulator
@pytest.mark.parametrize("via", ["head", "nll"])
@pytest.mark.parametrize("bad", head_cases.BAD_LABELS, ids=str)
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_bad_label_on_emulator(emu, C, bad, via):
    head_cases.run_bad_label(emu, C, bad, via)


@needs_emulator
@pytest.mark.parametrize("which", ["faces", "stride_bwd_cap"])
def test_determinism_on_emulator(emu, which):
    head_cases.run_determinism(emu, which)


@needs_emulator
@pytest.mark.parametrize("C", head_cases.MM_C)
def test_mass_mean_on_emulator(emu, C):
    head_cases.run_mass_mean(emu, C)


@needs_emulator
@pytest.mark.parametrize("offset", head_cases.CK_OFFSETS)
@pytest.mark.parametrize("n", head_cases.CK_LENGTHS)
def test_checksum_on_emulator(emu, n, offset):
    head_cases.run_checksum_single(emu, n, offset)


@needs_emulator
@pytest.mark.parametrize("offset", head_cases.CK_OFFSETS)
def test_checksum_multi_on_emulator(emu, offset):
    head_cases.run_checksum_multi(emu, offset)

"""GPU tier: the fused head of dn_head.hip in every instantiation, the mass-weighted mean and the content checksum on the device, as isolated
ops -- condition-scaled error against fp64, non-finite and extreme inputs against torch, determinism, the checksum against its integer model.
Bodies and criteria in head_cases.py; every case leaves a ``head_ops`` or ``mass_mean`` record in the margins file."""
import os

import pytest
import torch

import head_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    _hip.lib()                            # raises if libdiffnet_hip.so is missing: no fallback
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", head_cases.CASES + head_cases.STRIDE_CASES + head_cases.GPU_ONLY_CASES, ids=head_cases.case_id)
def test_head(dev, case):
    head_cases.run_case(dev, case)


@pytest.mark.parametrize("route", ["head", "head_faces", "nll"])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_masked_class(dev, C, route):
    head_cases.run_masked_class(dev, C, route)


def test_nll_of_log_zero(dev):
    head_cases.run_nll_of_log_zero(dev)


@pytest.mark.parametrize("target", [0, 1, 2])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_extreme_row(dev, C, target):
    head_cases.run_extreme_row(dev, C, target)


@pytest.mark.parametrize("lsm", [True, False], ids=["logit", "given"])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_target_masked(dev, C, smoothing, lsm):
    head_cases.run_target_masked(dev, C, smoothing, lsm)


@pytest.mark.parametrize("gather", ["none", "faces"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_poisoned_logit(dev, C, value, gather):
    head_cases.run_poison(dev, C, value, gather)


@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_nan_in_ignored_row(dev, C):
    head_cases.run_nan_in_ignored_row(dev, C)


@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_all_rows_ignored(dev, C):
    head_cases.run_all_ignored(dev, C)


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("gather", ["none", "faces"])
def test_single_class(dev, gather, smoothing):
    head_cases.run_single_class(dev, gather, smoothing)


@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_denormal_logits(dev, C):
    head_cases.run_denormal(dev, C)


@pytest.mark.parametrize("via", ["head", "nll"])
@pytest.mark.parametrize("bad", head_cases.BAD_LABELS, ids=str)
@pytest.mark.parametrize("C", head_cases.NONFINITE_C)
def test_bad_label(dev, C, bad, via):
    head_cases.run_bad_label(dev, C, bad, via)


@pytest.mark.parametrize("which", list(head_cases.DETERMINISM_CASES))
def test_determinism(dev, which):
    head_cases.run_determinism(dev, which)


@pytest.mark.parametrize("C", head_cases.MM_C)
def test_mass_mean(dev, C):
    head_cases.run_mass_mean(dev, C)


@pytest.mark.parametrize("offset", head_cases.CK_OFFSETS)
@pytest.mark.parametrize("n", head_cases.CK_LENGTHS)
def test_checksum(dev, n, offset):
    head_cases.run_checksum_single(dev, n, offset)


@pytest.mark.parametrize("offset", head_cases.CK_OFFSETS)
def test_checksum_multi(dev, offset):
    head_cases.run_checksum_multi(dev, offset)

"""GPU tier: every route of the nn.Linear entry points (dn_api.hip: smallk_rows, thin_tn, smalln_tn, the row GEMM and the split-V products) and
``hks_kernel`` off its tile sizes on the device, as isolated ops against fp64 -- condition-scaled error, the magnitude words bit for bit,
misaligned operands.  Bodies and criteria in linear_cases.py; every case leaves a ``linear_routes`` record in the margins file."""
import os

import pytest
import torch

import linear_cases

pytestmark = pytest.mark.gpu
case_id = lambda c: "%dx%d-%d-%d%s" % (c[0][0], c[0][1], c[1], c[2], c[3] and "-" + c[3])


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


@pytest.mark.parametrize("case", linear_cases.CASES, ids=case_id)
def test_route(dev, case):
    linear_cases.run_case(dev, *case)


@pytest.mark.parametrize("log2_scale", linear_cases.WORD_SCALES)
@pytest.mark.parametrize("where", linear_cases.WORD_PLACES)
@pytest.mark.parametrize("sizes,thin,wide", linear_cases.WORD_WIDTHS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
@pytest.mark.parametrize("passname", ["fwd", "bwd"])
def test_magnitude_word(dev, passname, sizes, thin, wide, where, log2_scale):
    linear_cases.run_word(dev, passname, sizes, thin, wide, where, log2_scale)


def test_unaligned_out(dev):
    linear_cases.run_unaligned_out(dev)


def test_exact_workspace_many_chunks(dev):
    linear_cases.run_exact_workspace_many_chunks(dev)


@pytest.mark.parametrize("B,V,K,S,per_batch", linear_cases.HKS_CASES)
def test_hks(dev, B, V, K, S, per_batch):
    linear_cases.run_hks(dev, B, V, K, S, per_batch)

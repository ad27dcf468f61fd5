"""GPU tier: the CSR gathers on an operator with long, empty and hub rows, on the device -- every instantiation of ``spmm_kernel`` (the
cooperative index fetch, DN_SP_COOP, exists in this build only) as an isolated op against fp64, packing and the norm word, the gather forms of
the chained forward and their saved gx / gy bit for bit, ``sg_grad_kernel``, a cloud's operators through forward + backward, and the isolation of
a non-finite value inside its mesh.  Bodies and criteria in sparse_cases.py; every gather case leaves a ``sparse_irregular`` record in the
margins file."""
import os

import pytest
import torch

import sparse_cases

pytestmark = pytest.mark.gpu
case_id = lambda c: "%d%s" % (c[0], "-misaligned" if c[1] else "")


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


@pytest.mark.parametrize("case", sparse_cases.CASES, ids=case_id)
def test_gather(dev, case):
    sparse_cases.run_case(dev, *case)


def test_packing(dev):
    sparse_cases.run_packing(dev)


def test_norm_word(dev):
    sparse_cases.run_norm_word(dev)


def test_determinism(dev):
    sparse_cases.run_determinism(dev)


@pytest.mark.parametrize("form", list(sparse_cases.FORMS))
def test_chain_vs_unfused(dev, form):
    sparse_cases.run_chain_form(dev, form)


def test_spectral_vs_gather(dev):
    sparse_cases.run_spectral_form(dev)


@pytest.mark.parametrize("form", list(sparse_cases.FORMS))
def test_saved_gather_is_spmm_bit_for_bit(dev, form):
    sparse_cases.run_saved_gather_bitwise(dev, form)


def test_cloud_forward_backward(dev):
    sparse_cases.run_cloud_backward(dev)


@pytest.mark.parametrize("planted", [0, 1])
@pytest.mark.parametrize("route", list(sparse_cases.ISOLATION_ROUTES))
def test_nan_stays_in_its_mesh(dev, route, planted):
    sparse_cases.run_nan_isolation(dev, route, planted)

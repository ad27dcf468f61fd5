"""GPU tier: the exact k-nearest-neighbour search (dn_knn.hip) on the device -- the shared cases of knn_cases.py, two workload-shaped runs,
``geometry.find_knn`` on device tensors (kernel route for both methods, torch route past the kernel's limits) and the registered operator
under ``torch.compile``."""
import os

import pytest
import torch

import knn_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tier needs a ROCm device"
    from diffusion_net import _hip
    _hip._use_library_for_tests(None, False)
    if not os.path.exists(_hip.LIB_PATH):  # fresh checkout on the GPU box: compile the HIP sources
        import __graft_entry__
        __graft_entry__.build()
    lib = _hip.lib()                      # raises if libdiffnet_hip.so is missing: no fallback
    assert lib.dn_knn_max_k() == 32
    return torch.device("cuda:0")


@pytest.mark.parametrize("N,M,D,k,flags", knn_cases.CASES)
def test_case(dev, N, M, D, k, flags):
    knn_cases.run_case(dev, N, M, D, k, flags)


@pytest.mark.parametrize("D,k,largest", [(3, 30, False), (30, 30, False), (30, 3, True), (30, 1, False)])
def test_split_and_merge(dev, D, k, largest):
    knn_cases.run_splits(dev, D, k, largest)


def test_exact_ties(dev):
    knn_cases.run_exact_ties(dev)


def test_duplicates(dev):
    knn_cases.run_duplicates(dev)


def test_reference_fixture(dev):
    knn_cases.run_reference_fixture(dev)


@pytest.mark.parametrize("N,D,k,omit", [(6890, 30, 1, False), (10000, 3, 30, True)])
def test_workload_shapes(dev, N, D, k, omit):
    """The FAUST evaluation (nearest neighbour in the 30-dimensional spectral embedding) and the neighbourhood query of a 10 000-point
    cloud, against fp64 brute force on the device; the library's own choice of slices, and one slice, give the same bits."""
    from diffusion_net import ops
    g = torch.Generator().manual_seed(21)
    src = torch.randn(N, D, generator=g).to(dev)
    tgt = src if omit else torch.randn(N, D, generator=g).to(dev)
    got = ops.knn(src, tgt, k, omit_diagonal=omit)
    one = ops.knn(src, tgt, k, omit_diagonal=omit, n_split=1)
    assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    knn_cases.check_knn_on_device(src, tgt, k, False, omit, got)


def test_find_knn_on_device_is_the_kernel_for_both_methods(dev):
    """The line the functional-correspondence evaluation runs: device tensors, method='cpu_kd', a column slice of a wider eigenbasis."""
    import diffusion_net
    from diffusion_net import ops
    g = torch.Generator().manual_seed(22)
    evec2 = torch.randn(700, 128, generator=g).to(dev)
    evec1_on_2 = torch.randn(650, 30, generator=g).to(dev)
    want = ops.knn(evec2[:, :30], evec1_on_2, 1)
    for method in ("cpu_kd", "brute"):
        got = diffusion_net.geometry.find_knn(evec2[:, :30], evec1_on_2, k=1, method=method)
        assert got.values.is_cuda and torch.equal(got.values, want[0]) and torch.equal(got.indices, want[1])
        vals, inds = got
        assert vals is got.values and inds is got.indices
    pts = torch.randn(500, 3, generator=g).to(dev)
    want = ops.knn(pts, pts, 30, omit_diagonal=True)
    got = diffusion_net.find_knn(pts, pts, 30, omit_diagonal=True, method="cpu_kd")
    assert torch.equal(got.values, want[0]) and torch.equal(got.indices, want[1])


def test_torch_route_past_the_kernel_limits(dev):
    import diffusion_net
    src, tgt = knn_cases.inputs(300, 400, 5, False, 23)
    got = diffusion_net.find_knn(src.to(dev), tgt.to(dev), 40)                     # k > 32
    knn_cases.check_knn(src, tgt, 40, False, False, (got.values, got.indices))
    a = src.to(dev).requires_grad_(True)
    got = diffusion_net.find_knn(a, tgt.to(dev), 6)                                # differentiable, as the reference's 'brute' branch
    knn_cases.check_knn(src, tgt, 6, False, False, (got.values, got.indices))
    got.values.sum().backward()
    assert a.grad is not None and bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().sum()) > 0
    got = diffusion_net.find_knn(src.double().to(dev), tgt.double().to(dev), 6)    # another dtype
    assert got.values.dtype == torch.float64 and torch.equal(got.indices.cpu(), knn_cases._knn(dev, src, tgt, 6)[1])


def test_torch_route_at_workload_size(dev):
    """The torch route in more than one row block, at the FAUST shape (47 million pairs), against fp64 brute force."""
    import diffusion_net
    g = torch.Generator().manual_seed(25)
    src, tgt = torch.randn(6890, 30, generator=g).to(dev), torch.randn(6890, 30, generator=g).to(dev)
    got = diffusion_net.find_knn(src, tgt, 40)
    knn_cases.check_knn_on_device(src, tgt, 40, False, False, (got.values, got.indices))


def test_registered_operator_under_torch_compile(dev):
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn)
    src, tgt = knn_cases.inputs(300, 400, 30, False, 24)
    src, tgt = src.to(dev), tgt.to(dev)

    def f(a, b):
        d, i = torch.ops.diffusion_net.knn(a * 1.0, b, 4, False, False)
        return d + 0.0, i

    eager = f(src, tgt)
    compiled = torch.compile(f, fullgraph=True)(src, tgt)
    assert torch.equal(compiled[0], eager[0]) and torch.equal(compiled[1], eager[1])
    knn_cases.check_knn(src.cpu(), tgt.cpu(), 4, False, False, eager)

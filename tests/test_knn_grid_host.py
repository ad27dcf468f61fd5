"""CPU tier, no kernel: what ``method='grid'`` does to ``geometry.find_knn`` on host tensors, the errors of ``ops.knn_grid`` that are raised
before any launch, the registered operator's fake kernel, and the binding."""
import pytest
import torch

import diffusion_net
from diffusion_net import _hip, geometry, ops


def test_grid_on_host_tensors_is_the_brute_route():
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(40, 3, generator=g), torch.randn(60, 3, generator=g)
    want = geometry.find_knn(a, b, 5, method="brute")
    got = geometry.find_knn(a, b, 5, method="grid")
    assert torch.equal(got.values, want.values) and torch.equal(got.indices, want.indices)
    want = geometry.find_knn(a, a, 4, omit_diagonal=True)
    got = geometry.find_knn(a, a, 4, omit_diagonal=True, method="grid")
    assert torch.equal(got.values, want.values) and torch.equal(got.indices, want.indices)


def test_method_errors():
    a, b = torch.randn(5, 3), torch.randn(6, 3)
    with pytest.raises(ValueError, match="largest"):
        geometry.find_knn(a, b, 2, largest=True, method="grid")
    with pytest.raises(ValueError, match="unrecognized method"):
        geometry.find_knn(a, b, 2, method="ball_tree")
    with pytest.raises(ValueError, match="omit_diagonal"):
        geometry.find_knn(a, b, 2, omit_diagonal=True, method="grid")


def test_ops_knn_grid_needs_a_device():
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.knn_grid(torch.randn(5, 3), torch.randn(6, 3), 2)


def test_pipeline_threshold_is_a_module_constant():
    assert geometry.KNN_GRID_MIN_POINTS is None or isinstance(geometry.KNN_GRID_MIN_POINTS, int)
    assert callable(geometry._cloud_self_knn)


def test_fake_kernel_and_binding():
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn_grid)
    d, i = torch.ops.diffusion_net.knn_grid(torch.empty(7, 3, device="meta"), torch.empty(9, 3, device="meta"), 4, False, 0)
    assert tuple(d.shape) == (7, 4) and d.dtype == torch.float32 and tuple(i.shape) == (7, 4) and i.dtype == torch.int64
    for name in ("dn_knn_grid_cells", "dn_knn_grid_cell_budget", "dn_knn_grid_workspace_bytes", "dn_knn_grid_keys_f32", "dn_knn_grid_search_f32"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert diffusion_net.find_knn is geometry.find_knn

"""CPU tier: the host routes of ``geometry.find_knn`` (torch 'brute', sklearn 'cpu_kd') against the reference's recorded outputs
(tests/golden/geom_knn_ref.npz), its ValueErrors, and where the name resolves."""
import pytest
import torch

import diffusion_net
import knn_cases


@pytest.mark.parametrize("method", ["brute", "cpu_kd"])
def test_host_routes_match_the_reference(method):
    ran = 0
    for name, src, tgt, k, largest, omit, ref in knn_cases.golden_cases():
        if method not in ref:
            continue
        got = diffusion_net.geometry.find_knn(src, tgt, k, largest=largest, omit_diagonal=omit, method=method)
        assert got.values is got[0] and got.indices is got[1]
        vals, inds = got                                       # both call styles of the reference's users
        knn_cases.check_against_reference(src, tgt, k, largest, omit, (vals, inds), {method: ref[method]})
        ran += 1
    assert ran == (4 if method == "brute" else 3)


def test_value_errors_of_the_reference():
    a, b = torch.randn(10, 3), torch.randn(8, 3)
    with pytest.raises(ValueError, match="omit_diagonal can only be used when source and target are same shape"):
        diffusion_net.geometry.find_knn(a, b, 2, omit_diagonal=True)
    with pytest.raises(ValueError, match="can't do largest with cpu_kd"):
        diffusion_net.geometry.find_knn(a, b, 2, largest=True, method="cpu_kd")
    with pytest.raises(ValueError, match="unrecognized method"):
        diffusion_net.geometry.find_knn(a, b, 2, method="ball_tree")


def test_points_on_two_devices_are_refused_up_front():
    a, b = torch.randn(10, 3), torch.randn(8, 3, device="meta")
    with pytest.raises(RuntimeError, match="source points on cpu, target points on meta"):
        diffusion_net.geometry.find_knn(a, b, 2)


def test_fake_kernel_of_the_registered_operator_is_fp32():
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn)
    for dt in (torch.float32, torch.float64):
        d, i = torch.ops.diffusion_net.knn(torch.empty(7, 3, dtype=dt, device="meta"), torch.empty(9, 3, dtype=dt, device="meta"), 4, False, False)
        assert d.shape == (7, 4) and d.dtype == torch.float32 and i.shape == (7, 4) and i.dtype == torch.int64


def test_find_knn_resolves_on_the_package():
    assert callable(diffusion_net.geometry.find_knn)
    assert diffusion_net.find_knn is diffusion_net.geometry.find_knn


def test_host_brute_is_differentiable():
    a = torch.randn(20, 3, requires_grad=True)
    vals, _ = diffusion_net.find_knn(a, torch.randn(30, 3), 4)
    vals.sum().backward()
    assert a.grad is not None and bool(a.grad.abs().sum() > 0)

"""GPU tier: the Chebyshev recurrence step (dn_eigen.hip) on the device -- the shared cases of eigen_cases.py against ``numpy.longdouble``
on the same CSR arrays -- and the device route of ``geometry.laplacian_eigenbasis``, every run checked in numpy against its inputs and
against shift-invert ``eigsh``; ``compute_operators_with(..., eigensolver="subspace")`` and a ``DiffusionNet`` forward on its operators."""
import os

import numpy as np
import pytest
import torch

import eigen_cases as ec

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
    assert lib.dn_cheb_rows_per_workgroup() >= 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("pad", [0, ec.PAD])
@pytest.mark.parametrize("nb", ec.NBS)
def test_block_widths(dev, nb, pad):
    ec.run_shapes(dev, nb, pad)


@pytest.mark.parametrize("nb", [1, 65])
def test_small_row_counts(dev, nb):
    ec.run_small_rows(dev, nb)


def test_call_forms(dev):
    ec.run_call_forms(dev)


def test_refused_calls(dev):
    ec.run_refused_calls(dev)


def test_op_errors(dev):
    ec.run_op_errors(dev)


def test_host_tensors_are_refused(dev):
    from diffusion_net import ops
    rowptr, col, val = ec.device_csr(ec.small_csr(9), "cpu")
    Y = torch.ones(9, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cheb_step(rowptr, col, val, Y, None, 1.0, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        ops.cheb_step(rowptr.to(dev), col.to(dev), val.to(dev), Y, None, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("name", list(ec.SOLVER_CASES))
def test_device_route(dev, name):
    ec.run_solver(name, dev, "kernel")


def test_device_route_goes_through_the_kernel_and_repeats(dev, monkeypatch):
    from diffusion_net import ops
    calls = []
    real = ops.cheb_step
    monkeypatch.setattr(ops, "cheb_step", lambda *a, **k: calls.append(1) or real(*a, **k))
    a = ec.solve("sphere300_k16", dev, "kernel")
    assert len(calls) == a[2]["products"] > 0
    b = ec.solve("sphere300_k16", dev, "kernel")
    assert a[2]["iterations"] == b[2]["iterations"] and a[2]["degrees"] == b[2]["degrees"]
    assert float((a[0] - b[0]).abs().max()) <= 2 * ec.RTOL * float(a[0][-1])


def test_max_iter_reached_raises(dev):
    with pytest.raises(RuntimeError, match="did not reach rtol"):
        ec.solve("sphere300_k16", dev, "kernel", max_iter=1)


def test_compute_operators_with_the_subspace_solver(dev):
    ec.run_compute_operators(dev)


def test_cache_round_trip_and_bad_values(dev, tmp_path, monkeypatch):
    ec.run_cache_round_trip(dev, tmp_path, monkeypatch)


def test_custom_operator(dev):
    from diffusion_net import ops, torchlib  # noqa: F401
    csr = ec.device_csr(ec.small_csr(9), dev)
    Y = torch.from_numpy(np.random.RandomState(4).randn(9, 5)).to(dev)
    assert torch.equal(torch.ops.diffusion_net.cheb_step(*csr, Y, None, 2.0, 0.5, 0.0), ops.cheb_step(*csr, Y, None, 2.0, 0.5, 0.0))


def test_network_forward_on_subspace_operators(dev):
    """A ``DiffusionNet`` forward on operators built with ``eigensolver="subspace"``: a finite output of the right shape."""
    import diffusion_net
    from diffusion_net import synthetic
    v, f = synthetic.sphere_mesh(300, seed=ec.MESH_SEED)
    verts, faces = torch.from_numpy(v).float().to(dev), torch.from_numpy(f).to(dev)
    frames, mass, L, evals, evecs, gradX, gradY = diffusion_net.geometry.compute_operators_with(verts, faces, 32, eigensolver="subspace")
    assert evals.dtype == torch.float32 and tuple(evecs.shape) == (300, 32) and evecs.is_cuda
    torch.manual_seed(3)
    model = diffusion_net.layers.DiffusionNet(3, 5, C_width=32, N_block=2, outputs_at="vertices", dropout=False).to(dev).eval()
    with torch.no_grad():
        out = model(verts, mass, L=L, evals=evals, evecs=evecs, gradX=gradX, gradY=gradY)
    assert tuple(out.shape) == (300, 5) and bool(torch.isfinite(out).all())

"""GPU tier: the implicit diffusion (dn_implicit.hip) on the device -- the shared cases of implicit_cases.py against the fp64 dense solve --
plus what only a device can show: the check=False form captured in a graph, the refusal of host tensors."""
import os

import numpy as np
import pytest
import torch

import implicit_cases as ic

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
    assert lib.dn_implicit_rows_per_tile() >= 1
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ic.FAMILIES)
def test_families(dev, name):
    ic.run_family(name, dev)


@pytest.mark.parametrize("C", ic.WIDTHS)
def test_widths(dev, C):
    ic.run_family("ragged", dev, C)


def test_one_vertex(dev):
    ic.run_family("v1", dev)


@pytest.mark.parametrize("name", ["sphere300", "sphere300_mass6", "graph200", "ragged"])
def test_iteration_counts_match_the_numpy_route(dev, name):
    ic.run_iteration_counts(name, dev)


def test_call_forms(dev):
    ic.run_call_forms(dev)


def test_max_iter_reached_raises(dev):
    ic.run_max_iter_raises(dev)


def test_isolation(dev):
    ic.run_isolation(dev)


@pytest.mark.parametrize("name,C", [("sphere300", 5), ("sphere300_mass6", 5), ("sphere300_chan", 5), ("graph200", 5), ("ragged", 65), ("tile_edges", 130)])
def test_backward(dev, name, C):
    ic.run_backward(name, dev, C)


def test_custom_operator(dev):
    ic.run_custom_operator(dev)


def test_refused_calls(dev):
    ic.run_refused_calls(dev)


def test_op_errors(dev):
    ic.run_op_errors(dev)


def test_layer(dev):
    ic.run_layer(dev)


def test_network(dev):
    ic.run_network(dev)


def test_host_tensors_are_refused(dev):
    from diffusion_net import ops
    rowptr, col, val, m, t, u, sizes = ic.device_operands("small", 5, "cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.implicit_solve(rowptr, col, val, m, t, u, sizes)
    with pytest.raises(RuntimeError):
        ops.implicit_solve(rowptr.to(dev), col.to(dev), val.to(dev), m.to(dev), t.to(dev), u, sizes)
    with pytest.raises(RuntimeError):
        ops.implicit_solve(rowptr.to(dev), col.to(dev), val.to(dev), m, t.to(dev), u.to(dev), sizes)


def test_graph_capture_of_forward_and_backward(dev):
    """Forward plus backward of the check=False form (``ops.ImplicitDiffusionFn`` with check off: a fixed number of iterations, no host read)
    captured in a ``torch.cuda.graph`` and replayed twice: the eager bits, and the bounds."""
    from diffusion_net import ops
    name, C, n_it = "ragged", 5, 100
    rowptr, col, val, m, t, u, sizes = ic.device_operands(name, C, dev)
    op = ops.ImplicitOperator(rowptr, col, val, m, sizes)
    w = torch.from_numpy(ic.grad_yardstick(name, C)[0]).to(dev)

    def step(u_, t_):
        x = ops.ImplicitDiffusionFn.apply(u_, t_, op, ic.RTOL, n_it, False)
        d_u, d_t = torch.autograd.grad(x, (u_, t_), w)
        return x, d_u, d_t

    su, st_ = u.clone().requires_grad_(True), t.clone().requires_grad_(True)
    eager = [a.detach().clone() for a in step(su, st_)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(su, st_)                      # warm-up on the capture's side of things: tables, code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(su, st_)
    for _ in range(2):
        for o in outs:
            o.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(outs, eager, ("x", "d_u", "d_t")):
            assert torch.equal(ic.bits(got), ic.bits(want)), what
    err = ic.mesh_norms(outs[0].detach().cpu().numpy().astype(np.float64) - ic.yardstick(name, C), sizes)
    assert float((err / ic.forward_bound(name, C)).max()) <= 1.0
    ic.check_backward(name, C, dev, outs[1], outs[2], "graph replay")

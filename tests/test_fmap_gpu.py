"""GPU tier: the regularised spectral solve of the functional-map layer (dn_fmap.hip) on the device -- the shared cases of fmap_cases.py,
``fmaps.compute_correspondence`` / ``fmaps.functional_map`` against the reference's recorded outputs, a HIP-graph capture of forward plus
backward (which any host synchronisation on the route would break) and the registered operator under ``torch.compile``."""
import os

import pytest
import torch

import fmap_cases

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
    assert lib.dn_fmap_max_k() == 64
    return torch.device("cuda:0")


@pytest.mark.parametrize("K,F,P", fmap_cases.CASES)
def test_case(dev, K, F, P):
    fmap_cases.run_case(dev, K, F, P)


def test_determinism(dev):
    fmap_cases.run_determinism(dev)


def test_singular_row(dev):
    fmap_cases.run_singular_row(dev)


def test_limits_and_errors(dev):
    fmap_cases.run_limits(dev)


@pytest.mark.parametrize("how", ["compute_correspondence", "functional_map"])
def test_reference_fixture(dev, how):
    fmap_cases.run_reference_fixture(dev, how)


def test_forward_and_backward_capture_in_a_graph(dev):
    """forward + backward of ``functional_map`` (V = 70, K = 5, F = 3) captured on one stream, replayed on new input values, against the
    eager call bit for bit.  A route that waits for the device anywhere -- an ``info`` check, a ``.item()`` -- cannot be captured."""
    from diffusion_net import fmaps
    t = fmap_cases.spectral_inputs(70, 5, 3, 41)
    u = fmap_cases.spectral_inputs(70, 5, 3, 42)
    d = {k: v.to(dev) for k, v in t.items()}
    c_gt = torch.randn(5, 5, generator=torch.Generator().manual_seed(43)).to(dev)

    def step(fx, fy):
        fx.grad = fy.grad = None
        C = fmaps.functional_map(fx, fy, d["mass_x"], d["mass_y"], d["evals_x"], d["evals_y"], d["evecs_x"], d["evecs_y"], n_fmap=5,
                                 lambda_param=fmap_cases.LAM)
        ((C - c_gt) ** 2).mean().backward()
        return C.detach(), fx.grad, fy.grad

    fx, fy = d["feat_x"].clone().requires_grad_(True), d["feat_y"].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):             # warm-up off the default stream, as torch asks before a capture
        step(fx, fy)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(fx, fy)
    with torch.no_grad():
        fx.copy_(u["feat_x"].to(dev))
        fy.copy_(u["feat_y"].to(dev))
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in out]
    ex, ey = u["feat_x"].to(dev).requires_grad_(True), u["feat_y"].to(dev).requires_grad_(True)
    want = step(ex, ey)
    for g, w in zip(got, want):
        assert bool(torch.isfinite(w).all()) and torch.equal(g, w)
    assert not torch.equal(got[0], fmaps.functional_map(d["feat_x"], d["feat_y"], d["mass_x"], d["mass_y"], d["evals_x"], d["evals_y"],
                                                        d["evecs_x"], d["evecs_y"], n_fmap=5, lambda_param=fmap_cases.LAM))


def test_registered_operator_under_torch_compile(dev):
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fmap_solve)
    A, B, ex, ey = (t.to(dev) for t in fmap_cases.op_inputs(30, 16, 2))
    dC = torch.randn(2, 30, 30, generator=torch.Generator().manual_seed(5)).to(dev)

    def f(a, b):
        C = torch.ops.diffusion_net.fmap_solve(a * 1.0, b, ex, ey, fmap_cases.LAM)
        return C + 0.0

    runs = []
    for fn in (f, torch.compile(f, fullgraph=True)):
        a, b = A.clone().requires_grad_(True), B.clone().requires_grad_(True)
        C = fn(a, b)
        C.backward(dC)
        runs.append((C.detach(), a.grad, b.grad))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    ref = fmap_cases.formula64(A.cpu(), B.cpu(), ex.cpu(), ey.cpu(), fmap_cases.LAM32)
    assert fmap_cases._share(runs[0][0], ref) <= fmap_cases.OP_BOUND

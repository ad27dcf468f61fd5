"""CPU tier: the torch routes of ``diffusion_net.fmaps`` (host tensors, fp64, K past the kernel, differentiable eigenvalues) against the
reference's recorded outputs (tests/golden/geom_fmap_ref.npz), the errors, the meta implementation of the registered operator and where the
names resolve."""
import pytest
import torch

import diffusion_net
import fmap_cases


@pytest.mark.parametrize("how", ["compute_correspondence", "functional_map"])
def test_host_fp32_route_matches_the_reference(how):
    fmap_cases.run_reference_fixture("cpu", how)


@pytest.mark.parametrize("how", ["compute_correspondence", "functional_map"])
def test_host_fp64_route_matches_the_reference(how):
    """fp64 against fp64: two evaluations of one formula that differ in the order of their sums.  First-order bound on either one: the
    projections are sums of V terms, G and H of F terms, a backward-stable solve of order K adds K -- relative perturbations of
    n 2^-52, n = V + F + K, of a system of condition `cond`; two evaluations, so 2 n 2^-52 cond on C relative to its largest entry.  The
    gradient goes through the inverse once more: 2 n 2^-52 cond^2."""
    for name, t in fmap_cases.golden_cases():
        cond = fmap_cases.fixture_condition(t)
        K = t["evals_x"].shape[0]
        eps = 2 * (t["feat_x"].shape[0] + t["feat_x"].shape[1] + K) * 2.0 ** -52
        C, gx, gy = fmap_cases._with_grads(how, t, torch.float64, "cpu")
        for got, ref, bound in ((C, t["C_f64"], eps * cond), (gx, t["grad_feat_x_f64"], eps * cond ** 2),
                                (gy, t["grad_feat_y_f64"], eps * cond ** 2)):
            err = float((got - ref).abs().max() / ref.abs().max())
            print("fmap host fp64 %s %s: %.3e (bound %.3e)" % (name, how, err, bound))
            assert err <= bound, (name, how)


def test_differentiable_eigenvalues_take_the_torch_route():
    A, B, ex, ey = fmap_cases.op_inputs(5, 3, 1)
    ex, ey = ex[0].double().requires_grad_(True), ey[0].double().requires_grad_(True)
    lam = torch.tensor(fmap_cases.LAM, dtype=torch.float64, requires_grad=True)
    C = diffusion_net.fmaps.solve(A[0].double(), B[0].double(), ex, ey, lam)
    C.sum().backward()
    for g in (ex.grad, ey.grad, lam.grad):
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    assert torch.autograd.gradcheck(lambda x, y: diffusion_net.fmaps.solve(A[0].double(), B[0].double(), x, y, fmap_cases.LAM),
                                    (ex.detach().requires_grad_(True), ey.detach().requires_grad_(True)))


def test_singular_system_is_a_nan_row_on_the_torch_route():
    A, B, ex, ey = fmap_cases.op_inputs(5, 3, 1)
    C = diffusion_net.fmaps.solve(torch.zeros_like(A[0]), B[0], ex[0], ey[0], fmap_cases.LAM)
    assert bool(torch.isnan(C[0]).all()) and bool(torch.isfinite(C[1:]).all())


def test_kernel_entry_refuses_host_tensors_and_bad_shapes():
    from diffusion_net import ops
    A, B, ex, ey = fmap_cases.op_inputs(5, 3, 1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fmap_solve(A, B, ex, ey, fmap_cases.LAM)
    with pytest.raises(ValueError, match="square"):
        diffusion_net.fmaps.solve(A, B, ex[:, :4], ey, fmap_cases.LAM)


def test_fake_kernel_of_the_registered_operator():
    from diffusion_net import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fmap_solve)
    m = lambda *s: torch.empty(*s, device="meta")
    C = torch.ops.diffusion_net.fmap_solve(m(3, 30, 128), m(3, 30, 128), m(3, 30), m(3, 30), 1e-3)
    assert tuple(C.shape) == (3, 30, 30) and C.dtype == torch.float32
    C = torch.ops.diffusion_net.fmap_solve(m(5, 3), m(5, 3), m(5), m(5), 1e-3)
    assert tuple(C.shape) == (5, 5)
    dA, dB = torch.ops.diffusion_net.fmap_solve_bwd(m(3, 30, 30), m(3, 30, 128), m(3, 30, 128), m(3, 30), m(3, 30), 1e-3)
    assert tuple(dA.shape) == (3, 30, 128) == tuple(dB.shape)


def test_names_resolve_on_the_package():
    from diffusion_net import _hip, ops
    assert callable(diffusion_net.fmaps.compute_correspondence) and callable(diffusion_net.fmaps.functional_map)
    assert callable(ops.fmap_solve) and issubclass(ops.FmapSolveFn, torch.autograd.Function)
    assert _hip.FMAP_MAX_K == 64 and "dn_fmap_solve_bwd_f32" in _hip.EXPORTED_SYMBOLS

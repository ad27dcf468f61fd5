"""CPU tier, no library: the numpy route of the implicit diffusion (``precompute.implicit_diffusion_host``, the iteration-count yardstick of
the kernel tiers) against the fp64 dense solve, the public surface, and the errors that need no kernel.  Bodies and criteria in
implicit_cases.py."""
import inspect

import numpy as np
import pytest
import torch

import implicit_cases as ic

HOST_FAMILIES = ("sphere300", "sphere300_mass6", "sphere300_chan", "graph200")


@pytest.mark.parametrize("name", HOST_FAMILIES)
def test_numpy_route_meets_the_forward_bound(name):
    from diffusion_net import precompute as P
    L, m, sizes = ic.family(name)
    x, info = P.implicit_diffusion_host(L, m, ic.times(5), ic.rhs(name, 5), sizes, rtol=ic.RTOL, max_iter=ic.MAX_ITER, return_info=True)
    bound = ic.RTOL * ic.mesh_norms(m.astype(np.float64)[:, None] * ic.rhs(name, 5), sizes) / float(m.min())      # no fp32 store here
    share = float((ic.mesh_norms(x - ic.yardstick(name, 5), sizes) / bound).max())
    print("numpy route %s: %.3f of the bound, iterations %s" % (name, share, info["iterations"].tolist()))
    assert share <= 1.0 and (info["residual"] <= ic.RTOL).all()
    assert info["iterations"].max() <= ic.MAX_ITER // 2         # the cap of 200 leaves more than 2x room (sphere300: 74 iterations)


def test_numpy_route_on_a_ragged_batch_freezes_and_isolates():
    from diffusion_net import precompute as P
    L, m, sizes = ic.family("ragged")
    u = ic.rhs("ragged", 5)
    x, info = P.implicit_diffusion_host(L, m, ic.times(5), u, sizes, rtol=ic.RTOL, max_iter=ic.MAX_ITER, return_info=True)
    assert info["iterations"].shape == (4, 5) and info["iterations"][3].max() == 0          # the one-vertex mesh needs no iteration
    for (lo, hi), n in zip(ic.segments(sizes)[:2], sizes[:2]):                              # a mesh alone: the same values
        alone = P.implicit_diffusion_host(L[lo:hi, lo:hi], m[lo:hi], ic.times(5), u[lo:hi], rtol=ic.RTOL, max_iter=ic.MAX_ITER)
        assert np.array_equal(alone, x[lo:hi])
    with pytest.raises(RuntimeError, match="did not reach rtol"):
        P.implicit_diffusion_host(L, m, ic.times(5), u, sizes, rtol=ic.RTOL, max_iter=1)
    with pytest.raises(ValueError):
        P.implicit_diffusion_host(L, m, ic.times(5), u, [5])


def test_public_surface():
    import diffusion_net
    from diffusion_net import _hip, layers, ops, torchlib  # noqa: F401
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(ops.implicit_solve) == ["rowptr", "col", "val", "mass", "time", "rhs", "sizes", "x0", "rtol", "max_iter", "iters_per_check", "check",
                                       "return_info"]
    d = {k: v.default for k, v in inspect.signature(ops.implicit_solve).parameters.items()}
    assert (d["rtol"], d["max_iter"], d["iters_per_check"], d["check"], d["return_info"]) == (1e-9, 1000, 16, True, False)
    assert issubclass(ops.ImplicitDiffusionFn, torch.autograd.Function)
    for name in ("dn_implicit_rows_per_tile", "dn_implicit_workspace_bytes", "dn_implicit_init_f32", "dn_implicit_iterate_f32",
                 "dn_implicit_finish_f32", "dn_implicit_lx_dot_f32"):
        assert name in _hip.EXPORTED_SYMBOLS
    assert callable(torch.ops.diffusion_net.implicit_solve)
    for cls in (lambda m: layers.LearnedTimeDiffusion(4, method=m), lambda m: layers.DiffusionNetBlock(4, [4], diffusion_method=m),
                lambda m: layers.DiffusionNet(3, 2, C_width=4, N_block=1, diffusion_method=m)):
        for m in ("spectral", "implicit_dense", "implicit_sparse"):
            cls(m)
    with pytest.raises(ValueError, match="invalid setting for diffusion_method"):
        layers.DiffusionNet(3, 2, diffusion_method="implicit_cg")
    a = layers.DiffusionNet(3, 2, C_width=4, N_block=1, diffusion_method="implicit_sparse")
    b = layers.DiffusionNet(3, 2, C_width=4, N_block=1)
    assert list(a.state_dict()) == list(b.state_dict())
    lay = a.blocks[0].diffusion
    assert (lay.implicit_rtol, lay.implicit_max_iter, lay.implicit_check) == (1e-9, 1000, True)


def test_host_tensors_are_refused_without_a_device():
    """No emulator bound and no ROCm device in use: the op raises, there is no CPU path."""
    from diffusion_net import _hip, ops
    _hip._use_library_for_tests(None, False)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.implicit_solve(*ic.device_operands("graph200", 5, "cpu"))

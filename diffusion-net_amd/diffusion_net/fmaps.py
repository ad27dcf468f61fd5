"""``diffusion_net.fmaps`` -- the functional-map layer of the reference's functional_correspondence experiment
(experiments/functional_correspondence/fmaps_model.py:11-40, 79-81).

For spectral coefficients A, B [K, F] (the features of shapes x and y in their truncated eigenbases), G = A A^T and H = B A^T, row i of the
map C [K, K] is

    c_i = (G + lam D_i)^-1 H[i, :]^T,        D_i = diag_j (evals_x[j] - evals_y[i])^2.

``compute_correspondence`` has the signature and the [1, K, K] result of the experiment's function: the script changes one import
(``from diffusion_net.fmaps import compute_correspondence``).  ``functional_map`` takes what the model holds -- features, mass, eigenvalues,
eigenvectors -- projects with ``geometry.to_basis`` and never forms ``evecs^T diag(mass)``; no route here builds a V x V matrix.

Routing, as in ``geometry.find_knn``: fp32 tensors on a ROCm device with K <= 64, where neither the eigenvalues nor lam require grad, run
the HIP solve (``ops.fmap_solve``: fp64 arithmetic on the fp32 coefficients, closed-form backward, two and three launches, no host
synchronisation -- a training step can be captured in a HIP graph).  Everything else -- host tensors, other dtypes, larger K, differentiable
eigenvalues, lam given as a tensor -- takes one batched ``torch.linalg.solve_ex`` over the K systems in the dtype of the coefficients.

One difference from the script: a singular system gives a NaN row of C here, on both routes; the script's ``torch.inverse`` raises (after
waiting for the device).  ``ops.fmap_solve(..., check=True)`` is the call that raises.
"""
import torch

from . import geometry, ops


def _solve_torch(A, B, evals_x, evals_y, lam):
    """The formula in torch, vectorised over the rows of C: A, B [..., K, F], evals [..., K] -> [..., K, K]; differentiable in everything."""
    evals_x, evals_y = evals_x.to(A.dtype), evals_y.to(A.dtype)
    At = A.transpose(-1, -2)
    G, H = A @ At, B @ At
    D = (evals_x[..., None, :] - evals_y[..., :, None]) ** 2                    # [..., i, j]
    M = G[..., None, :, :] + lam * torch.diag_embed(D)                          # [..., i, K, K]
    X, info = torch.linalg.solve_ex(M, H[..., :, :, None], check_errors=False)   # (no error check: that would wait for the device)
    return torch.where((info != 0)[..., None], torch.full_like(X[..., 0], float("nan")), X[..., 0])


def _on_kernel(A, B, evals_x, evals_y, lam):
    ts = (A, B, evals_x, evals_y)
    return (all(t.is_cuda and t.dtype == torch.float32 for t in ts) and len({t.device for t in ts}) == 1
            and A.dim() in (2, 3) and 1 <= A.shape[-2] <= ops._hip.FMAP_MAX_K
            and not evals_x.requires_grad and not evals_y.requires_grad and not isinstance(lam, torch.Tensor))


def solve(A, B, evals_x, evals_y, lambda_param=1e-3):
    """The map of spectral coefficients ``A``, ``B`` [K, F] or [P, K, F] and eigenvalues [K] or [P, K] -> [K, K] or [P, K, K], routed as the
    module says."""
    if A.shape != B.shape or A.dim() < 2 or tuple(evals_x.shape) != tuple(A.shape[:-1]) or tuple(evals_y.shape) != tuple(A.shape[:-1]):
        raise ValueError("functional maps are square: coefficients [.., K, F] of one shape and K eigenvalues per shape (got %s, %s, %s, %s)" % (
            tuple(A.shape), tuple(B.shape), tuple(evals_x.shape), tuple(evals_y.shape)))
    if _on_kernel(A, B, evals_x, evals_y, lambda_param):
        if torch.compiler.is_compiling():
            from . import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fmap_solve)
            return torch.ops.diffusion_net.fmap_solve(A, B, evals_x, evals_y, float(lambda_param))
        return ops.fmap_solve(A, B, evals_x, evals_y, lambda_param)
    return _solve_torch(A, B, evals_x, evals_y, lambda_param)


def compute_correspondence(feat_x, feat_y, evals_x, evals_y, evecs_trans_x, evecs_trans_y, lambda_param=1e-3):
    """The experiment's function: features [V, F], eigenvalues [K], ``evecs_trans`` [K, V] = evecs^T diag(mass) -> C [1, K, K]."""
    A, B = evecs_trans_x @ feat_x, evecs_trans_y @ feat_y
    return solve(A, B, evals_x, evals_y, lambda_param).unsqueeze(0)


def functional_map(feat_x, feat_y, mass_x, mass_y, evals_x, evals_y, evecs_x, evecs_y, n_fmap=30, lambda_param=1e-3):
    """What the experiment's model computes after its two feature passes: features [V, F], mass [V], eigenvalues [k_eig], eigenvectors
    [V, k_eig] of both shapes -> C [K, K] on the first K = ``n_fmap`` eigenpairs.  The projection is evecs^T (mass * feat): on a ROCm
    device ``geometry.to_basis`` (HIP), on the host the same product in torch."""
    K = int(n_fmap)
    spec = []
    for feat, mass, evecs in ((feat_x, mass_x, evecs_x), (feat_y, mass_y, evecs_y)):
        basis = evecs[:, :K]
        if feat.is_cuda and feat.dtype == torch.float32 and basis.dtype == torch.float32 and mass.dtype == torch.float32:
            spec.append(geometry.to_basis(feat, basis, mass))
        else:
            spec.append(basis.transpose(-1, -2) @ (feat * mass[:, None]))
    return solve(spec[0], spec[1], evals_x[:K], evals_y[:K], lambda_param)

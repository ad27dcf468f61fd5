"""Host-side geometry precompute: the per-mesh operators the hot path consumes.

north_star keeps this stage on the host CPU, cached on disk "as the reference does"; the reference delegates the
Laplacian to potpourri3d (not installable here) and builds the gradient operator in a per-vertex Python loop
(geometry.py:222-263).  This module restates the pipeline of ``compute_operators`` (geometry.py:276-392) with
numpy/scipy only, fully vectorised:

    normals -> tangent frames -> cotan Laplacian + lumped mass -> generalized eigenproblem (shift-invert eigsh)
            -> per-vertex least-squares gradient operator (complex; split into gradX / gradY)

and the npz operator cache of ``get_operators`` (geometry.py:426-570) with the same file naming
(sha1(verts,faces)_<bucket>.npz) and the same keys, so caches written by either implementation are interchangeable.
Point clouds (empty ``faces``): normals, frames and gradients come from ``geometry.cloud_operators`` (HIP kernel on a ROCm device,
vectorised numpy otherwise); the point-cloud LAPLACIAN of robust_laplacian is not restated -- ``compute_operators`` takes it from its
``laplacian=`` argument or from that package if it is installed -- but ``laplacian="delaunay"`` builds the local-Delaunay Laplacian the
wheel starts from (``point_cloud_laplacian_host`` here, dn_cloud_lap.hip on a ROCm device), without its intrinsic re-triangulation.
"""
from __future__ import annotations

import os

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla
import torch

from .utils import hash_arrays  # noqa: F401  (the cache key; also reachable as precompute.hash_arrays)

EPS = 1e-8            # geometry.py:309
GRAD_REG = 1e-5       # geometry.py:239


# ----------------------------------------------------------------------------------------- Laplacian, mass
def cotan_laplacian(verts: np.ndarray, faces: np.ndarray, denom_eps: float = 1e-10) -> sp.csr_matrix:
    """Positive semi-definite weak cotan Laplacian: for every face corner k with opposite edge (i,j),
    w = 0.5*cot(angle_k) = 0.5 * <a,b> / (|a x b| + eps); L[i,i] += w, L[j,j] += w, L[i,j] -= w, L[j,i] -= w."""
    V = verts.shape[0]
    rows, cols, vals = [], [], []
    for k in range(3):
        i, j, o = faces[:, (k + 1) % 3], faces[:, (k + 2) % 3], faces[:, k]
        a, b = verts[i] - verts[o], verts[j] - verts[o]
        w = 0.5 * np.einsum("ij,ij->i", a, b) / (np.linalg.norm(np.cross(a, b), axis=1) + denom_eps)
        rows += [i, j, i, j]
        cols += [i, j, j, i]
        vals += [w, w, -w, -w]
    L = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(V, V))
    return L.tocsr()


def vertex_areas(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Barycentric lumped mass: one third of the area of every incident face."""
    e1, e2 = verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    return np.bincount(faces.reshape(-1), weights=np.repeat(area / 3.0, 3), minlength=verts.shape[0])


# ----------------------------------------------------------------------------------------- normals, frames
def _unit_face_normal_sum(verts, faces):
    n = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    n = n / (np.linalg.norm(n, axis=1, keepdims=True) + 1e-6)         # normalize() of geometry.py:37-47
    out = np.zeros_like(verts)
    for k in range(3):
        np.add.at(out, faces[:, k], n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return out / np.linalg.norm(out, axis=1, keepdims=True)


def vertex_normals(verts: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Sum of unit face normals per vertex, normalised; degenerate vertices are re-estimated on slightly jittered
    positions and, failing that, get a fixed pseudo-random direction (behaviour of geometry.py:114-148)."""
    normals = _unit_face_normal_sum(verts, faces)
    bad = np.isnan(normals).any(axis=1)
    if bad.any():
        rng = np.random.RandomState(seed=777)
        scale = np.linalg.norm(verts.max(0) - verts.min(0)) * 1e-4
        jitter = (rng.rand(*verts.shape) - 0.5) * scale
        normals = _unit_face_normal_sum(verts + bad[:, None] * jitter, faces)
        bad = np.isnan(normals).any(axis=1)
        if bad.any():
            rnd = np.random.RandomState(seed=777).rand(*verts.shape) - 0.5
            normals[bad] = rnd[bad] / np.linalg.norm(rnd[bad], axis=1, keepdims=True)
    if np.isnan(normals).any():
        raise ValueError("NaN normals :(")
    return normals


def neighborhood_normal(points: np.ndarray) -> np.ndarray:
    """(N,K,3) neighbourhoods centred on their point -> (N,3) unit normals: the right singular vector of the smallest singular value of
    every K x 3 block, in the dtype of ``points`` and with the sign LAPACK returns (geometry.py:92-99).  numpy in, numpy out.
    (K < 3, where the reference's reduced SVD has no third vector and raises: the full one, whose last vector spans the null space.)"""
    vh = np.linalg.svd(points, full_matrices=points.shape[1] < 3)[2]
    normal = vh[:, 2, :]
    return normal / np.linalg.norm(normal, axis=-1, keepdims=True)


def tangent_frames(normals: np.ndarray) -> np.ndarray:
    """(V,3,3) rows = (basisX, basisY, normal): basisX is e_x (or e_y where the normal is within ~26 degrees of e_x)
    projected onto the tangent plane, basisY = n x basisX (geometry.py:151-177)."""
    V = normals.shape[0]
    cand = np.where((np.abs(normals[:, 0]) < 0.9)[:, None], np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    bx = cand - normals * np.einsum("ij,ij->i", cand, normals)[:, None]
    bx = bx / (np.linalg.norm(bx, axis=1, keepdims=True) + 1e-6)
    by = np.cross(normals, bx)
    frames = np.stack([bx, by, normals], axis=1)
    if np.isnan(frames).any():
        raise ValueError("NaN coordinate frame! Must be very degenerate")
    return frames.reshape(V, 3, 3)


# ----------------------------------------------------------------------------------------- gradient operator
def gradient_operator(verts: np.ndarray, frames: np.ndarray, edges: np.ndarray) -> sp.csc_matrix:
    """Complex (V,V) operator: row v holds the least-squares gradient stencil of vertex v over its outgoing edges
    (tail v -> tip j), expressed in v's tangent frame (real = X, imag = Y).

    Per vertex, with t_e the 2-D tangent coordinates of edge e:  G = sum_e t_e t_e^T + 1e-5 I,
    coefficient of neighbour j_e = G^-1 t_e, coefficient of v itself = -sum_e G^-1 t_e.
    (Vectorised restatement of the per-vertex solve of geometry.py:222-263.)"""
    tail, tip = edges[0], edges[1]
    keep = tail != tip
    tail, tip = tail[keep], tip[keep]
    d = verts[tip] - verts[tail]
    tx = np.einsum("ij,ij->i", d, frames[tail, 0])
    ty = np.einsum("ij,ij->i", d, frames[tail, 1])
    return gradient_from_tangents(verts.shape[0], tail, tip, tx, ty)


def gradient_from_tangents(V: int, tail: np.ndarray, tip: np.ndarray, tx: np.ndarray, ty: np.ndarray) -> sp.csc_matrix:
    """The per-vertex 2 x 2 solves of ``gradient_operator`` on edges (tail -> tip, none with tail == tip) whose tangent coordinates
    (tx, ty) in the tail's frame are given."""
    gxx = np.bincount(tail, weights=tx * tx, minlength=V) + GRAD_REG
    gxy = np.bincount(tail, weights=tx * ty, minlength=V)
    gyy = np.bincount(tail, weights=ty * ty, minlength=V) + GRAD_REG
    det = gxx * gyy - gxy * gxy
    ixx, ixy, iyy = gyy / det, -gxy / det, gxx / det
    cx = ixx[tail] * tx + ixy[tail] * ty
    cy = ixy[tail] * tx + iyy[tail] * ty
    coef = cx + 1j * cy
    diag = -(np.bincount(tail, weights=cx, minlength=V) + 1j * np.bincount(tail, weights=cy, minlength=V))
    rows = np.concatenate([np.arange(V), tail])
    cols = np.concatenate([np.arange(V), tip])
    data = np.concatenate([diag, coef])
    return sp.coo_matrix((data, (rows, cols)), shape=(V, V)).tocsc()


# ----------------------------------------------------------------------------------------- eigenbasis
def laplacian_eigenbasis(L: sp.spmatrix, massvec: np.ndarray, k_eig: int):
    """k smallest generalized eigenpairs of (L + eps I) phi = lambda M phi by shift-invert Lanczos; up to 4 retries with a
    growing diagonal shift if the factorisation fails (geometry.py:337-361).  Eigenvalues clipped at 0."""
    if k_eig == 0:
        return np.zeros((0,)), np.zeros((L.shape[0], 0))
    A = (L + sp.identity(L.shape[0]) * EPS).tocsc()
    M = sp.diags(massvec)
    fails = 0
    while True:
        try:
            evals, evecs = sla.eigsh(A, k=k_eig, M=M, sigma=EPS)
            return np.clip(evals, 0.0, np.inf), evecs
        except Exception as err:   # noqa: BLE001 -- ARPACK / SuperLU raise assorted types
            if fails > 3:
                raise ValueError("failed to compute eigendecomp") from err
            fails += 1
            A = A + sp.identity(L.shape[0]) * (EPS * 10 ** fails)


# ----------------------------------------------------------------------------------------- eigenbasis by filtered subspace iteration
# The same pencil, (L + eps I) phi = lambda M phi, without a sparse factorisation: with D = diag(massvec^-1/2) and S = D (L + eps I) D
# (symmetric, CSR, fp64) the k smallest pairs of S x = lambda x give phi = D x.  A block X of nb = k + max(16, ceil(k / 4)) orthonormal
# columns is Rayleigh-Ritz'ed (H = X^T S X, (w, Q) = eigh(H), X <- X Q) and, until the first k residuals ||S x_i - w_i x_i|| fall below
# rtol w_k, filtered by the Chebyshev polynomial T_m((S - c) / e) of the interval [a, ub] = [w_nb, Gershgorin bound] -- which damps what the
# block does not want and grows what lies below a -- and re-orthonormalised by Cholesky-QR applied twice.  The degree m is the smallest
# that separates the block's own ends by at most SUBSPACE_AMP = 1e6: that bounds the condition number of the filtered block (measured:
# at most 2.8e6), and Cholesky-QR is valid below about 1e8.  One driver serves the numpy route (scipy products, here) and the device route
# (geometry.laplacian_eigenbasis: the products are dn_eigen.hip, the tall dense products torch); the nb x nb eigh and Cholesky run on the
# host in both.
SUBSPACE_AMP = 1e6
SUBSPACE_MAX_DEGREE = 64


def subspace_block_width(k_eig: int) -> int:
    return int(k_eig) + max(16, -(-int(k_eig) // 4))


def scaled_operator(L, massvec: np.ndarray):
    """S = D (L + eps I) D as scipy CSR fp64 with sorted indices, d = massvec^-1/2, ub = max_i sum_j |S_ij| (Gershgorin)."""
    V = L.shape[0]
    m = np.asarray(massvec, dtype=np.float64).reshape(-1)
    if m.shape[0] != V or not (m > 0).all():
        raise ValueError("laplacian eigenbasis: the mass must be %d positive numbers" % V)
    d = 1.0 / np.sqrt(m)
    Dm = sp.diags(d)
    S = (Dm @ (sp.csr_matrix(L).astype(np.float64) + sp.identity(V, format="csr") * EPS) @ Dm).tocsr()
    S.sum_duplicates()
    S.sort_indices()
    ub = float(abs(S).sum(axis=1).max()) if V else 0.0
    if not np.isfinite(ub):
        raise ValueError("laplacian eigenbasis: L and the mass must be finite")
    return S, d, ub


class _NumpyBlocks:
    """The block operations of ``subspace_iterate`` in numpy / scipy (the device route's: geometry._TorchBlocks)."""
    route = "numpy"

    def __init__(self, S):
        self.S = S

    def from_host(self, a):
        return np.array(a, dtype=np.float64)

    def to_host(self, a):
        return np.asarray(a)

    def step(self, Y, Z, alpha, beta, gamma, out=None):
        r = alpha * (self.S @ Y)
        if beta != 0.0:
            r += beta * Y
        if gamma != 0.0:
            r += gamma * Z
        return r

    def tmm(self, A, B):
        return A.T @ B

    def mm(self, A, B):
        return A @ B

    def solve_upper_right(self, X, R):          # X R^-1
        import scipy.linalg as la
        return la.solve_triangular(R, X.T, trans="T", lower=False).T

    def residuals(self, SX, X, w, k):
        return np.linalg.norm(SX[:, :k] - X[:, :k] * w[:k], axis=0)

    def finish(self, X, d, k):
        evecs = X[:, :k] * d[:, None]
        top = np.abs(evecs).argmax(axis=0)      # the first index of the largest magnitude
        sign = np.where(evecs[top, np.arange(k)] < 0, -1.0, 1.0)
        return evecs * sign


def _cholesky_upper(G, what):
    import scipy.linalg as la
    try:
        R = la.cholesky((G + G.T) * 0.5, lower=False)
    except la.LinAlgError as err:
        raise RuntimeError("laplacian eigenbasis (subspace): Cholesky-QR failed %s: %s" % (what, err)) from err
    if not np.isfinite(R).all():
        raise RuntimeError("laplacian eigenbasis (subspace): Cholesky-QR failed %s: non-finite factor" % what)
    return R


def _cholqr2(be, X, what):
    for _ in range(2):
        R = _cholesky_upper(be.to_host(be.tmm(X, X)), what)
        X = be.solve_upper_right(X, be.from_host(R))
    return X


def subspace_iterate(be, V, d, ub, k_eig, rtol=1e-9, seed=0, max_iter=100):
    """The driver: ``be`` supplies the block operations (products with S, tall dense products), this function the algorithm and the small
    factorisations (scipy, on the host).  -> (evals [k] numpy, evecs [V, k] in ``be``'s array type, info dict).  ``RuntimeError`` with the
    iteration and the residual when Cholesky fails or ``max_iter`` Rayleigh-Ritz rounds do not reach ``rtol``: there is no fallback."""
    import math
    import scipy.linalg as la
    k, nb = int(k_eig), subspace_block_width(k_eig)
    info = dict(route=be.route, nb=nb, ub=ub, iterations=0, products=0, degrees=[], residual=float("inf"), rtol=float(rtol))
    X0 = np.random.default_rng(seed).standard_normal((V, nb))          # made on the host: every route starts from the same block
    X = _cholqr2(be, be.from_host(X0), "on the starting block")
    res = float("inf")
    for it in range(int(max_iter)):
        SX = be.step(X, None, 1.0, 0.0, 0.0)
        info["products"] += 1
        H = be.to_host(be.tmm(X, SX))
        w, Q = la.eigh((H + H.T) * 0.5)
        Qb = be.from_host(Q)
        X, SX = be.mm(X, Qb), be.mm(SX, Qb)
        res = float(np.max(be.to_host(be.residuals(SX, X, be.from_host(w), k))))
        info["iterations"], info["residual"] = it + 1, res
        if not np.isfinite(res):
            raise RuntimeError("laplacian eigenbasis (subspace): non-finite residual in iteration %d" % (it + 1))
        if res <= rtol * w[k - 1]:
            evecs = be.finish(X, be.from_host(d), k)
            return np.clip(w[:k], 0.0, np.inf), evecs, info
        if it + 1 == int(max_iter):
            break
        a = float(w[-1])
        if not a < ub:
            raise RuntimeError("laplacian eigenbasis (subspace): the block's largest Ritz value %g is not below the bound %g of the spectrum "
                               "(iteration %d, residual %g)" % (a, ub, it + 1, res))
        c, e = (ub + a) / 2.0, (ub - a) / 2.0
        deg = int(min(SUBSPACE_MAX_DEGREE, max(2, math.ceil(math.acosh(SUBSPACE_AMP) / math.acosh((ub + a) / (ub - a))))))
        info["degrees"].append(deg)
        prev, cur = X, be.step(X, None, 1.0 / e, -c / e, 0.0)            # T_0 X, T_1 X
        for _ in range(2, deg + 1):                                      # T_(j+1) = 2 ((S - c) / e) T_j - T_(j-1), written over T_(j-1)
            prev, cur = cur, be.step(cur, prev, 2.0 / e, -2.0 * c / e, -1.0, out=prev)
        info["products"] += deg
        X = _cholqr2(be, cur, "in iteration %d (residual %g)" % (it + 1, res))
    raise RuntimeError("laplacian eigenbasis (subspace): %d iterations did not reach rtol = %g (residual %g, needs %g)"
                       % (int(max_iter), rtol, res, rtol * w[k - 1]))


def _dense_eigenbasis(L, massvec, k):
    """Tiny meshes (2 nb > V): the dense pencil on the host."""
    import scipy.linalg as la
    V = L.shape[0]
    if k > V:
        raise ValueError("laplacian eigenbasis: %d eigenpairs asked of a %d x %d pencil" % (k, V, V))
    A = (sp.csr_matrix(L).astype(np.float64) + sp.identity(V, format="csr") * EPS).toarray()
    w, U = la.eigh((A + A.T) * 0.5, np.diag(np.asarray(massvec, dtype=np.float64)), subset_by_index=[0, k - 1])
    top = np.abs(U).argmax(axis=0)
    U = U * np.where(U[top, np.arange(k)] < 0, -1.0, 1.0)
    return np.clip(w, 0.0, np.inf), U


def laplacian_eigenbasis_subspace(L, massvec, k_eig, *, rtol=1e-9, seed=0, max_iter=100, return_info=False):
    """``laplacian_eigenbasis`` by Chebyshev-filtered subspace iteration in numpy / scipy, fp64: (evals [k] ascending and clipped at 0,
    evecs [V, k] M-orthonormal, each column signed so that its entry of largest magnitude -- the first on ties -- is positive).  The same
    pencil (L + EPS I) phi = lambda M phi and the same driver as ``geometry.laplacian_eigenbasis``, which runs the products on the device.
    2 nb > V (nb = k + max(16, ceil(k / 4))): ``scipy.linalg.eigh`` of the dense pencil instead.  ``return_info``: also a dict with the
    route, nb, ub, iterations, products with S, filter degrees and the final residual.  ``RuntimeError`` if Cholesky-QR fails or
    ``max_iter`` iterations do not reach ``rtol``."""
    V, k = L.shape[0], int(k_eig)
    m = np.asarray(massvec, dtype=np.float64).reshape(-1)
    if k == 0:
        out = (np.zeros((0,)), np.zeros((V, 0)))
        info = dict(route="empty", nb=0, ub=0.0, iterations=0, products=0, degrees=[], residual=0.0, rtol=float(rtol))
    elif 2 * subspace_block_width(k) > V:
        out = _dense_eigenbasis(L, m, k)
        info = dict(route="dense", nb=subspace_block_width(k), ub=0.0, iterations=0, products=0, degrees=[], residual=0.0, rtol=float(rtol))
    else:
        S, d, ub = scaled_operator(L, m)
        evals, evecs, info = subspace_iterate(_NumpyBlocks(S), V, d, ub, k, rtol, seed, max_iter)
        out = (evals, evecs)
    return (*out, info) if return_info else out


def implicit_diffusion_host(L, mass, time, u, sizes=None, *, x0=None, rtol=1e-9, max_iter=1000, return_info=False):
    """The recurrence of ``ops.implicit_solve`` (dn_implicit.hip) in numpy fp64, all channels at once: for every mesh b (``sizes``: its rows;
    default one mesh) and channel c, ``(diag(m_b) + time[c] L_b) x = m_b * u`` by Jacobi-preconditioned conjugate gradients.

        d = m + t diag(L);  x = x0 (default u);  r = m u - A x;  z = r / d;  p = z;  rz = r.z
        until ||r|| <= rtol ||m u||:   q = A p;  alpha = rz / p.q;  x += alpha p;  r -= alpha q;  z = r / d;
                                       rz' = r.z;  beta = rz' / rz;  p = z + beta p;  rz = rz'

    Norms and dot products are per (mesh, channel), over that mesh's rows.  A system that is done is frozen (its x, r, p stop changing) and
    the loop ends when every system is done; ``RuntimeError`` when ``max_iter`` iterations leave one unfinished.  The operands are taken as
    they are (fp32 arrays are widened).  -> x [V, C] fp64, with ``return_info`` also {"iterations" [n_mesh, C], "residual" [n_mesh, C]}."""
    L = sp.csr_matrix(L).astype(np.float64)
    m = np.asarray(mass, dtype=np.float64).reshape(-1)
    t = np.asarray(time, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64)
    V, C = u.shape
    sizes = [V] if sizes is None else [int(s) for s in sizes]
    if sum(sizes) != V or L.shape != (V, V) or m.shape != (V,) or t.shape != (C,):
        raise ValueError("implicit_diffusion_host takes L [V, V], mass [V], time [C], u [V, C] and sizes that sum to V")
    seg = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    mesh_of = np.repeat(np.arange(len(sizes)), sizes)
    dots = lambda a, b: np.add.reduceat(a * b, seg, axis=0) if V else np.zeros((len(sizes), C))      # [n_mesh, C]
    A = lambda y: m[:, None] * y + t[None, :] * (L @ y)
    d = m[:, None] + t[None, :] * L.diagonal()[:, None]
    b = m[:, None] * u
    x = u.copy() if x0 is None else np.array(x0, dtype=np.float64)
    r = b - A(x)
    p = r / d
    rz, rr, thr = dots(r, p), dots(r, r), rtol * np.sqrt(dots(b, b))
    done = np.sqrt(rr) <= thr
    iters = np.zeros(done.shape, dtype=np.int64)
    it = 0
    while not done.all():
        if it >= max_iter:
            raise RuntimeError("implicit diffusion (host): %d iterations did not reach rtol = %g (%d systems left)" % (it, rtol, int((~done).sum())))
        live = ~done                                             # [n_mesh, C]: the systems this iteration advances
        rows = live[mesh_of]                                     # [V, C]
        q = A(p)
        with np.errstate(all="ignore"):
            alpha = np.where(live, rz / dots(p, q), 0.0)
            x = np.where(rows, x + alpha[mesh_of] * p, x)
            r = np.where(rows, r - alpha[mesh_of] * q, r)
            z = r / d
            rz_new = dots(r, z)
            beta = np.where(live, rz_new / rz, 0.0)
        rz, rr = np.where(live, rz_new, rz), np.where(live, dots(r, r), rr)
        iters += live
        done = done | (live & (np.sqrt(rr) <= thr))
        with np.errstate(all="ignore"):
            p = np.where((~done)[mesh_of], z + beta[mesh_of] * p, p)
        it += 1
    if return_info:
        with np.errstate(all="ignore"):
            res = np.where(rr == 0.0, 0.0, np.sqrt(rr) / np.sqrt(dots(b, b)))
        return x, {"iterations": iters, "residual": res}
    return x


EIGENSOLVERS = (None, "subspace")


def _eigenbasis(L, mass, k_eig, eigensolver, device):
    """(evals, evecs) numpy fp64 of ``compute_operators``: shift-invert ``eigsh`` (None) or ``geometry.laplacian_eigenbasis``."""
    if eigensolver is None:
        return laplacian_eigenbasis(L, mass, k_eig)
    from . import geometry                         # (geometry imports this module)
    evals, evecs = geometry.laplacian_eigenbasis(L, torch.from_numpy(np.ascontiguousarray(mass, dtype=np.float64)).to(device), k_eig)
    return evals.detach().cpu().numpy(), evecs.detach().cpu().numpy()


def _check_eigensolver(eigensolver):
    if eigensolver not in EIGENSOLVERS:
        raise ValueError("eigensolver=%r: None (shift-invert eigsh) or \"subspace\"" % (eigensolver,))


ASSEMBLIES = (None, "device")


def _check_assembly(assembly):
    if assembly not in ASSEMBLIES:
        raise ValueError("assembly=%r: None (the host functions of this module) or \"device\"" % (assembly,))


# ----------------------------------------------------------------------------------------- point-cloud Laplacian (local Delaunay stars)
STAR_CR_TOL = 1e-12   # |cross(a, b)| <= STAR_CR_TOL sqrt(W_a W_b): a, b and the centre are collinear (dn_cloud_lap.hip: LP_CR_TOL)


def cloud_project(pts: np.ndarray, nbr: np.ndarray, frames: np.ndarray):
    """Tangent-plane coordinates of every neighbour about its point: X, Y, W = X^2 + Y^2, each [V, k] fp64.  A slot whose index is the
    point itself, or that projects onto it, has W = 0 and takes no part in the star."""
    pts, frames = np.asarray(pts, dtype=np.float64), np.asarray(frames, dtype=np.float64).reshape(-1, 3, 3)
    e = pts[nbr] - pts[:, None, :]
    X = np.einsum("nkd,nd->nk", e, frames[:, 0])
    Y = np.einsum("nkd,nd->nk", e, frames[:, 1])
    own = nbr == np.arange(pts.shape[0])[:, None]
    X, Y = np.where(own, 0.0, X), np.where(own, 0.0, Y)
    W = X * X + Y * Y
    dead = ~(W > 0)
    return np.where(dead, 0.0, X), np.where(dead, 0.0, Y), np.where(dead, 0.0, W)


def _incircle(xa, ya, wa, xb, yb, wb, cr_ab, xc, yc, wc):
    """< 0: c strictly inside circle(0, a, b) for (a, b) counter-clockwise (cr_ab > 0)."""
    return wc * cr_ab - wb * (xa * yc - ya * xc) + wa * (xb * yc - yb * xc)


def cloud_stars(X: np.ndarray, Y: np.ndarray, W: np.ndarray) -> np.ndarray:
    """partner [V, k] int32: slot b of the star triangle {a, b} of the origin with cross(a, b) > 0, or -1 -- the triangles at the origin of
    the planar Delaunay triangulation of {0} u {(X_a, Y_a)}.  Slot a pivots over the slots c on its counter-clockwise side (c replaces
    the candidate b when it is strictly inside circle(0, a, b)), then the circle is checked against every slot; ties are not inside, so
    the lower slot is kept.  2 k vectorised steps over all slots at once."""
    V, k = X.shape
    slot = np.arange(k)[None, :]
    partner = np.full((V, k), -1, dtype=np.int32)
    xb, yb, wb, cr_ab = (np.zeros((V, k)) for _ in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(k):
            xc, yc, wc = X[:, c:c + 1], Y[:, c:c + 1], W[:, c:c + 1]
            cr_ac = X * yc - Y * xc
            cand = (W > 0) & (wc > 0) & (slot != c) & (cr_ac > STAR_CR_TOL * np.sqrt(W * wc))
            take = cand & ((partner < 0) | (_incircle(X, Y, W, xb, yb, wb, cr_ab, xc, yc, wc) < 0))
            partner = np.where(take, np.int32(c), partner)
            xb, yb, wb, cr_ab = np.where(take, xc, xb), np.where(take, yc, yb), np.where(take, wc, wb), np.where(take, cr_ac, cr_ab)
        empty = partner >= 0
        for c in range(k):
            xc, yc, wc = X[:, c:c + 1], Y[:, c:c + 1], W[:, c:c + 1]
            inside = (wc > 0) & (slot != c) & (partner != c) & (_incircle(X, Y, W, xb, yb, wb, cr_ab, xc, yc, wc) < 0)
            empty &= ~inside
    return np.where(empty, partner, np.int32(-1))


def cloud_laplacian_terms(pts: np.ndarray, nbr: np.ndarray, partner: np.ndarray):
    """The per-triangle terms of the Laplacian and the mass: for every filled slot (i, a) with b = partner[i, a] the lifted triangle
    (i, nbr[i, a], nbr[i, b]) gives, per corner, w = cot / 2 / 3 on the opposite edge (-w off the diagonal, +w on both diagonals) and
    area / 3 / 3 to every vertex.  -> (rows, cols, vals) of L with one term per edge end, (verts, vals) of the mass, all concatenated."""
    pts = np.asarray(pts, dtype=np.float64)
    i, a = np.nonzero(partner >= 0)
    v0, v1, v2 = i, nbr[i, a], nbr[i, partner[i, a]]
    u, v = pts[v1] - pts[v0], pts[v2] - pts[v0]
    t = v - u
    with np.errstate(invalid="ignore", divide="ignore"):
        cn = np.linalg.norm(np.cross(u, v), axis=1)
        w12 = np.einsum("ij,ij->i", u, v) / cn / 6.0
        w02 = -np.einsum("ij,ij->i", u, t) / cn / 6.0
        w01 = np.einsum("ij,ij->i", v, t) / cn / 6.0
    keep = (cn > 0) & np.isfinite(w12) & np.isfinite(w02) & np.isfinite(w01) & (v1 != v0) & (v2 != v0) & (v1 != v2)
    v0, v1, v2, cn, w12, w02, w01 = (x[keep] for x in (v0, v1, v2, cn, w12, w02, w01))
    rows, cols, vals = [], [], []
    for p, q, w in ((v0, v1, w01), (v0, v2, w02), (v1, v2, w12)):
        rows += [p, q, p, q]
        cols += [p, q, q, p]
        vals += [w, w, -w, -w]
    m = cn / 18.0
    return (np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)), (np.concatenate([v0, v1, v2]), np.concatenate([m, m, m]))


def point_cloud_laplacian_from_table(pts, nbr, frames, with_parts=False):
    """``point_cloud_laplacian_host`` on a given neighbour table [V, k] and given frames [V, 3, 3]: (L scipy CSR fp64, mass [V] fp64).
    ``with_parts``: also a dict with ``partner`` [V, k] and the sums of the ABSOLUTE terms of every entry, ``L_abs`` (CSR, the pattern of
    L) and ``mass_abs`` -- what a rounding of the entry is measured against."""
    pts = np.asarray(pts, dtype=np.float64)
    nbr = np.asarray(nbr).astype(np.int64)
    V = pts.shape[0]
    if nbr.size and (nbr.min() < 0 or nbr.max() >= V):
        raise IndexError("point-cloud Laplacian: the neighbour table holds an index outside [0, %d)" % V)
    partner = cloud_stars(*cloud_project(pts, nbr, frames))
    (rows, cols, vals), (mv, mw) = cloud_laplacian_terms(pts, nbr, partner)
    # every term stands under (i, j) and under (j, i): sum the upper copies (in the order of the slots) and mirror them -- L == L^T exactly
    up = rows <= cols
    ukey, inv = np.unique(rows[up] * np.int64(V) + cols[up], return_inverse=True)
    r, c = ukey // V, ukey % V
    off = r != c

    def assemble(terms):
        s = np.bincount(inv, weights=terms, minlength=len(ukey))
        m = sp.coo_matrix((np.concatenate([s, s[off]]), (np.concatenate([r, c[off]]), np.concatenate([c, r[off]]))), shape=(V, V)).tocsr()
        m.sort_indices()
        return m

    L = assemble(vals[up])
    mass = np.bincount(mv, weights=mw, minlength=V)
    if not with_parts:
        return L, mass
    return L, mass, dict(partner=partner, L_abs=assemble(np.abs(vals[up])), mass_abs=mass)


def point_cloud_laplacian_host(v64, n_neighbors=30, frames=None):
    """Laplacian and lumped mass of a point cloud, (L scipy CSR [V, V] fp64, mass [V] fp64): the local-Delaunay construction of Sharp &
    Crane, "A Laplacian for Nonmanifold Triangle Meshes" (2020), section 5.7 -- every point's ``n_neighbors`` nearest neighbours are
    projected on its tangent plane, the star of the point in their planar Delaunay triangulation gives triangles, and L and the mass are
    the cotan Laplacian and the vertex areas of all those triangles, each weighted 1/3 -- WITHOUT the intrinsic Delaunay / tufted-cover
    re-triangulation that ``robust_laplacian.point_cloud_laplacian`` then applies.  L is symmetric, has zero row sums and is positive
    semi-definite for any input (a sum of per-triangle Dirichlet forms); single weights can be negative on bad samplings.

    ``v64`` [V, 3] positions (numpy or torch), ``frames`` [V, 3, 3] tangent frames (rows basisX, basisY, normal) or None: those of the
    normals estimated from the same neighbourhoods, as ``geometry.cloud_operators`` does on the host.  Vectorised numpy in fp64; the HIP
    route (``ops.cloud_laplacian``, dn_cloud_lap.hip) is the same arithmetic.  A valid ``laplacian=`` callable of ``compute_operators``."""
    from .geometry import find_knn                 # (geometry imports this module)
    pts = v64.detach().cpu().numpy() if isinstance(v64, torch.Tensor) else np.asarray(v64)
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    V, k = pts.shape[0], int(n_neighbors)
    t = torch.from_numpy(pts)
    nbr = find_knn(t, t, k, omit_diagonal=True, method="cpu_kd").indices.numpy()
    if frames is None:
        frames = tangent_frames(neighborhood_normal(pts[nbr] - pts[:, None, :]))
    elif isinstance(frames, torch.Tensor):
        frames = frames.detach().cpu().numpy()
    return point_cloud_laplacian_from_table(pts, nbr, np.asarray(frames, dtype=np.float64).reshape(V, 3, 3))


# ----------------------------------------------------------------------------------------- torch-facing API
def _to_torch_sparse(mat, device, dtype):
    coo = mat.tocoo()
    idx = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(coo.data.astype(np.float64)), coo.shape).coalesce().to(device=device, dtype=dtype)


def _cloud_laplacian(v64, laplacian):
    """(L, massvec) of a point cloud: the caller's pair, the caller's function of the fp64 positions, or robust_laplacian's."""
    if laplacian is None:
        try:
            import robust_laplacian
        except ImportError as err:
            raise ImportError(
                "compute_operators on a point cloud (empty faces) needs a point-cloud Laplacian, which this package does not restate: "
                "either pass laplacian=(L, massvec) or laplacian=<callable: fp64 positions [V,3] -> (L, M)>, "
                "or install the robust_laplacian package (its point_cloud_laplacian is then used, as in the reference); "
                "laplacian=\"delaunay\" builds this package's own local-Delaunay Laplacian instead") from err
        laplacian = robust_laplacian.point_cloud_laplacian
    L, M = laplacian(v64) if callable(laplacian) else laplacian
    if isinstance(M, torch.Tensor):
        M = M.detach().cpu().numpy()
    mass = M.diagonal() if sp.issparse(M) or np.ndim(M) == 2 else np.asarray(M)
    mass = np.asarray(mass, dtype=np.float64).reshape(-1)
    L = sp.csr_matrix(L).astype(np.float64)
    if L.shape != (v64.shape[0], v64.shape[0]) or mass.shape != (v64.shape[0],):
        raise ValueError("laplacian: L %s and mass %s do not fit %d points" % (L.shape, mass.shape, v64.shape[0]))
    return L, mass


def _compute_cloud_operators(verts, k_eig, normals, laplacian, n_neighbors_cloud=30, eigensolver=None):
    """The point-cloud branch of ``compute_operators`` (geometry.py:306-392 with is_cloud)."""
    from . import geometry                         # (geometry imports this module)
    device, dtype = verts.device, verts.dtype
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    if isinstance(laplacian, str):
        if laplacian != "delaunay":
            raise ValueError("laplacian=%r: the only named point-cloud Laplacian is \"delaunay\"" % laplacian)
        # the frames and the neighbour table of the gradient operator serve the stars too; on a ROCm device nothing but the eigenproblem
        # (scipy's shift-invert Lanczos, as for meshes) runs on the host
        frames, gradX, gradY, nbr = geometry._cloud_operators_and_table(verts, n_neighbors_cloud, normals)
        Lt, mass_t = geometry._laplacian_of_table(verts, nbr, frames)
        L = _sparse_to_csc(Lt).astype(np.float64).tocsr()
        mass = mass_t.detach().cpu().numpy().astype(np.float64)
        mass = mass + EPS * mass.mean()
        if np.isnan(L.data).any():
            raise RuntimeError("NaN Laplace matrix")
        if np.isnan(mass).any():
            raise RuntimeError("NaN mass matrix")
        evals, evecs = _eigenbasis(L, mass, k_eig, eigensolver, device)
        return frames, t(mass), Lt, t(evals), t(evecs), gradX, gradY
    frames, gradX, gradY = geometry.cloud_operators(verts, n_neighbors_cloud, normals=normals)
    v64 = verts.detach().cpu().numpy().astype(np.float64)
    L, mass = _cloud_laplacian(v64, laplacian)
    if np.isnan(L.data).any():
        raise RuntimeError("NaN Laplace matrix")
    if np.isnan(mass).any():
        raise RuntimeError("NaN mass matrix")
    evals, evecs = _eigenbasis(L, mass, k_eig, eigensolver, device)
    return frames, t(mass), _to_torch_sparse(L, device, dtype), t(evals), t(evecs), gradX, gradY


def compute_operators(verts, faces, k_eig, normals=None, *, laplacian=None):
    """Same contract as the reference's ``compute_operators`` (geometry.py:276-392), torch in / torch out:
    returns (frames [V,3,3], massvec [V], L sparse, evals [k], evecs [V,k], gradX sparse, gradY sparse).

    Empty ``faces``: a point cloud.  Frames and gradients are those of ``geometry.cloud_operators`` (30 neighbours, as the reference);
    the Laplacian and the mass come from ``laplacian`` -- ``(L scipy sparse, massvec)`` or a callable taking the fp64 positions [V,3] and
    returning ``(L, M)`` (M a diagonal sparse matrix or a vector) -- or, without it, from ``robust_laplacian.point_cloud_laplacian`` if
    that package is installed (ImportError otherwise).  ``laplacian="delaunay"``: this package's own local-Delaunay Laplacian
    (``point_cloud_laplacian_host``: Sharp & Crane 2020, section 5.7, without the intrinsic / tufted re-triangulation of robust_laplacian)
    on the frames and the neighbour table the gradient operator is built from -- on a ROCm device by the HIP kernels of
    dn_cloud_lap.hip (``ops.cloud_laplacian``), otherwise in numpy -- with EPS x the mean mass added to the mass, as for a mesh.

    The eigenbasis is shift-invert ``eigsh`` on the host, as the reference's; ``compute_operators_with`` takes the choice of another solver
    (this function keeps the parameter list it has had)."""
    return compute_operators_with(verts, faces, k_eig, normals, laplacian=laplacian, eigensolver=None)


def _compute_mesh_operators_device(verts, faces, k_eig, normals, eigensolver):
    """The mesh branch of ``compute_operators_via`` under ``assembly="device"``: normals, frames, L, mass and the gradient operator by
    ``geometry._mesh_operators_fp64`` (dn_mesh.hip); the eigenproblem gets the fp64 CSR and mass, downloaded once."""
    from . import geometry                         # (geometry imports this module)
    device, dtype = verts.device, verts.dtype
    V = verts.shape[0]
    rowptr, col, lval, mass_t, frames, gx, gy = geometry._mesh_operators_fp64(verts, faces, normals)
    mass_t = mass_t + EPS * mass_t.mean()
    L = sp.csr_matrix((lval.cpu().numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(V, V))
    mass = mass_t.cpu().numpy()
    if np.isnan(L.data).any():
        raise RuntimeError("NaN Laplace matrix")
    if np.isnan(mass).any():
        raise RuntimeError("NaN mass matrix")
    evals, evecs = _eigenbasis(L, mass, k_eig, eigensolver, device)
    idx = torch.stack((geometry._csr_rows(rowptr, col.numel()), col.to(torch.int64)))
    sparse = lambda v: torch.sparse_coo_tensor(idx, v.to(dtype), (V, V), is_coalesced=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    return frames.to(dtype), mass_t.to(dtype), sparse(lval), t(evals), t(evecs), sparse(gx), sparse(gy)


def compute_operators_with(verts, faces, k_eig, normals=None, *, laplacian=None, eigensolver=None):
    """``compute_operators`` with the choice of the eigensolver (``get_operators`` and ``get_all_operators`` take the same keyword and pass it
    here).  ``eigensolver``: None -- shift-invert ``eigsh`` on the host, as the reference -- or ``"subspace"``:
    ``geometry.laplacian_eigenbasis``, Chebyshev-filtered subspace iteration whose products run on the device (dn_eigen.hip) where there is
    one, for meshes and for both point-cloud branches alike.  The pairs solve the same pencil to ``rtol = 1e-9``; the eigenvectors differ by
    sign (and by a rotation inside a repeated eigenvalue), the six other outputs are identical.  Anything else: ``ValueError``.
    (This function keeps the parameter list it has had, as ``compute_operators`` did: ``compute_operators_via`` adds ``assembly``.)"""
    return compute_operators_via(verts, faces, k_eig, normals, laplacian=laplacian, eigensolver=eigensolver, assembly=None)


def compute_operators_via(verts, faces, k_eig, normals=None, *, laplacian=None, eigensolver=None, assembly=None):
    """``compute_operators_with`` with the choice of where a mesh is assembled (``get_operators`` and ``get_all_operators`` take the same
    keyword and pass it here).  ``assembly``: None -- the normals, frames, cotan Laplacian, mass and gradient operator of a MESH come from the fp64 host functions of
    this module and are uploaded -- or ``"device"``: fp32 positions on a ROCm device are assembled there by the kernels of dn_mesh.hip
    (``geometry.mesh_operators``: fp64 inside, no floating-point atomics, the gradient operator on L's own pattern); the eigenproblem gets
    the fp64 L and mass, downloaded once, and the seven outputs are rounded to the dtype of ``verts`` once.  The two routes sum the same
    terms in another order: they agree to fp64 round-off before that rounding.  Without a device, and for positions that are not fp32,
    ``"device"`` is the host route; a point cloud (empty ``faces``) chooses its own route either way.  Anything else: ``ValueError``."""
    _check_eigensolver(eigensolver)
    _check_assembly(assembly)
    device, dtype = verts.device, verts.dtype
    if faces.numel() == 0:
        return _compute_cloud_operators(verts, k_eig, normals, laplacian, eigensolver=eigensolver)
    if laplacian is not None:
        raise ValueError("laplacian= is for point clouds (empty faces); a triangle mesh gets its cotan Laplacian")
    if assembly == "device":
        from . import geometry                     # (geometry imports this module)
        if geometry._mesh_on_device(verts):
            return _compute_mesh_operators_device(verts, faces, k_eig, normals, eigensolver)
    v = verts.detach().cpu().numpy().astype(np.float64)
    f = faces.detach().cpu().numpy().astype(np.int64)
    n = vertex_normals(v, f) if normals is None else normals.detach().cpu().numpy().astype(np.float64)
    frames = tangent_frames(n)
    L = cotan_laplacian(v, f, denom_eps=1e-10)
    mass = vertex_areas(v, f)
    mass = mass + EPS * mass.mean()
    if np.isnan(L.data).any():
        raise RuntimeError("NaN Laplace matrix")
    if np.isnan(mass).any():
        raise RuntimeError("NaN mass matrix")
    evals, evecs = _eigenbasis(L, mass, k_eig, eigensolver, device)
    Lc = L.tocoo()
    grad = gradient_operator(v, frames, np.stack([Lc.row, Lc.col]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    return (t(frames), t(mass), _to_torch_sparse(L, device, dtype), t(evals), t(evecs),
            _to_torch_sparse(grad.real, device, dtype), _to_torch_sparse(grad.imag, device, dtype))


def _sparse_to_csc(t):
    idx, val = t.coalesce().indices().cpu().numpy(), t.coalesce().values().cpu().numpy()
    return sp.coo_matrix((val, (idx[0], idx[1])), shape=tuple(t.shape)).tocsc()


def get_operators(verts, faces, k_eig=128, op_cache_dir=None, normals=None, overwrite_cache=False, *, laplacian=None, eigensolver=None,
                  assembly=None):
    """``compute_operators`` behind the reference's on-disk npz cache (geometry.py:426-570): same key derivation, same
    file names, same array names (float32 payload, CSC triplets for L / gradX / gradY), so either implementation can
    read the other's cache.  A hit is verified against the stored verts/faces; an entry with too few eigenpairs is
    rebuilt.  ``laplacian``: passed on to ``compute_operators`` (point clouds).  The key is the reference's -- positions and faces only --
    so a hit cannot tell which Laplacian wrote the entry: a cache directory should be filled with one ``laplacian`` choice.
    ``eigensolver``: None or "subspace" (``compute_operators_with``); it is not part of the key either, so the same holds: a cache directory
    should be filled with one ``eigensolver`` choice.
    ``assembly``: None or "device" (``compute_operators_via``: where a mesh's operators are assembled).  It is not part of the key either;
    the two routes agree to fp64 round-off before the fp32 payload is written, so an entry of one serves the other."""
    _check_eigensolver(eigensolver)
    _check_assembly(assembly)
    device, dtype = verts.device, verts.dtype
    v_np, f_np = verts.detach().cpu().numpy(), faces.detach().cpu().numpy()
    if np.isnan(v_np).any():
        raise RuntimeError("tried to construct operators from NaN verts")
    path = None
    if op_cache_dir is not None:
        os.makedirs(op_cache_dir, exist_ok=True)
        key = hash_arrays((v_np, f_np))
        bucket = 0
        while True:
            path = os.path.join(op_cache_dir, f"{key}_{bucket}.npz")
            if not os.path.exists(path):
                break
            try:
                z = np.load(path, allow_pickle=True)
                if not (np.array_equal(v_np, z["verts"]) and np.array_equal(f_np, z["faces"])):
                    bucket += 1            # hash collision: next bucket
                    continue
                if overwrite_cache or int(z["k_eig"].item()) < k_eig or "L_data" not in z:
                    os.remove(path)
                    break
                rd = lambda p: sp.csc_matrix((z[p + "_data"], z[p + "_indices"], z[p + "_indptr"]), shape=tuple(z[p + "_shape"]))
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
                return (t(z["frames"]), t(z["mass"]), _to_torch_sparse(rd("L"), device, dtype), t(z["evals"][:k_eig]),
                        t(z["evecs"][:, :k_eig]), _to_torch_sparse(rd("gradX"), device, dtype),
                        _to_torch_sparse(rd("gradY"), device, dtype))
            except Exception:              # unreadable entry: rebuild in place  # noqa: BLE001
                break
    if eigensolver is None and assembly is None:
        out = compute_operators(verts, faces, k_eig, normals=normals, laplacian=laplacian)
    elif assembly is None:
        out = compute_operators_with(verts, faces, k_eig, normals=normals, laplacian=laplacian, eigensolver=eigensolver)
    else:
        out = compute_operators_via(verts, faces, k_eig, normals=normals, laplacian=laplacian, eigensolver=eigensolver, assembly=assembly)
    if path is not None:
        frames, mass, L, evals, evecs, gX, gY = out
        f32 = lambda a: a.detach().cpu().numpy().astype(np.float32)
        Lc, gXc, gYc = (_sparse_to_csc(m).astype(np.float32) for m in (L, gX, gY))
        np.savez(path, verts=v_np.astype(np.float32), frames=f32(frames), faces=f_np, k_eig=k_eig, mass=f32(mass),
                 L_data=Lc.data, L_indices=Lc.indices, L_indptr=Lc.indptr, L_shape=Lc.shape,
                 evals=f32(evals), evecs=f32(evecs),
                 gradX_data=gXc.data, gradX_indices=gXc.indices, gradX_indptr=gXc.indptr, gradX_shape=gXc.shape,
                 gradY_data=gYc.data, gradY_indices=gYc.indices, gradY_indptr=gYc.indptr, gradY_shape=gYc.shape)
    return out


def get_all_operators(verts_list, faces_list, k_eig, op_cache_dir=None, normals=None, *, laplacian=None, eigensolver=None, assembly=None):
    """Lists in, seven lists out (geometry.py:395-424).  ``laplacian``: None, one value for every entry, or a list with one per entry.
    ``eigensolver``, ``assembly``: one value for every entry (``compute_operators_with``, ``compute_operators_via``)."""
    _check_eigensolver(eigensolver)
    _check_assembly(assembly)
    cols = [[] for _ in range(7)]
    for i, (v, f) in enumerate(zip(verts_list, faces_list)):
        lap = laplacian[i] if isinstance(laplacian, list) else laplacian
        res = get_operators(v, f, k_eig, op_cache_dir, normals=None if normals is None else normals[i], laplacian=lap, eigensolver=eigensolver,
                            assembly=assembly)
        for c, r in zip(cols, res):
            c.append(r)
    return tuple(cols)


def normalize_positions(pos, faces=None, method="mean", scale_method="max_rad"):
    """Centre and unit-scale vertex positions (geometry.py:635-665)."""
    if method == "mean":
        pos = pos - pos.mean(dim=-2, keepdim=True)
    elif method == "bbox":
        lo, hi = pos.min(dim=-2).values, pos.max(dim=-2).values
        pos = pos - ((hi + lo) / 2.0).unsqueeze(-2)
    else:
        raise ValueError("unrecognized method")
    if scale_method == "max_rad":
        return pos / pos.norm(dim=-1).max(dim=-1, keepdim=True).values.unsqueeze(-1)
    if scale_method == "area":
        if faces is None:
            raise ValueError("must pass faces for area normalization")
        c = pos[faces]
        area = 0.5 * torch.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], dim=-1).norm(dim=1).sum()
        return pos * (1.0 / torch.sqrt(area))
    raise ValueError("unrecognized scale method")


def compute_hks(evals, evecs, scales):
    """Heat-kernel signature sum_k exp(-lambda_k s) phi_k(v)^2 -> (V,S) or (B,V,S) (geometry.py:600-628)."""
    squeeze = evals.dim() == 1
    if squeeze:
        evals, evecs, scales = evals[None], evecs[None], scales[None]
    coefs = torch.exp(-evals.unsqueeze(1) * scales.unsqueeze(-1))          # (B,S,K)
    out = torch.einsum("bsk,bvk->bvs", coefs, evecs * evecs)
    return out[0] if squeeze else out


def compute_hks_autoscale(evals, evecs, count):
    scales = torch.logspace(-2, 0.0, steps=count, device=evals.device, dtype=evals.dtype)   # geometry.py:630-633
    return compute_hks(evals, evecs, scales)

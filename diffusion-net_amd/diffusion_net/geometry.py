"""``diffusion_net.geometry`` -- the two basis transforms on the hot path, HIP-backed.

Signatures follow the reference (geometry.py:572-598): batched tensors, basis [B,V,K],
values [B,V,C] / [B,K,C], massvec [B,V] (an unbatched leading dimension is accepted too).
The host-side operator precompute keeps the reference's names here (``compute_operators``, ``get_operators``,
``get_all_operators``, ``normalize_positions``, ``compute_hks[_autoscale]``) and lives in ``precompute.py``
(numpy/scipy restatement).  ``find_knn`` is the nearest-neighbour query of the evaluation scripts and of the
point-cloud operators: ``vertex_normals``, ``build_tangent_frames``, ``build_grad_point_cloud`` (the reference's names) and
``cloud_operators`` (normals, frames and gradient stencils of a cloud in one HIP pass over its neighbour table).
"""
from collections import namedtuple

import torch

from . import ops
from .batch import MeshBatch
from .precompute import compute_operators, get_all_operators, get_operators, neighborhood_normal, normalize_positions  # noqa: F401
from . import precompute as _pre


def _spectral_batch(basis, massvec):
    if basis.dim() == 2:
        basis = basis[None]
        massvec = massvec[None] if massvec is not None else None
    B, V, K = basis.shape
    if massvec is None:
        massvec = torch.ones(B, V, dtype=basis.dtype, device=basis.device)
    return MeshBatch.from_reference_args(massvec, torch.zeros(B, K, dtype=basis.dtype, device=basis.device), basis)


def to_basis(values, basis, massvec):
    """(B,V,D),(B,V,K),(B,V) -> (B,K,D): basis^T (values * mass)."""
    mb = _spectral_batch(basis, massvec)
    D = values.shape[-1]
    spec = ops.ToBasisFn.apply(values.reshape(-1, D), mb)
    return spec if values.dim() == 3 else spec[0]


def from_basis(values, basis):
    """(B,K,D),(B,V,K) -> (B,V,D): basis @ values."""
    if values.is_complex() or basis.is_complex():
        raise NotImplementedError("complex basis transforms are dead code in the reference (geometry.py:595-596)")
    mb = _spectral_batch(basis, None)
    D = values.shape[-1]
    out = ops.FromBasisFn.apply(values.reshape(mb.n_mesh, -1, D), mb)
    return out.reshape(*basis.shape[:-1], D)


def compute_hks(evals, evecs, scales):
    """Heat kernel signature (geometry.py:600-628): (K),(V,K),(S) -> (V,S), or batched (B,K),(B,V,K),(B,S) -> (B,V,S).
    On a ROCm device and outside autograd this is one streaming HIP pass over the eigenbasis (``dn_hks_f32``); host
    tensors (the reference computes it in its CPU dataset loaders) and differentiable calls use the torch formula."""
    on_dev = evecs.is_cuda and evals.is_cuda and scales.is_cuda and evecs.dtype == torch.float32
    if not on_dev or evecs.requires_grad or evals.requires_grad or scales.requires_grad:
        return _pre.compute_hks(evals, evecs, scales)
    return ops.hks(evals, evecs, scales)


def compute_hks_autoscale(evals, evecs, count):
    scales = torch.logspace(-2, 0.0, steps=count, device=evals.device, dtype=evals.dtype)   # geometry.py:630-633
    return compute_hks(evals, evecs, scales)


KnnResult = namedtuple("KnnResult", ["values", "indices"])
_KNN_CHUNK_PAIRS = 1 << 26     # pairs per distance block of the torch path ...
_KNN_CHUNK_ELEMS = 1 << 27     # ... and elements of its N x M x D difference block


def _knn_torch(source, target, k, largest, omit_diagonal):
    """Row blocks of the reference's own formula -- norm of the expanded difference -- and ``topk`` of each: differentiable, any dtype, any
    k <= M, bounded memory (at most 2^26 pairs and 2^27 difference elements at a time).  Not ``torch.cdist``: past some ten million pairs
    per call its non-matmul mode returned wrong distances on the device (measured at both workload shapes, tools/knn_timing.py), and its
    matmul mode is the |a|^2 + |b|^2 - 2ab expansion, whose cancellation reorders near neighbours."""
    N, M, D = source.shape[0], target.shape[0], source.shape[1]
    rows = max(1, min(N, _KNN_CHUNK_PAIRS // max(M, 1), _KNN_CHUNK_ELEMS // max(M * D, 1)))
    masked = float("-inf") if largest else float("inf")
    vals, inds = [], []
    for r0 in range(0, N, rows):
        d = (source[r0:r0 + rows, None, :] - target[None, :, :]).norm(dim=-1)
        if omit_diagonal:
            own = torch.arange(r0, r0 + d.shape[0], device=d.device)[:, None] == torch.arange(M, device=d.device)[None, :]
            d = d.masked_fill(own, masked)
        top = torch.topk(d, k=k, largest=largest, sorted=True)
        vals.append(top.values)
        inds.append(top.indices)
    if not vals:
        return KnnResult(source.new_empty(0, k), torch.empty(0, k, dtype=torch.int64, device=source.device))
    return KnnResult(torch.cat(vals), torch.cat(inds))


def _knn_kdtree(source, target, k, omit_diagonal):
    """Host route of ``method='cpu_kd'``: an sklearn KD-tree over the targets, distances recomputed in torch from the indices."""
    import numpy as np
    from sklearn.neighbors import KDTree    # only this route needs sklearn: the package does not import it otherwise
    from .utils import toNP
    tree = KDTree(toNP(target))
    nbr = tree.query(toNP(source), k=k + 1 if omit_diagonal else k, return_distance=False)
    if omit_diagonal:
        # Drop the point itself from its row; a row where duplicates pushed it out of the k + 1 hits loses its last hit instead.
        keep = nbr != np.arange(nbr.shape[0])[:, None]
        keep[keep.all(axis=1), -1] = False
        nbr = nbr[keep].reshape(nbr.shape[0], k)
    inds = torch.as_tensor(nbr, dtype=torch.int64, device=source.device)
    return KnnResult((source[:, None, :] - target[inds]).norm(dim=-1), inds)


def find_knn(points_source, points_target, k, largest=False, omit_diagonal=False, method="brute"):
    """The k nearest neighbours of every source point among the target points (geometry.py:667-724): ``(values, indices)``, sorted in
    increasing distance (``largest``: the k farthest, decreasing).  The result unpacks as a pair and has ``.values`` / ``.indices``.

    fp32 tensors on a ROCm device with nothing requiring grad and k <= 32 run the exact HIP search (``ops.knn``) for ``'brute'`` AND
    ``'cpu_kd'`` -- both are exact searches, so the evaluation scripts' ``method='cpu_kd'`` never leaves the device, and there is no size
    switch.  Other device tensors take a row-chunked torch path (the reference's difference formula; differentiable, as its ``'brute'`` branch); host tensors do what
    the reference does (``'brute'``: torch, ``'cpu_kd'``: ``sklearn.neighbors.KDTree``).
    Difference from the reference: with duplicate points and ``omit_diagonal`` its KD-tree branch may drop a duplicate other than the point
    itself; the device routes always exclude index i.  The distances are identical."""
    if omit_diagonal and points_source.shape[0] != points_target.shape[0]:
        raise ValueError("omit_diagonal can only be used when source and target are same shape")
    if method not in ("brute", "cpu_kd"):
        raise ValueError("unrecognized method")
    if method == "cpu_kd" and largest:
        raise ValueError("can't do largest with cpu_kd")
    if points_source.device != points_target.device:
        raise RuntimeError("find_knn: source points on %s, target points on %s" % (points_source.device, points_target.device))
    k = int(k)
    if points_source.is_cuda:
        hip = (points_source.dtype == torch.float32 and points_target.dtype == torch.float32 and 1 <= k <= ops._hip.KNN_MAX_K
               and not points_source.requires_grad and not points_target.requires_grad)
        if not hip:
            return _knn_torch(points_source, points_target, k, largest, omit_diagonal)
        if torch.compiler.is_compiling():
            from . import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn)
            return KnnResult(*torch.ops.diffusion_net.knn(points_source, points_target, k, bool(largest), bool(omit_diagonal)))
        return KnnResult(*ops.knn(points_source, points_target, k, largest, omit_diagonal))
    if method == "cpu_kd":
        return _knn_kdtree(points_source, points_target, k, omit_diagonal)
    return _knn_torch(points_source, points_target, k, largest, omit_diagonal)


# ----------------------------------------------------------------------------------------------
# point clouds: normals, tangent frames, gradient operator (geometry.py:92-99, 114-123, 151-206)
# ----------------------------------------------------------------------------------------------
def _cloud_on_device(verts, n_neighbors_cloud):
    """fp32 points on a ROCm device with a neighbourhood the kernels take: ``ops.knn`` + ``ops.cloud_operators``.  (Host tensors take this
    route only while the test suite has bound the emulator build of the library, which runs the same kernels on host buffers.)"""
    return ((verts.is_cuda or ops._hip._allow_host_tensors) and verts.dtype == torch.float32
            and 1 <= int(n_neighbors_cloud) <= ops._hip.KNN_MAX_K)


def _cloud_neighbors(verts, n_neighbors_cloud):
    """[V, k] numpy indices of the reference's neighbourhood query (geometry.py:119, :184)."""
    return find_knn(verts, verts, int(n_neighbors_cloud), omit_diagonal=True, method="cpu_kd").indices.detach().cpu().numpy()


def _cloud_normals_host(verts, n_neighbors_cloud):
    """The reference's arithmetic: batched SVD of the neighbourhoods in the dtype of ``verts``, LAPACK's sign."""
    v = verts.detach().cpu().numpy()
    nbr = _cloud_neighbors(verts, n_neighbors_cloud)
    return torch.from_numpy(neighborhood_normal(v[nbr] - v[:, None, :])).to(device=verts.device, dtype=verts.dtype)


def vertex_normals(verts, faces, n_neighbors_cloud=30):
    """Unit vertex normals, torch in / torch out (geometry.py:114-148).  Mesh: normalised sum of the unit face normals (host code of
    ``precompute.vertex_normals``).  Point cloud (empty ``faces``): the direction of least spread of the ``n_neighbors_cloud`` nearest
    neighbours about the point -- on a ROCm device (fp32, at most 32 neighbours) by the HIP kernels, sign as include/diffnet_hip.h
    defines it (largest component positive); otherwise batched ``np.linalg.svd`` as in the reference, sign as LAPACK returns it."""
    if faces.numel() != 0:
        n = _pre.vertex_normals(verts.detach().cpu().numpy().astype("float64"), faces.detach().cpu().numpy().astype("int64"))
        normals = torch.from_numpy(n).to(device=verts.device, dtype=verts.dtype)
    elif _cloud_on_device(verts, n_neighbors_cloud):
        nbr = ops.knn(verts, verts, int(n_neighbors_cloud), omit_diagonal=True)[1]
        normals = ops.cloud_operators(verts, nbr)[0]
    else:
        normals = _cloud_normals_host(verts, n_neighbors_cloud)
    if torch.any(torch.isnan(normals)):
        raise ValueError("NaN normals :(")
    return normals


def _frames_of_normals(normals):
    """rows (basisX, basisY, normal): e_x -- e_y where |n_x| >= 0.9 -- projected on the tangent plane and divided by (norm + 1e-6),
    basisY = n x basisX (geometry.py:151-177, in the dtype and on the device of ``normals``)."""
    ex = torch.tensor([1.0, 0.0, 0.0], device=normals.device, dtype=normals.dtype)
    ey = torch.tensor([0.0, 1.0, 0.0], device=normals.device, dtype=normals.dtype)
    cand = torch.where((normals[:, 0].abs() < 0.9)[:, None], ex, ey)
    bx = cand - normals * (cand * normals).sum(dim=-1, keepdim=True)
    bx = bx / (bx.norm(dim=-1, keepdim=True) + 1e-6)
    by = torch.cross(normals, bx, dim=-1)
    frames = torch.stack((bx, by, normals), dim=-2)
    if torch.any(torch.isnan(frames)):
        raise ValueError("NaN coordinate frame! Must be very degenerate")
    return frames


def build_tangent_frames(verts, faces, normals=None):
    """(V,3,3) frames, rows basisX / basisY / normal (geometry.py:151-177); ``normals``: use these instead of ``vertex_normals``."""
    if normals is None:
        if faces.numel() == 0 and _cloud_on_device(verts, 30):
            return cloud_operators(verts)[0]        # the kernel's own frames (fp64 inside, rounded once)
        normals = vertex_normals(verts, faces)
    return _frames_of_normals(normals.to(device=verts.device, dtype=verts.dtype))


def build_grad_point_cloud(verts, frames, n_neighbors_cloud=30):
    """Complex (V,V) scipy CSC gradient operator of a point cloud in the GIVEN frames (geometry.py:179-194, 209-273): row i is the
    least-squares stencil over the edges to the ``n_neighbors_cloud`` nearest neighbours of i, real part X, imaginary part Y.  The
    result lives on the host, so only the neighbour query runs on the device (``find_knn``); the tangent coordinates are formed in the
    dtype of ``verts`` and the 2 x 2 systems solved in fp64, both as in the reference."""
    import numpy as np
    V, k = verts.shape[0], int(n_neighbors_cloud)
    nbr = find_knn(verts, verts, k, omit_diagonal=True, method="cpu_kd").indices
    tail = torch.arange(V, device=verts.device).repeat_interleave(k)
    tip = nbr.reshape(-1)
    frames = frames.to(device=verts.device, dtype=verts.dtype)
    d = verts[tip] - verts[tail]
    tx = (d * frames[tail, 0]).sum(dim=-1).detach().cpu().numpy().astype(np.float64)
    ty = (d * frames[tail, 1]).sum(dim=-1).detach().cpu().numpy().astype(np.float64)
    tail, tip = tail.cpu().numpy(), tip.cpu().numpy()
    keep = tail != tip
    return _pre.gradient_from_tangents(V, tail[keep], tip[keep], tx[keep], ty[keep])


def cloud_operators(verts, n_neighbors_cloud=30, normals=None):
    """Frames and gradient operator of a point cloud: ``(frames [V,3,3], gradX, gradY)``, gradX / gradY coalesced sparse COO [V,V], all on
    the device and in the dtype of ``verts``.  ``normals`` [V,3]: use these instead of estimating them.

    fp32 points on a ROCm device with ``n_neighbors_cloud <= 32`` run ``ops.knn`` and ``ops.cloud_operators`` (dn_knn.hip, dn_cloud.hip)
    and never touch the host: fp64 inside, normals signed as include/diffnet_hip.h defines.  Everything else (host tensors, fp64, larger
    neighbourhoods) takes the reference's arithmetic in vectorised numpy: ``find_knn`` (``cpu_kd``), batched SVD in the dtype of
    ``verts`` with LAPACK's sign, frames in that dtype, 2 x 2 systems in fp64."""
    V = verts.shape[0]
    if _cloud_on_device(verts, n_neighbors_cloud):
        k = int(n_neighbors_cloud)
        nbr = ops.knn(verts, verts, k, omit_diagonal=True)[1]
        if normals is not None:
            normals = normals.to(device=verts.device, dtype=torch.float32)
        _, frames, _, col, vx, vy = ops.cloud_operators(verts, nbr, normals)
        idx = torch.stack((torch.arange(V, device=verts.device).repeat_interleave(k + 1), col.to(torch.int64)))
        gradX = torch.sparse_coo_tensor(idx, vx, (V, V)).coalesce()
        gradY = torch.sparse_coo_tensor(idx, vy, (V, V)).coalesce()
        return frames, gradX, gradY
    if normals is None:
        normals = _cloud_normals_host(verts, n_neighbors_cloud)
        if torch.any(torch.isnan(normals)):
            raise ValueError("NaN normals :(")
    frames = _frames_of_normals(normals.to(device=verts.device, dtype=verts.dtype))
    grad = build_grad_point_cloud(verts, frames, n_neighbors_cloud)
    return (frames, _pre._to_torch_sparse(grad.real, verts.device, verts.dtype), _pre._to_torch_sparse(grad.imag, verts.device, verts.dtype))

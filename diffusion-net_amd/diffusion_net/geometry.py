"""``diffusion_net.geometry`` -- the two basis transforms on the hot path, HIP-backed.

Signatures follow the reference (geometry.py:572-598): batched tensors, basis [B,V,K],
values [B,V,C] / [B,K,C], massvec [B,V] (an unbatched leading dimension is accepted too).
The host-side operator precompute keeps the reference's names here (``compute_operators``, ``get_operators``,
``get_all_operators``, ``normalize_positions``, ``compute_hks[_autoscale]``) and lives in ``precompute.py``
(numpy/scipy restatement).  ``find_knn`` is the nearest-neighbour query of the evaluation scripts and of the
point-cloud operators: ``vertex_normals``, ``build_tangent_frames``, ``build_grad_point_cloud`` (the reference's names) and
``cloud_operators`` (normals, frames and gradient stencils of a cloud in one HIP pass over its neighbour table);
``point_cloud_laplacian`` is the local-Delaunay Laplacian and mass of a cloud (dn_cloud_lap.hip on the device).
``farthest_point_sampling`` / ``farthest_point_samples`` thin a cloud (or a batch of clouds) with the sample loop on the device (dn_fps.hip);
``norm`` .. ``face_normals`` are the reference's torch vector helpers.
``mesh_operators`` assembles what a triangle mesh needs in front of the eigenproblem -- frames, mass, cotan Laplacian, gradient operator
-- on the device (dn_mesh.hip); ``compute_operators_via(..., assembly="device")`` builds the seven operators on it.
``geodesic_label_errors`` and ``get_all_pairs_geodesic_distance`` are the evaluation metric of the correspondence experiments: all-pairs
distances on the mesh's Steiner-point graph (``mesh_distance_graph``, ``geodesic_distances``), swept on the device by dn_geodesic.hip.
"""
from collections import namedtuple

import torch

from . import ops
from .batch import MeshBatch
from .precompute import compute_operators, get_all_operators, get_operators, neighborhood_normal, normalize_positions  # noqa: F401
from .precompute import compute_operators_via, compute_operators_with  # noqa: F401
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
    itself; the device routes always exclude index i.  The distances are identical.

    ``method='grid'`` (not in the reference): where the cell-grid kernel applies -- the conditions above and D <= 3, no ``largest`` -- the
    search is ``ops.knn_grid``, whose work grows with N k and whose result is ``ops.knn``'s bit for bit; everything else takes the route
    ``'brute'`` takes."""
    if omit_diagonal and points_source.shape[0] != points_target.shape[0]:
        raise ValueError("omit_diagonal can only be used when source and target are same shape")
    if method not in ("brute", "cpu_kd", "grid"):
        raise ValueError("unrecognized method")
    if method == "cpu_kd" and largest:
        raise ValueError("can't do largest with cpu_kd")
    if method == "grid" and largest:
        raise ValueError("can't do largest with grid")
    if points_source.device != points_target.device:
        raise RuntimeError("find_knn: source points on %s, target points on %s" % (points_source.device, points_target.device))
    k = int(k)
    if points_source.is_cuda:
        hip = (points_source.dtype == torch.float32 and points_target.dtype == torch.float32 and 1 <= k <= ops._hip.KNN_MAX_K
               and not points_source.requires_grad and not points_target.requires_grad)
        if not hip:
            return _knn_torch(points_source, points_target, k, largest, omit_diagonal)
        grid = method == "grid" and points_source.dim() == 2 and points_source.shape[1] <= 3
        if torch.compiler.is_compiling():
            from . import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.knn, knn_grid)
            if grid:
                return KnnResult(*torch.ops.diffusion_net.knn_grid(points_source, points_target, k, bool(omit_diagonal), 0))
            return KnnResult(*torch.ops.diffusion_net.knn(points_source, points_target, k, bool(largest), bool(omit_diagonal)))
        if grid:
            return KnnResult(*ops.knn_grid(points_source, points_target, k, omit_diagonal))
        return KnnResult(*ops.knn(points_source, points_target, k, largest, omit_diagonal))
    if method == "cpu_kd":
        return _knn_kdtree(points_source, points_target, k, omit_diagonal)
    return _knn_torch(points_source, points_target, k, largest, omit_diagonal)


# ----------------------------------------------------------------------------------------------
# torch vector helpers (geometry.py:24-90) and farthest point sampling (geometry.py:727-751)
# ----------------------------------------------------------------------------------------------
def norm(x, highdim=False):
    """Length of every vector along the last dimension: (..., d) -> (...)."""
    return torch.norm(x, dim=len(x.shape) - 1)


def norm2(x, highdim=False):
    """Squared length of every vector along the last dimension."""
    return dot(x, x)


def normalize(x, divide_eps=1e-6, highdim=False):
    """Every vector divided by (its length + ``divide_eps``)."""
    if len(x.shape) == 1:
        raise ValueError("called normalize() on single vector of dim " + str(x.shape) + " are you sure?")
    if not highdim and x.shape[-1] > 4:
        raise ValueError("called normalize() with large last dimension " + str(x.shape) + " are you sure?")
    return x / (norm(x, highdim=highdim) + divide_eps).unsqueeze(-1)


def face_coords(verts, faces):
    return verts[faces]


def cross(vec_A, vec_B):
    return torch.cross(vec_A, vec_B, dim=-1)


def dot(vec_A, vec_B):
    return torch.sum(vec_A * vec_B, dim=-1)


def project_to_tangent(vecs, unit_normals):
    """(..., 3) vectors with their component along the (unit) normals removed."""
    dots = dot(vecs, unit_normals)
    return vecs - unit_normals * dots.unsqueeze(-1)


def _face_raw_normal(verts, faces):
    coords = face_coords(verts, faces)
    return cross(coords[:, 1, :] - coords[:, 0, :], coords[:, 2, :] - coords[:, 0, :])


def face_area(verts, faces):
    return 0.5 * norm(_face_raw_normal(verts, faces))


def face_normals(verts, faces, normalized=True):
    raw_normal = _face_raw_normal(verts, faces)
    return normalize(raw_normal) if normalized else raw_normal


def _fps_on_device(points):
    """fp32 [V, 3] points on a ROCm device with nothing requiring grad: the HIP sampler (``ops.fps``, dn_fps.hip).  (Host tensors take this
    route only while the tests have bound the emulator build of the same kernels.)"""
    return ((points.is_cuda or ops._hip._allow_host_tensors) and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 3 and points.shape[0] > 0 and not points.requires_grad)


def _fps_torch(points, n_sample):
    """The reference's loop.  On a device the index stays a tensor: no host round trip per sample."""
    N = points.shape[0]
    chosen_mask = torch.zeros(N, dtype=torch.bool, device=points.device)
    min_dists = torch.ones(N, dtype=points.dtype, device=points.device) * float("inf")
    points = normalize_positions(points)
    i = torch.min(norm2(points), dim=0).indices
    chosen_mask[i] = True
    for _ in range(n_sample - 1):
        dists = norm2(points[i, :].unsqueeze(0) - points)
        min_dists = torch.minimum(dists, min_dists)
        i = torch.max(min_dists, dim=0).indices
        if not points.is_cuda:
            i = i.item()
        chosen_mask[i] = True
    return chosen_mask


def farthest_point_sampling(points, n_sample):
    """A [V] bool mask with ``n_sample`` points set (geometry.py:727-751): the point nearest the centre of the normalised cloud first, then
    always the point farthest from those chosen so far; equal distances go to the lowest index.  ``n_sample == 0`` still sets the first
    point, and with more samples than distinct points the lowest index is chosen again, so fewer than ``n_sample`` may be set -- both as
    in the reference.

    fp32 [V, 3] points on a ROCm device with nothing requiring grad are normalised with torch on the device and sampled by ``ops.fps``
    (one launch for clouds up to ``ops._hip.FPS_RESIDENT_MAX_POINTS`` points, one per sample above); nothing synchronises with the host, so
    the call can be captured in a graph.  Other device tensors run the reference's loop with the index kept on the device; host tensors do
    what the reference does."""
    N = points.shape[0]
    if n_sample > N:
        raise ValueError("not enough points to sample")
    if not _fps_on_device(points):
        return _fps_torch(points, n_sample)
    pts = normalize_positions(points)
    if torch.compiler.is_compiling():
        from . import torchlib  # noqa: F401  (registers torch.ops.diffusion_net.fps)
        order = torch.ops.diffusion_net.fps(pts, max(int(n_sample), 1))[0]
    else:
        order = ops.fps(pts, max(int(n_sample), 1))[0][0]
    return torch.zeros(N, dtype=torch.bool, device=points.device).index_fill_(0, order, True)


def farthest_point_samples(points_list, n_sample):
    """``farthest_point_sampling`` of several clouds: the list of their masks.  Clouds the kernel takes (see there), all on one device, are
    normalised one by one, packed back to back and sampled by ONE ``ops.fps`` call; anything else is sampled cloud by cloud."""
    points_list = list(points_list)
    for p in points_list:
        if n_sample > p.shape[0]:
            raise ValueError("not enough points to sample")
    if (len(points_list) < 2 or not all(_fps_on_device(p) for p in points_list)
            or any(p.device != points_list[0].device for p in points_list)):
        return [farthest_point_sampling(p, n_sample) for p in points_list]
    sizes = [p.shape[0] for p in points_list]
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    packed = torch.cat([normalize_positions(p) for p in points_list])
    order = ops.fps(packed, max(int(n_sample), 1), offsets=offsets)[0]
    mask = torch.zeros(packed.shape[0], dtype=torch.bool, device=packed.device).index_fill_(0, order.reshape(-1), True)
    return list(mask.split(sizes))


# ----------------------------------------------------------------------------------------------
# point clouds: normals, tangent frames, gradient operator (geometry.py:92-99, 114-123, 151-206)
# ----------------------------------------------------------------------------------------------
def _cloud_on_device(verts, n_neighbors_cloud):
    """fp32 points on a ROCm device with a neighbourhood the kernels take: ``ops.knn`` + ``ops.cloud_operators``.  (Host tensors take this
    route only while the test suite has bound the emulator build of the library, which runs the same kernels on host buffers.)"""
    return ((verts.is_cuda or ops._hip._allow_host_tensors) and verts.dtype == torch.float32
            and 1 <= int(n_neighbors_cloud) <= ops._hip.KNN_MAX_K)


# Self-queries of clouds of at least this many points take the cell-grid search (``ops.knn_grid``: the same bits as ``ops.knn``, so the rule
# changes speed only).  None: the rule is off, every self-query is ``ops.knn``.  Measured (tools/knn_grid_timing.py,
# profiles/knn_grid_timing.txt): the smallest size from which the grid route is faster than brute force by more than twice the same-code
# spread on both inputs, at that and every larger measured size -- 1.8 x at 10 000 points, 28 x and 30 x at 200 000; at 2 000 points the
# uniform cube is slower on the grid (1.07 ms against 0.67 ms).
KNN_GRID_MIN_POINTS = 10000


def _cloud_self_knn(verts, k):
    """[V, k] int64 neighbour table of a cloud among its own points for the device kernels (``_cloud_on_device(verts, k)`` holds)."""
    if KNN_GRID_MIN_POINTS is not None and verts.shape[0] >= KNN_GRID_MIN_POINTS and verts.dim() == 2 and verts.shape[1] <= 3:
        return ops.knn_grid(verts, verts, int(k), omit_diagonal=True)[1]
    return ops.knn(verts, verts, int(k), omit_diagonal=True)[1]


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
        nbr = _cloud_self_knn(verts, n_neighbors_cloud)
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
    if verts.is_cuda and _cloud_on_device(verts, n_neighbors_cloud) and not verts.requires_grad:   # (where find_knn runs ops.knn)
        nbr = _cloud_self_knn(verts, n_neighbors_cloud)
    else:
        nbr = find_knn(verts, verts, int(n_neighbors_cloud), omit_diagonal=True, method="cpu_kd").indices
    return _grad_of_table(verts, frames, nbr)


def _grad_of_table(verts, frames, nbr):
    """``build_grad_point_cloud`` on a given neighbour table [V, k] (int64, on the device of ``verts``)."""
    import numpy as np
    V, k = nbr.shape
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
    return _cloud_operators_and_table(verts, n_neighbors_cloud, normals)[:3]


def _cloud_operators_and_table(verts, n_neighbors_cloud, normals):
    """``cloud_operators`` and the neighbour table [V, k] (int64, on the device of ``verts``) its gradient operator was built from."""
    V = verts.shape[0]
    if _cloud_on_device(verts, n_neighbors_cloud):
        k = int(n_neighbors_cloud)
        nbr = _cloud_self_knn(verts, k)
        if normals is not None:
            normals = normals.to(device=verts.device, dtype=torch.float32)
        _, frames, _, col, vx, vy = ops.cloud_operators(verts, nbr, normals)
        idx = torch.stack((torch.arange(V, device=verts.device).repeat_interleave(k + 1), col.to(torch.int64)))
        gradX = torch.sparse_coo_tensor(idx, vx, (V, V)).coalesce()
        gradY = torch.sparse_coo_tensor(idx, vy, (V, V)).coalesce()
        return frames, gradX, gradY, nbr
    nbr = find_knn(verts, verts, int(n_neighbors_cloud), omit_diagonal=True, method="cpu_kd").indices
    if normals is None:
        v = verts.detach().cpu().numpy()
        normals = torch.from_numpy(neighborhood_normal(v[nbr.cpu().numpy()] - v[:, None, :])).to(device=verts.device, dtype=verts.dtype)
        if torch.any(torch.isnan(normals)):
            raise ValueError("NaN normals :(")
    frames = _frames_of_normals(normals.to(device=verts.device, dtype=verts.dtype))
    grad = _grad_of_table(verts, frames, nbr)
    return (frames, _pre._to_torch_sparse(grad.real, verts.device, verts.dtype), _pre._to_torch_sparse(grad.imag, verts.device, verts.dtype), nbr)


def _laplacian_of_table(verts, nbr, frames):
    """(L coalesced sparse COO [V,V], mass [V]) of the local-Delaunay construction on a neighbour table and frames, on the device and in
    the dtype of ``verts``: ``ops.cloud_laplacian`` where ``cloud_operators`` runs its kernels, otherwise the numpy route in fp64."""
    V = verts.shape[0]
    if _cloud_on_device(verts, nbr.shape[1]):
        _, rowptr, col, val, mass = ops.cloud_laplacian(verts, nbr, frames.to(device=verts.device, dtype=torch.float32))
        counts = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(V, device=verts.device), counts, output_size=col.numel())
        return torch.sparse_coo_tensor(torch.stack((rows, col.to(torch.int64))), val, (V, V)).coalesce(), mass
    L, mass = _pre.point_cloud_laplacian_from_table(verts.detach().cpu().numpy(), nbr.detach().cpu().numpy(), frames.detach().cpu().numpy())
    return _pre._to_torch_sparse(L, verts.device, verts.dtype), torch.from_numpy(mass).to(device=verts.device, dtype=verts.dtype)


def point_cloud_laplacian(verts, n_neighbors=30, frames=None):
    """Laplacian and lumped mass of a point cloud: ``(L, massvec)``, L a coalesced sparse COO [V,V], both on the device and in the dtype
    of ``verts``.  The local-Delaunay construction of Sharp & Crane (2020, section 5.7) as ``precompute.point_cloud_laplacian_host``
    states it -- NOT robust_laplacian's, which re-triangulates the same triangles intrinsically (tufted cover): here single weights can be
    negative on bad samplings, while L is symmetric, has zero row sums and is positive semi-definite regardless.  ``frames`` [V,3,3]: use
    these tangent frames instead of those of the estimated normals.

    fp32 points on a ROCm device with ``n_neighbors <= 32`` run ``ops.knn``, ``ops.cloud_operators`` (skipped when ``frames`` is given)
    and ``ops.cloud_laplacian`` (dn_knn.hip, dn_cloud.hip, dn_cloud_lap.hip) and never touch the host; everything else takes
    ``precompute.point_cloud_laplacian_host`` (vectorised numpy in fp64)."""
    if _cloud_on_device(verts, n_neighbors):
        nbr = _cloud_self_knn(verts, n_neighbors)
        if frames is None:
            frames = ops.cloud_operators(verts, nbr)[1]
        return _laplacian_of_table(verts, nbr, frames)
    L, mass = _pre.point_cloud_laplacian_host(verts.detach().cpu().numpy(), n_neighbors, frames)
    return _pre._to_torch_sparse(L, verts.device, verts.dtype), torch.from_numpy(mass).to(device=verts.device, dtype=verts.dtype)


# ----------------------------------------------------------------------------------------------
# triangle meshes: cotan Laplacian, mass, frames, gradient operator (geometry.py:114-177, 209-273, 306-335) on the device (dn_mesh.hip)
# ----------------------------------------------------------------------------------------------
def _mesh_on_device(verts):
    """fp32 positions on a ROCm device: ``ops.mesh_assemble`` + ``ops.mesh_frames_gradients``.  (Host tensors take this route only while
    the test suite has bound the emulator build of the library, which runs the same kernels on host buffers.)"""
    return (verts.is_cuda or ops._hip._allow_host_tensors) and verts.dtype == torch.float32


def _mesh_operators_fp64(verts, faces, normals=None):
    """The device route of ``mesh_operators`` in fp64, before any cast: (rowptr [V + 1] int32, col [nnz] int32, lval [nnz], mass [V],
    frames [V, 3, 3], gx [nnz], gy [nnz]) on the device of ``verts``; L, gradX and gradY share the pattern."""
    dev = verts.device
    faces = faces.to(device=dev, dtype=torch.int64)
    rowptr, col, lval, mass, nsum = ops.mesh_assemble(verts, faces)
    if normals is not None:
        n64 = normals.to(device=dev, dtype=torch.float64)
    else:
        n64 = nsum / torch.linalg.vector_norm(nsum, dim=1, keepdim=True)
        if not bool(torch.isfinite(n64).all()):
            # an unreferenced vertex, opposing faces: the reference's jitter-and-fixed-direction rule re-estimates the neighbours too, so
            # the normals of the whole mesh come from the host function that states it
            import numpy as np
            n = _pre.vertex_normals(verts.detach().cpu().numpy().astype(np.float64), faces.detach().cpu().numpy())
            n64 = torch.from_numpy(np.ascontiguousarray(n)).to(dev)
    frames, gx, gy = ops.mesh_frames_gradients(verts, rowptr, col, n64.contiguous())
    if bool(torch.isnan(frames).any()):
        raise ValueError("NaN coordinate frame! Must be very degenerate")
    return rowptr, col, lval, mass, frames, gx, gy


def _csr_rows(rowptr, n_entries):
    counts = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    return torch.repeat_interleave(torch.arange(counts.numel(), device=rowptr.device), counts, output_size=n_entries)


def mesh_operators(verts, faces, normals=None):
    """Frames, lumped mass, cotan Laplacian and gradient operator of a triangle mesh: ``(frames [V,3,3], massvec [V], L, gradX, gradY)``,
    L / gradX / gradY coalesced sparse COO [V,V], all on the device and in the dtype of ``verts`` -- what ``compute_operators`` assembles
    in front of the eigenproblem (``massvec`` is the raw mass, without its EPS x mean).  ``normals`` [V,3]: use these (cast to fp64)
    instead of the normalised sums of the unit face normals.

    fp32 positions on a ROCm device run ``ops.mesh_assemble`` and ``ops.mesh_frames_gradients`` (dn_mesh.hip): fp64 inside, rounded
    once; gradX and gradY stand on L's own pattern (explicit zeros included).  If a vertex has no finite normal (unreferenced, opposing
    faces) the normals of the whole mesh are taken from ``precompute.vertex_normals`` on the host, which states the reference's rule for
    them.  Everything else (host tensors, fp64) takes the host functions of ``precompute`` in fp64.  NaN frames: ``ValueError``."""
    V = verts.shape[0]
    if _mesh_on_device(verts):
        rowptr, col, lval, mass, frames, gx, gy = _mesh_operators_fp64(verts, faces, normals)
        idx = torch.stack((_csr_rows(rowptr, col.numel()), col.to(torch.int64)))
        sparse = lambda v: torch.sparse_coo_tensor(idx, v.to(verts.dtype), (V, V), is_coalesced=True)
        return frames.to(verts.dtype), mass.to(verts.dtype), sparse(lval), sparse(gx), sparse(gy)
    import numpy as np
    v = verts.detach().cpu().numpy().astype(np.float64)
    f = faces.detach().cpu().numpy().astype(np.int64)
    n = _pre.vertex_normals(v, f) if normals is None else normals.detach().cpu().numpy().astype(np.float64)
    frames = _pre.tangent_frames(n)
    L = _pre.cotan_laplacian(v, f, denom_eps=1e-10)
    Lc = L.tocoo()
    grad = _pre.gradient_operator(v, frames, np.stack([Lc.row, Lc.col]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=verts.device, dtype=verts.dtype)
    sp = lambda m: _pre._to_torch_sparse(m, verts.device, verts.dtype)
    return t(frames), t(_pre.vertex_areas(v, f)), sp(L), sp(grad.real), sp(grad.imag)


# ----------------------------------------------------------------------------------------------
# Laplacian eigenbasis: Chebyshev-filtered subspace iteration, the products with S on the device (dn_eigen.hip)
# ----------------------------------------------------------------------------------------------
class _TorchBlocks:
    """The block operations of ``precompute.subspace_iterate`` on fp64 torch blocks [V, nb]: every product with S is ``ops.cheb_step``, the
    tall dense products are torch calls on the same device; only nb x nb matrices and k residual norms cross to the host."""
    route = "kernel"

    def __init__(self, S, dev):
        import numpy as np
        self.dev = dev
        self.rowptr = torch.from_numpy(S.indptr.astype(np.int32)).to(dev)
        self.col = torch.from_numpy(S.indices.astype(np.int32)).to(dev)
        self.val = torch.from_numpy(S.data.astype(np.float64)).to(dev)

    def from_host(self, a):
        import numpy as np
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.dev)

    def to_host(self, a):
        return a.cpu().numpy()

    def step(self, Y, Z, alpha, beta, gamma, out=None):
        return ops.cheb_step(self.rowptr, self.col, self.val, Y, Z, alpha, beta, gamma, out=out)

    def tmm(self, A, B):
        return A.t() @ B

    def mm(self, A, B):
        return A @ B

    def solve_upper_right(self, X, R):          # X R^-1
        return torch.linalg.solve_triangular(R, X, upper=True, left=False).contiguous()

    def residuals(self, SX, X, w, k):
        return torch.linalg.vector_norm(SX[:, :k] - X[:, :k] * w[:k], dim=0)

    def finish(self, X, d, k):
        evecs = X[:, :k] * d[:, None]
        mag = evecs.abs()
        first = (mag == mag.max(dim=0, keepdim=True).values).to(torch.int8).argmax(dim=0)      # the first index of the largest magnitude
        sign = 1.0 - 2.0 * (evecs.gather(0, first[None, :]) < 0).to(evecs.dtype)
        return evecs * sign


def _eigen_on_device():
    return torch.cuda.is_available() or ops._hip._allow_host_tensors


def _scipy_of(L):
    import scipy.sparse
    if isinstance(L, torch.Tensor):
        if L.layout != torch.sparse_coo:
            L = L.to_sparse() if L.layout == torch.strided else L.to_sparse_coo()
        return _pre._sparse_to_csc(L).tocsr()
    return scipy.sparse.csr_matrix(L)


def laplacian_eigenbasis(L, massvec, k_eig, *, rtol=1e-9, seed=0, max_iter=100, dtype=None, return_info=False):
    """The ``k_eig`` smallest pairs of (L + EPS I) phi = lambda M phi, M = diag(massvec) -- the pencil of ``compute_operators`` -- by
    Chebyshev-filtered subspace iteration (``precompute.subspace_iterate``), without a sparse factorisation: (evals [k] ascending, clipped at
    0; evecs [V, k] M-orthonormal, each column signed so that its entry of largest magnitude, the first on ties, is positive) as torch
    tensors on the device of ``massvec`` in ``dtype`` (default: ``massvec``'s).  All arithmetic is fp64.  ``L``: a torch sparse tensor or a
    scipy matrix [V, V], symmetric positive semi-definite; ``massvec`` [V] positive (torch, or array-like: the host).

    With a ROCm device every product with S = D (L + EPS I) D, D = diag(massvec^-1/2), is ``ops.cheb_step`` (dn_eigen.hip) and the tall
    dense products are fp64 torch calls on that device; the nb x nb ``eigh`` and Cholesky factorisations, nb = k + max(16, ceil(k / 4)),
    run on the host (a few small transfers and synchronisations per outer iteration, of which there are 3 .. 9).  Without a device: the
    same driver on numpy / scipy (``precompute.laplacian_eigenbasis_subspace``).  2 nb > V: ``scipy.linalg.eigh`` of the dense pencil on the
    host, in either case.  The starting block is drawn on the host from ``numpy.random.default_rng(seed)``: both routes start alike.
    ``return_info``: also a dict -- ``route`` ("kernel", "numpy", "dense" or "empty"), ``nb``, ``ub`` (the Gershgorin bound of S),
    ``iterations``, ``products`` (with S), ``degrees`` (of the filters) and ``residual`` (max_i ||S x_i - w_i x_i||_2 at the end).
    ``RuntimeError`` if a Cholesky factorisation fails or ``max_iter`` iterations do not reach ``rtol``: there is no fallback."""
    import numpy as np
    if not isinstance(massvec, torch.Tensor):
        massvec = torch.as_tensor(np.asarray(massvec))
    out_dev = massvec.device
    out_dtype = dtype if dtype is not None else (massvec.dtype if massvec.dtype.is_floating_point else torch.float64)
    m = massvec.detach().cpu().numpy().astype(np.float64).reshape(-1)
    Ls = _scipy_of(L)
    V, k = Ls.shape[0], int(k_eig)
    if Ls.shape != (V, V) or m.shape != (V,):
        raise ValueError("laplacian_eigenbasis: L %s and massvec %s do not fit" % (Ls.shape, m.shape))
    if k < 0:
        raise ValueError("laplacian_eigenbasis: k_eig = %d" % k)
    if k == 0 or 2 * _pre.subspace_block_width(k) > V or not _eigen_on_device():
        evals, evecs, info = _pre.laplacian_eigenbasis_subspace(Ls, m, k, rtol=rtol, seed=seed, max_iter=max_iter, return_info=True)
        evals, evecs = torch.from_numpy(np.ascontiguousarray(evals)), torch.from_numpy(np.ascontiguousarray(evecs))
    else:
        # (host buffers only while the test suite has bound the emulator build of the library, which cannot read device memory)
        if ops._hip._allow_host_tensors:
            dev = torch.device("cpu")
        else:
            dev = out_dev if out_dev.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        S, d, ub = _pre.scaled_operator(Ls, m)
        evals, evecs, info = _pre.subspace_iterate(_TorchBlocks(S, dev), V, d, ub, k, rtol, seed, max_iter)
        evals = torch.from_numpy(np.ascontiguousarray(evals))
    evals, evecs = evals.to(device=out_dev, dtype=out_dtype), evecs.to(device=out_dev, dtype=out_dtype)
    return (evals, evecs, info) if return_info else (evals, evecs)


# ----------------------------------------------------------------------------------------------
# geodesic evaluation metric (geometry.py:754-896): all-pairs distances on the Steiner-point graph of the mesh
# ----------------------------------------------------------------------------------------------
def _as_numpy(x):
    """torch tensor (any device) or array-like -> numpy array on the host."""
    import numpy as np
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _steiner_graph(verts, faces, n_steiner):
    """``mesh_distance_graph`` and the [n_nodes, 3] fp64 positions of its nodes."""
    import numpy as np
    import scipy.sparse
    x = np.asarray(_as_numpy(verts), dtype=np.float64).reshape(-1, 3)
    f = np.asarray(_as_numpy(faces)).astype(np.int64).reshape(-1, 3)
    V, m = x.shape[0], int(n_steiner)
    if m < 0:
        raise ValueError("n_steiner must be >= 0")
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("mesh_distance_graph: a face index is outside [0, %d)" % V)
    # half-edge i of a face runs f[i] -> f[i + 1] and faces the vertex f[i + 2]
    ha, hb, opp = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    key = np.minimum(ha, hb) * V + np.maximum(ha, hb)
    ukey, edge_of = np.unique(key, return_inverse=True)
    ea, eb = ukey // V, ukey % V
    E = ukey.shape[0]
    t = (np.arange(1, m + 1, dtype=np.float64) / (m + 1))[None, :, None]
    pos = np.concatenate([x, ((1.0 - t) * x[ea][:, None, :] + t * x[eb][:, None, :]).reshape(-1, 3)])
    steiner = V + np.arange(E, dtype=np.int64)[:, None] * m + np.arange(m, dtype=np.int64)[None, :]          # [E, m]
    chain = np.concatenate([ea[:, None], steiner, eb[:, None]], axis=1)                                    # (i)
    tails, tips = [chain[:, :-1].reshape(-1)], [chain[:, 1:].reshape(-1)]
    if m:
        fs = steiner[edge_of].reshape(-1, 3, m)                                                            # the Steiner nodes of a face's edges
        for p, q in ((0, 1), (1, 2), (0, 2)):                                                              # (ii)
            tails.append(np.repeat(fs[:, p, :], m, axis=1).reshape(-1))
            tips.append(np.tile(fs[:, q, :], (1, m)).reshape(-1))
        tails.append(steiner[edge_of].reshape(-1))                                                         # (iii)
        tips.append(np.repeat(opp, m))
    tail, tip = np.concatenate(tails), np.concatenate(tips)
    n = pos.shape[0]
    lo, hi = np.minimum(tail, tip), np.maximum(tail, tip)
    pair = np.unique(lo[lo != hi] * n + hi[lo != hi])                                                      # each arc once
    lo, hi = pair // n, pair % n
    w = np.sqrt(((pos[lo] - pos[hi]) ** 2).sum(axis=1))
    g = scipy.sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n)).tocsr()
    g.sort_indices()
    return g, pos


def mesh_distance_graph(verts, faces, n_steiner=3):
    """The Steiner-point graph of a triangle mesh (Lanthier, Maheshwari, Sack) as a symmetric scipy CSR matrix of fp64 arc lengths.

    Nodes 0 .. V-1 are the vertices (positions cast to fp64).  Every undirected edge (a, b), a < b, that occurs in a face carries
    ``m = n_steiner`` further nodes at (1 - t) x_a + t x_b, t = j / (m + 1), j = 1 .. m; edge e (edges sorted by (a, b)) owns nodes
    V + e m .. V + e m + m - 1.  Arcs, each once, weighted by the Euclidean distance of the two node positions: (i) consecutive nodes
    along every edge, a, s_1, .., s_m, b; (ii) in every face, every Steiner node with every Steiner node of the face's other two edges;
    (iii) in every face, every Steiner node with the vertex opposite its edge.  Every arc is a straight segment inside a face, so a path of
    the graph is a path on the surface: graph distances are never below the geodesic, exact along edges, and can only fall as m grows.
    ``n_steiner = 0`` is the edge graph.  Boundary and non-manifold edges, duplicate vertices (zero-length arcs) and unreferenced
    vertices (empty rows) are legal.  Vectorised numpy: no Python loop over faces or edges."""
    return _steiner_graph(verts, faces, n_steiner)[0]


def _geodesic_on_device():
    return torch.cuda.is_available() or ops._hip._allow_host_tensors


_GEODESIC_BLOCK_BYTES = 1 << 30


def geodesic_distances(verts, faces, sources=None, n_steiner=3):
    """Distances on the surface from the vertices ``sources`` (None: all) to every vertex: [len(sources), V] fp64 numpy, torch or numpy in.
    Shortest paths on ``mesh_distance_graph(verts, faces, n_steiner)``: an upper bound of the geodesic distance, exact along edges.
    With a ROCm device the (min, +) sweeps of ``ops.minplus_distances`` (dn_geodesic.hip), otherwise ``scipy.sparse.csgraph.dijkstra`` on
    the same graph; both return, for every pair, the minimum over paths of the left-to-right fp64 sum of the arc lengths -- the same bits."""
    import numpy as np
    g = mesh_distance_graph(verts, faces, n_steiner)
    V = np.asarray(_as_numpy(verts)).reshape(-1, 3).shape[0]
    src = np.arange(V, dtype=np.int64) if sources is None else np.asarray(_as_numpy(sources)).astype(np.int64).reshape(-1)
    if src.size and (src.min() < 0 or src.max() >= V):
        raise ValueError("geodesic_distances: a source is outside [0, %d)" % V)
    out = np.empty((src.shape[0], V), dtype=np.float64)
    if src.size == 0 or V == 0:
        return out
    if not _geodesic_on_device():
        import scipy.sparse.csgraph
        out[:] = scipy.sparse.csgraph.dijkstra(g, directed=True, indices=src)[:, :V]
        return out
    # (host buffers only while the test suite has bound the emulator build of the library, which cannot read device memory)
    dev = torch.device("cpu") if ops._hip._allow_host_tensors else torch.device("cuda", torch.cuda.current_device())
    gd, new_of = _band_ordered(g)
    rowptr = torch.from_numpy(gd.indptr.astype(np.int32)).to(dev)
    col = torch.from_numpy(gd.indices.astype(np.int32)).to(dev)
    w = torch.from_numpy(gd.data.astype(np.float64)).to(dev)
    keep = torch.from_numpy(new_of[:V]).to(dev)
    n = g.shape[0]
    per_call = max(1, _GEODESIC_BLOCK_BYTES // (8 * n))          # only the V vertex columns of a block are kept: bounded device memory
    for s0 in range(0, src.shape[0], per_call):
        d = ops.minplus_distances(rowptr, col, w, torch.from_numpy(new_of[src[s0:s0 + per_call]]), max_block_bytes=_GEODESIC_BLOCK_BYTES)
        out[s0:s0 + d.shape[0]] = d[:, keep].cpu().numpy()
    return out


def _band_ordered(g):
    """``g`` with its nodes renumbered in reverse Cuthill-McKee order, and ``new_of`` [n] int64 (new number of every old node).  The
    kernel's workgroups own runs of consecutive nodes, so neighbours numbered close to each other are rows that are still in cache; a
    distance is a minimum over paths and does not depend on how the nodes are numbered, so the result is the same bits."""
    import numpy as np
    import scipy.sparse
    import scipy.sparse.csgraph
    n = g.shape[0]
    old_of = scipy.sparse.csgraph.reverse_cuthill_mckee(g, symmetric_mode=True).astype(np.int64)
    new_of = np.empty(n, dtype=np.int64)
    new_of[old_of] = np.arange(n, dtype=np.int64)
    coo = g.tocoo()
    gd = scipy.sparse.coo_matrix((coo.data, (new_of[coo.row], new_of[coo.col])), shape=(n, n)).tocsr()   # (explicit zeros stay arcs)
    gd.sort_indices()
    return gd, new_of


def _geodesic_cache_lookup(cache_dir, stem, verts_np, faces_np):
    """The reference's bucket search (geometry.py:824-850) over ``<stem>_<i>.npz``: (matrix or None, the path of the first free bucket)."""
    import os
    import numpy as np
    i = 0
    while True:
        path = os.path.join(cache_dir, "%s_%d.npz" % (stem, i))
        try:
            npz = np.load(path, allow_pickle=True)
        except FileNotFoundError:
            return None, path
        if np.array_equal(verts_np, npz["verts"]) and np.array_equal(faces_np, npz["faces"]):
            return npz["dist"], path
        i += 1


def _symmetrised(dists):
    """geometry.py:871-879: non-finite -> NaN, fmin with the transpose, what is still NaN -> the largest finite value."""
    import numpy as np
    dists = np.nan_to_num(dists, nan=np.nan, posinf=np.nan, neginf=np.nan)
    dists = np.fmin(dists, np.transpose(dists))
    max_dist = np.nanmax(dists)
    return np.nan_to_num(dists, nan=max_dist, posinf=max_dist, neginf=max_dist)


def get_all_pairs_geodesic_distance(verts_np, faces_np, geodesic_cache_dir=None, *, method="steiner", n_steiner=3):
    """The dense V x V matrix of surface distances (geometry.py:804-896; numpy in, numpy out), cached as the reference caches it.

    ``method='steiner'`` (default): ``geodesic_distances`` on the Steiner-point graph with ``n_steiner`` nodes per edge -- an upper bound
    of the geodesic, where the reference is exact.  ``method='exact'``: ``igl.exact_geodesic`` per source, as the reference does (needs
    libigl).  Either way the matrix is made exactly symmetric as in the reference.

    Cache: a file in the reference's own format and name, ``<hash>_<i>.npz`` (keys verts, faces, dist), was written by libigl, is exact,
    and is returned as it is whatever ``method`` says.  Only ``method='exact'`` writes under that name; the Steiner route reads and writes
    ``<hash>_steiner<m>_<i>.npz`` (the same keys plus method and n_steiner)."""
    import numpy as np
    from . import utils
    if method not in ("steiner", "exact"):
        raise ValueError("unrecognized method")
    m = int(n_steiner)
    exact_path = own_path = None
    if geodesic_cache_dir is not None:
        utils.ensure_dir_exists(geodesic_cache_dir)
        key = str(utils.hash_arrays((verts_np, faces_np)))
        found, exact_path = _geodesic_cache_lookup(geodesic_cache_dir, key, verts_np, faces_np)
        if found is not None:
            return found
        if method == "steiner":
            found, own_path = _geodesic_cache_lookup(geodesic_cache_dir, "%s_steiner%d" % (key, m), verts_np, faces_np)
            if found is not None:
                return found
    if method == "exact":
        try:
            import igl
        except ImportError:
            raise ImportError("method='exact' needs python libigl (`conda install -c conda-forge igl`); "
                              "method='steiner' computes an upper bound of the geodesic distances without it")
        print("Computing all-pairs geodesic distance (method=exact, igl.exact_geodesic per source; warning: SLOW!)")
        N = verts_np.shape[0]
        targets = np.arange(N)[:, np.newaxis]
        dists = np.array([igl.exact_geodesic(verts_np, faces_np, np.array([i])[:, np.newaxis], targets) for i in range(N)])
        dists = _symmetrised(dists.reshape(N, N))
        if exact_path is not None:
            np.savez(exact_path, verts=verts_np, faces=faces_np, dist=dists)
        return dists
    print("Computing all-pairs geodesic distance (method=steiner, n_steiner=%d)" % m)
    dists = _symmetrised(geodesic_distances(verts_np, faces_np, None, m))
    if own_path is not None:
        np.savez(own_path, verts=verts_np, faces=faces_np, dist=dists, method="steiner", n_steiner=m)
    return dists


def geodesic_label_errors(target_verts, target_faces, pred_labels, gt_labels, normalization='diameter', geodesic_cache_dir=None):
    """Distances on the target surface between predicted and ground-truth labels (geometry.py:754-781), divided by the largest distance of
    the surface (``'diameter'``: a numpy array) or by the square root of its area (``'area'``: an fp64 torch tensor, as in the reference).
    The distances are ``get_all_pairs_geodesic_distance``'s: exact where the cache holds a matrix libigl wrote, otherwise the Steiner-graph
    upper bound."""
    import numpy as np
    if normalization not in ("diameter", "area"):
        raise ValueError("unrecognized normalization")
    target_verts, target_faces = _as_numpy(target_verts), _as_numpy(target_faces)
    pred_labels, gt_labels = _as_numpy(pred_labels), _as_numpy(gt_labels)
    dists = get_all_pairs_geodesic_distance(target_verts, target_faces, geodesic_cache_dir)
    result_dists = dists[pred_labels, gt_labels]
    if normalization == "diameter":
        return result_dists / np.max(dists)
    v, f = torch.tensor(target_verts), torch.tensor(target_faces).long()
    coords = v[f]
    total_area = torch.sum(0.5 * torch.linalg.cross(coords[:, 1] - coords[:, 0], coords[:, 2] - coords[:, 0], dim=-1).norm(dim=-1))
    return torch.as_tensor(result_dists) / torch.sqrt(total_area)

"""torch.autograd bindings of the HIP hot ops (C ABI in include/diffnet_hip.h).

Each Function enqueues the library's kernels on the current torch stream; forward saves the
activations the hand-written backward needs.  No op has a torch/CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import weakref
from typing import List, NamedTuple, Optional

import torch

from . import _hip
from .batch import GatherPattern, MeshBatch, register_handle


def _on_device(fn):
    """Run a Function's forward/backward (or a custom operator of torchlib.py) with the tensors' device current: the library reads the current device for its
    per-device function attributes and CU counts, and a launch on another device's stream is an error -- `model.to('cuda:1')`
    without a surrounding `torch.cuda.device` must just work, as it does for torch's own ops."""
    @functools.wraps(fn)
    def wrapped(*args):
        dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if dev is None or torch.cuda.current_device() == dev.index:
            return fn(*args)
        with torch.cuda.device(dev):
            return fn(*args)
    return wrapped


def _require(t: torch.Tensor, mb=None):
    """Tensors on a ROCm device, and on the SAME device as the packed operators they are used with (an operator cache hit or a
    caller-built MeshBatch from another GPU would otherwise be dereferenced on the wrong device)."""
    _hip.require_device(t)
    if mb is not None and mb.device is not None and torch.device(mb.device) != t.device:
        raise RuntimeError("MeshBatch lives on %s but the features are on %s" % (mb.device, t.device))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError("diffusion_net HIP ops are fp32 (got %s)" % t.dtype)
    return t.contiguous()


def _ws(mb: MeshBatch, nbytes: int):
    buf = _hip.workspace(mb.device, max(int(nbytes), 1024))
    return buf, buf.numel()


# ----------------------------------------------------------------------------------------------
# basis transforms (geometry.py:572-598)
# ----------------------------------------------------------------------------------------------
def _to_basis_raw(mb, x, use_mass):
    L = _hip.lib()
    Cc = x.shape[1]
    spec = torch.empty(mb.n_mesh, mb.k_eig, Cc, dtype=torch.float32, device=x.device)
    ws, n = _ws(mb, L.dn_to_basis_workspace_bytes(mb.ref(), Cc))
    _hip.check(L.dn_to_basis_f32(mb.ref(), x.data_ptr(), Cc, int(use_mass), spec.data_ptr(), ws.data_ptr(), n,
                                 _hip.stream_of(x)), "dn_to_basis_f32")
    return spec


def _from_basis_raw(mb, spec, scale_by_mass=False):
    L = _hip.lib()
    Cc = spec.shape[-1]
    out = torch.empty(mb.v_total, Cc, dtype=torch.float32, device=spec.device)
    _hip.check(L.dn_from_basis_f32(mb.ref(), spec.data_ptr(), Cc, int(scale_by_mass), out.data_ptr(),
                                   _hip.stream_of(spec)), "dn_from_basis_f32")
    return out


class ToBasisFn(torch.autograd.Function):
    """spec[m] = evecs_m^T (x_m * mass_m)  -> [n_mesh, K, C]"""

    @staticmethod
    @_on_device
    def forward(ctx, x, mb):
        _require(x, mb)
        ctx.mb = mb
        return _to_basis_raw(mb, _f32c(x), True)

    @staticmethod
    @_on_device
    def backward(ctx, d_spec):
        return _from_basis_raw(ctx.mb, _f32c(d_spec), scale_by_mass=True), None


class FromBasisFn(torch.autograd.Function):
    """x_m = evecs_m spec[m]  -> [v_total, C]"""

    @staticmethod
    @_on_device
    def forward(ctx, spec, mb):
        _require(spec, mb)
        ctx.mb = mb
        return _from_basis_raw(mb, _f32c(spec))

    @staticmethod
    @_on_device
    def backward(ctx, d_x):
        return _to_basis_raw(ctx.mb, _f32c(d_x), False), None


# ----------------------------------------------------------------------------------------------
# learned-time spectral diffusion (layers.py:44-67)
# ----------------------------------------------------------------------------------------------
class DiffusionFn(torch.autograd.Function):
    @staticmethod
    @_on_device
    def forward(ctx, x, time, mb):
        _require(x, mb)
        L = _hip.lib()
        x, time = _f32c(x), _f32c(time)
        Cc = x.shape[1]
        xs = torch.empty(mb.n_mesh, mb.k_eig, Cc, dtype=torch.float32, device=x.device)
        xd = torch.empty_like(x)
        ws, n = _ws(mb, L.dn_diffusion_workspace_bytes(mb.ref(), Cc))
        _hip.check(L.dn_diffusion_fwd_f32(mb.ref(), x.data_ptr(), time.data_ptr(), Cc, xs.data_ptr(), xd.data_ptr(),
                                          ws.data_ptr(), n, _hip.stream_of(x)), "dn_diffusion_fwd_f32")
        ctx.mb = mb
        ctx.save_for_backward(xs, time)
        return xd

    @staticmethod
    @_on_device
    def backward(ctx, d_xd):
        L = _hip.lib()
        mb = ctx.mb
        xs, time = ctx.saved_tensors
        d_xd = _f32c(d_xd)
        Cc = d_xd.shape[1]
        d_x = torch.empty_like(d_xd)
        d_t = torch.empty_like(time)
        ws, n = _ws(mb, L.dn_diffusion_workspace_bytes(mb.ref(), Cc))
        _hip.check(L.dn_diffusion_bwd_f32(mb.ref(), d_xd.data_ptr(), xs.data_ptr(), time.data_ptr(), Cc, None,
                                          d_x.data_ptr(), d_t.data_ptr(), ws.data_ptr(), n, _hip.stream_of(d_xd)),
                   "dn_diffusion_bwd_f32")
        return d_x, d_t, None


# ----------------------------------------------------------------------------------------------
# spatial gradients + gradient features (layers.py:217-223, 117-130)
# ----------------------------------------------------------------------------------------------
class GradApplyFn(torch.autograd.Function):
    @staticmethod
    @_on_device
    def forward(ctx, x, mb):
        _require(x, mb)
        x = _f32c(x)
        gx, gy = torch.empty_like(x), torch.empty_like(x)
        _hip.check(_hip.lib().dn_grad_apply_fwd_f32(mb.ref(), x.data_ptr(), x.shape[1], gx.data_ptr(), gy.data_ptr(),
                                                    _hip.stream_of(x)), "dn_grad_apply_fwd_f32")
        ctx.mb = mb
        return gx, gy

    @staticmethod
    @_on_device
    def backward(ctx, d_gx, d_gy):
        d_gx, d_gy = _f32c(d_gx), _f32c(d_gy)
        d_x = torch.empty_like(d_gx)
        _hip.check(_hip.lib().dn_grad_apply_bwd_f32(ctx.mb.ref(), d_gx.data_ptr(), d_gy.data_ptr(), None, d_gx.shape[1],
                                                    d_x.data_ptr(), _hip.stream_of(d_gx)), "dn_grad_apply_bwd_f32")
        return d_x, None


class GradFeatFn(torch.autograd.Function):
    @staticmethod
    @_on_device
    def forward(ctx, gx, gy, A_re, A_im, mb):
        _require(gx, mb)
        gx, gy, A_re = _f32c(gx), _f32c(gy), _f32c(A_re)
        A_im = _f32c(A_im) if A_im is not None else None
        g, bre, bim = torch.empty_like(gx), torch.empty_like(gx), torch.empty_like(gx)
        _hip.check(_hip.lib().dn_gradfeat_fwd_f32(mb.ref(), gx.data_ptr(), gy.data_ptr(), A_re.data_ptr(), _hip.ptr(A_im),
                                                  gx.shape[1], g.data_ptr(), bre.data_ptr(), bim.data_ptr(),
                                                  _hip.stream_of(gx)), "dn_gradfeat_fwd_f32")
        ctx.mb = mb
        ctx.has_im = A_im is not None
        ctx.save_for_backward(gx, gy, g, bre, bim, A_re, A_im if A_im is not None else A_re)
        return g

    @staticmethod
    @_on_device
    def backward(ctx, d_g):
        L = _hip.lib()
        mb = ctx.mb
        gx, gy, g, bre, bim, A_re, A_im = ctx.saved_tensors
        d_g = _f32c(d_g)
        Cc = gx.shape[1]
        d_gx, d_gy = torch.empty_like(gx), torch.empty_like(gx)
        dA_re = torch.empty_like(A_re)
        dA_im = torch.empty_like(A_re) if ctx.has_im else None
        ws, n = _ws(mb, L.dn_gradfeat_workspace_bytes(mb.ref(), Cc))
        _hip.check(L.dn_gradfeat_bwd_f32(mb.ref(), d_g.data_ptr(), g.data_ptr(), gx.data_ptr(), gy.data_ptr(), bre.data_ptr(),
                                         bim.data_ptr(), A_re.data_ptr(), A_im.data_ptr() if ctx.has_im else None, Cc,
                                         d_gx.data_ptr(), d_gy.data_ptr(), dA_re.data_ptr(), _hip.ptr(dA_im),
                                         ws.data_ptr(), n, _hip.stream_of(d_g)), "dn_gradfeat_bwd_f32")
        return d_gx, d_gy, dA_re, dA_im, None


# ----------------------------------------------------------------------------------------------
# nn.Linear on the row axis (first_lin / last_lin / stand-alone MiniMLP layers)
# ----------------------------------------------------------------------------------------------
def hks(evals, evecs, scales):
    """out[.., v, s] = sum_k exp(-evals[.., k] * scales[.., s]) * evecs[.., v, k]^2 (geometry.py:600-628), forward only."""
    _hip.require_device(evecs)
    squeeze = evals.dim() == 1
    if squeeze:
        evals, evecs, scales = evals[None], evecs[None], scales[None]
    evals, evecs, scales = _f32c(evals), _f32c(evecs), _f32c(scales)
    B, V, K = evecs.shape
    S = scales.shape[-1]
    out = torch.empty(B, V, S, dtype=torch.float32, device=evecs.device)
    per_batch = int(scales.dim() == 2 and scales.shape[0] == B and B > 1)
    _hip.check(_hip.lib().dn_hks_f32(evals.data_ptr(), evecs.data_ptr(), scales.data_ptr(), B, V, K, S, per_batch, out.data_ptr(),
                                     _hip.stream_of(evecs)), "dn_hks_f32")
    return out[0] if squeeze else out


@_on_device
def _knn_launch(src, tgt, k, largest, omit_diagonal, n_split):
    L = _hip.lib()
    N, D = src.shape
    M = tgt.shape[0]
    dist = torch.empty(N, k, dtype=torch.float32, device=src.device)
    idx = torch.empty(N, k, dtype=torch.int64, device=src.device)
    nbytes = L.dn_knn_workspace_bytes(N, M, D, k, n_split)
    ws = _hip.workspace(src.device, nbytes) if nbytes else None
    _hip.check(L.dn_knn_f32(src.data_ptr(), N, tgt.data_ptr(), M, D, k, int(largest), int(omit_diagonal), n_split, dist.data_ptr(),
                            idx.data_ptr(), _hip.ptr(ws), ws.numel() if ws is not None else 0, _hip.stream_of(src)), "dn_knn_f32")
    return dist, idx


def knn(src, tgt, k, largest=False, omit_diagonal=False, n_split=0):
    """Exact k nearest (``largest``: farthest) rows of ``tgt`` [M, D] for every row of ``src`` [N, D] -> (dist [N, k] fp32, idx [N, k] int64),
    sorted by distance, equal distances by the lower target index (geometry.py:667-724), forward only.  ``omit_diagonal``: target i is no
    candidate of row i.  ``n_split``: how many target slices are searched in parallel (0: the library chooses); the result does not depend on it."""
    _hip.require_device(src)
    _hip.require_device(tgt)
    src, tgt = _f32c(src), _f32c(tgt)
    if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != tgt.shape[1] or src.shape[1] < 1:
        raise ValueError("knn takes [N, D] and [M, D] points (got %s and %s)" % (tuple(src.shape), tuple(tgt.shape)))
    if src.device != tgt.device:
        raise RuntimeError("knn: source points on %s, target points on %s" % (src.device, tgt.device))
    k, n_split = int(k), int(n_split)
    if omit_diagonal and src.shape[0] != tgt.shape[0]:
        raise ValueError("omit_diagonal can only be used when source and target are same shape")
    if not 1 <= k <= _hip.KNN_MAX_K:
        raise ValueError("knn kernel takes 1 <= k <= %d (got %d)" % (_hip.KNN_MAX_K, k))
    if k > tgt.shape[0] - int(bool(omit_diagonal)):
        raise ValueError("k = %d neighbours asked of %d candidates" % (k, tgt.shape[0] - int(bool(omit_diagonal))))
    if n_split < 0:
        raise ValueError("n_split must be >= 0")
    return _knn_launch(src, tgt, k, bool(largest), bool(omit_diagonal), n_split)


@_on_device
def _knn_grid_launch(src, tgt, k, omit_diagonal, cells_per_axis, cell_budget, want_info):
    """Every device step of ``knn_grid`` without a host read: bounds (torch), cell keys, stable sort of the keys and cell start table
    (torch, as ``cloud_laplacian`` sorts its keys), gather + search."""
    L = _hip.lib()
    N, D = src.shape
    M = tgt.shape[0]
    dev = src.device
    st = _hip.stream_of(src)
    dist = torch.empty(N, k, dtype=torch.float32, device=dev)
    idx = torch.empty(N, k, dtype=torch.int64, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev) if want_info else None
    if N == 0:
        return dist, idx, info
    G = L.dn_knn_grid_cells(M, k, D, cells_per_axis)
    shared = src.data_ptr() == tgt.data_ptr() and N == M         # a self-query: the sources' cells are the targets'
    box = torch.cat((tgt.amin(dim=0), tgt.amax(dim=0)))
    tkey = torch.empty(M, dtype=torch.int32, device=dev)
    skey = None if shared else torch.empty(N, dtype=torch.int32, device=dev)
    _hip.check(L.dn_knn_grid_keys_f32(src.data_ptr(), N, tgt.data_ptr(), M, D, k, cells_per_axis, box.data_ptr(), _hip.ptr(skey),
                                      tkey.data_ptr(), st), "dn_knn_grid_keys_f32")
    tsorted, torder = torch.sort(tkey, stable=True)
    sorder = torder if shared else torch.sort(skey, stable=True)[1]
    cells = torch.arange(G ** D + 1, dtype=torch.int32, device=dev)
    cell_start = torch.searchsorted(tsorted, cells, out_int32=True)
    ws = _hip.workspace(dev, L.dn_knn_grid_workspace_bytes(N, M, D, k, cells_per_axis))
    _hip.check(L.dn_knn_grid_search_f32(src.data_ptr(), N, tgt.data_ptr(), M, D, k, int(omit_diagonal), cells_per_axis, cell_budget,
                                        box.data_ptr(), sorder.data_ptr(), torder.data_ptr(), cell_start.data_ptr(), dist.data_ptr(),
                                        idx.data_ptr(), _hip.ptr(info), ws.data_ptr(), ws.numel(), st), "dn_knn_grid_search_f32")
    return dist, idx, info


def knn_grid(src, tgt, k, omit_diagonal=False, cells_per_axis=0, return_info=False, cell_budget=None):
    """``knn`` for D <= 3 by a search over a dense grid of cells (include/diffnet_hip.h: dn_knn_grid_search_f32): the same bits as
    ``ops.knn(src, tgt, k, omit_diagonal=omit_diagonal)`` with work that grows with N k, forward only, no ``largest``.
    ``cells_per_axis``: cells per axis of the grid (0: the library chooses from M, k and D); ``cell_budget``: cells a query may visit before
    it scans all targets instead (None: the library's value; 0: every query scans) -- the result depends on neither.
    ``return_info``: also return ``{'max_shell', 'full_scans', 'cells_per_axis'}`` of the call (reading it waits for the kernels; nothing
    else in the call reads the host)."""
    _hip.require_device(src)
    _hip.require_device(tgt)
    src, tgt = _f32c(src), _f32c(tgt)
    if src.dim() != 2 or tgt.dim() != 2 or src.shape[1] != tgt.shape[1] or src.shape[1] < 1:
        raise ValueError("knn takes [N, D] and [M, D] points (got %s and %s)" % (tuple(src.shape), tuple(tgt.shape)))
    if src.shape[1] > 3:
        raise ValueError("knn_grid takes points of at most 3 dimensions (got %d)" % src.shape[1])
    if src.device != tgt.device:
        raise RuntimeError("knn: source points on %s, target points on %s" % (src.device, tgt.device))
    k, cells_per_axis = int(k), int(cells_per_axis)
    if omit_diagonal and src.shape[0] != tgt.shape[0]:
        raise ValueError("omit_diagonal can only be used when source and target are same shape")
    if not 1 <= k <= _hip.KNN_MAX_K:
        raise ValueError("knn kernel takes 1 <= k <= %d (got %d)" % (_hip.KNN_MAX_K, k))
    if k > tgt.shape[0] - int(bool(omit_diagonal)):
        raise ValueError("k = %d neighbours asked of %d candidates" % (k, tgt.shape[0] - int(bool(omit_diagonal))))
    if cells_per_axis < 0:
        raise ValueError("cells_per_axis must be >= 0")
    budget = -1 if cell_budget is None else int(cell_budget)
    if budget < -1:
        raise ValueError("cell_budget must be >= 0")
    dist, idx, info = _knn_grid_launch(src, tgt, k, bool(omit_diagonal), cells_per_axis, budget, bool(return_info))
    if not return_info:
        return dist, idx
    shell, scans = info.tolist()
    G = _hip.lib().dn_knn_grid_cells(tgt.shape[0], k, src.shape[1], cells_per_axis)
    return dist, idx, {"max_shell": shell, "full_scans": scans, "cells_per_axis": G}


@_on_device
def _fps_launch(points, offsets, n_clouds, min_points, max_points, n_sample, start, route, return_min_dist):
    L = _hip.lib()
    dev = points.device
    order = torch.empty(n_clouds, n_sample, dtype=torch.int64, device=dev)
    radii = torch.empty(n_clouds, n_sample, dtype=torch.float32, device=dev)
    md = torch.empty(points.shape[0], dtype=torch.float32, device=dev) if return_min_dist else None
    nbytes = L.dn_fps_workspace_bytes(points.shape[0], n_clouds, max_points, n_sample, route)
    ws = _hip.workspace(dev, nbytes) if nbytes else None
    _hip.check(L.dn_fps_f32(points.data_ptr(), offsets.data_ptr(), n_clouds, min_points, max_points, n_sample, _hip.ptr(start), route,
                            order.data_ptr(), radii.data_ptr(), _hip.ptr(md), _hip.ptr(ws), ws.numel() if ws is not None else 0,
                            _hip.stream_of(points)), "dn_fps_f32")
    return order, radii, md


_fps_offset_cache = {}


def _fps_offsets(sizes, device):
    """The device copy of a batch's offsets.  One cloud: made by device kernels alone, so a call can be captured in a graph without a
    warm-up; a batch: copied from the host once per (sizes, device) and kept (a capture after a warm-up call finds it here)."""
    if len(sizes) == 1:
        return torch.arange(2, dtype=torch.int64, device=device) * sizes[0]
    key = (sizes, str(device))
    offs = _fps_offset_cache.get(key)
    if offs is None:
        acc = [0]
        for n in sizes:
            acc.append(acc[-1] + n)
        if len(_fps_offset_cache) >= 64:
            _fps_offset_cache.clear()
        offs = _fps_offset_cache[key] = torch.tensor(acc, dtype=torch.int64).to(device)
    return offs


def fps(points, n_sample, offsets=None, start=None, route=0, return_min_dist=False):
    """Farthest point sampling of ``points`` [V, 3] fp32, ALREADY normalised (geometry.py:727-751), forward only -> (order [n_clouds,
    n_sample] int64, radii [n_clouds, n_sample] fp32) and, with ``return_min_dist``, min_dist2 [V] fp32.  ``offsets`` (a list of Python ints
    or an int64 HOST tensor, n_clouds + 1 entries, 0 first and V last; None: one cloud) packs several clouds back to back; ``order`` holds
    rows of the packed array in the order chosen, ``radii`` the squared distance of each sample to the earlier ones when it was chosen (+inf
    first).  ``start`` [n_clouds] int64 on the points' device names the first samples (None: the point nearest the origin).  ``route``: 0 the
    library's choice, 1 the one-launch resident kernel (clouds up to ``_hip.FPS_RESIDENT_MAX_POINTS``), 2 one launch per sample; the
    result does not depend on it.  Equal distances go to the lowest index."""
    _hip.require_device(points)
    points = _f32c(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("fps takes [V, 3] points (got %s)" % (tuple(points.shape),))
    n_sample, route = int(n_sample), int(route)
    if route not in (0, 1, 2):
        raise ValueError("fps route must be 0 (library's choice), 1 (resident) or 2 (stepped)")
    V = points.shape[0]
    if offsets is None:
        sizes_list = [V]
    else:
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
            raise ValueError("fps takes its offsets as host values (the cloud sizes select the kernel)")
        off_list = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        if len(off_list) < 1 or off_list[0] != 0 or off_list[-1] != V or any(b < a for a, b in zip(off_list, off_list[1:])):
            raise ValueError("fps offsets must rise from 0 to the number of points")
        sizes_list = [b - a for a, b in zip(off_list, off_list[1:])]
    n_clouds = len(sizes_list)
    if n_sample < 1:
        raise ValueError("fps takes n_sample >= 1 (got %d)" % n_sample)
    if n_clouds == 0:
        empty = (torch.empty(0, n_sample, dtype=torch.int64, device=points.device), torch.empty(0, n_sample, dtype=torch.float32, device=points.device))
        return empty + (torch.empty(0, dtype=torch.float32, device=points.device),) if return_min_dist else empty
    min_points, max_points = min(sizes_list), max(sizes_list)
    if n_sample > min_points:
        raise ValueError("not enough points to sample")
    if route == 1 and max_points > _hip.FPS_RESIDENT_MAX_POINTS:
        raise ValueError("fps resident route takes clouds of at most %d points (got %d)" % (_hip.FPS_RESIDENT_MAX_POINTS, max_points))
    offs = _fps_offsets(tuple(sizes_list), points.device)
    if start is not None:
        _hip.require_device(start)
        if start.dtype != torch.int64 or tuple(start.shape) != (n_clouds,) or start.device != points.device:
            raise ValueError("fps start must be [n_clouds] int64 on the points' device")
        start = start.contiguous()
    order, radii, md = _fps_launch(points, offs, n_clouds, min_points, max_points, n_sample, start, route, bool(return_min_dist))
    return (order, radii, md) if return_min_dist else (order, radii)


@_on_device
def _cloud_launch(points, nbr, normals_in):
    n, k = nbr.shape
    dev = points.device
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
    frames = torch.empty(n, 3, 3, dtype=torch.float32, device=dev)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(n * (k + 1), dtype=torch.int32, device=dev)
    vx = torch.empty(n * (k + 1), dtype=torch.float32, device=dev)
    vy = torch.empty(n * (k + 1), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        rowptr.zero_()
    _hip.check(_hip.lib().dn_cloud_operators_f32(points.data_ptr(), n, nbr.data_ptr(), k, _hip.ptr(normals_in), normals.data_ptr(),
                                                 frames.data_ptr(), rowptr.data_ptr(), col.data_ptr(), vx.data_ptr(), vy.data_ptr(),
                                                 status.data_ptr(), _hip.stream_of(points)), "dn_cloud_operators_f32")
    return normals, frames, rowptr, col, vx, vy, status


def cloud_operators(points, nbr, normals=None):
    """Normal, tangent frame and gradient stencil of every point of a cloud from the indices of its neighbours (geometry.py:92-99, 114-123,
    151-273 for a cloud; include/diffnet_hip.h: dn_cloud_operators_f32), forward only.  ``points`` [N, 3] fp32, ``nbr`` [N, k] int64 as
    ``ops.knn(points, points, k, omit_diagonal=True)`` returns them, ``normals`` [N, 3] fp32 or None (estimated).
    -> (normals [N, 3], frames [N, 3, 3], rowptr [N + 1] int32, col [N (k + 1)] int32, vx, vy [N (k + 1)] fp32): row i of the gradient
    operator has k + 1 entries, column i first, then the neighbours in ``nbr`` order.  Raises ``IndexError`` if a row of ``nbr`` holds an
    index outside [0, N) (reading the status word waits for the kernel)."""
    _hip.require_device(points)
    _hip.require_device(nbr)
    points = _f32c(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("cloud_operators takes [N, 3] points (got %s)" % (tuple(points.shape),))
    if nbr.dim() != 2 or nbr.shape[0] != points.shape[0]:
        raise ValueError("cloud_operators takes [N, k] neighbour indices for [N, 3] points (got %s for %s)" % (tuple(nbr.shape), tuple(points.shape)))
    if nbr.dtype != torch.int64:
        raise TypeError("cloud_operators takes int64 neighbour indices (got %s)" % nbr.dtype)
    if nbr.device != points.device:
        raise RuntimeError("cloud_operators: points on %s, neighbour indices on %s" % (points.device, nbr.device))
    n, k = nbr.shape
    if not 1 <= k <= _hip.KNN_MAX_K:
        raise ValueError("cloud_operators kernel takes 1 <= k <= %d neighbours (got %d)" % (_hip.KNN_MAX_K, k))
    if n * (k + 1) > 2 ** 31 - 1:
        raise ValueError("cloud_operators: %d x %d row entries do not fit a 32-bit row pointer" % (n, k + 1))
    if normals is not None:
        _hip.require_device(normals)
        normals = _f32c(normals)
        if tuple(normals.shape) != (n, 3):
            raise ValueError("cloud_operators takes [N, 3] normals (got %s)" % (tuple(normals.shape),))
        if normals.device != points.device:
            raise RuntimeError("cloud_operators: points on %s, normals on %s" % (points.device, normals.device))
    *out, status = _cloud_launch(points, nbr.contiguous(), normals)
    bad = int(status.item())
    if bad:
        raise IndexError("cloud_operators: %d row(s) of the neighbour table hold an index outside [0, %d)" % (bad, n))
    return tuple(out)


@_on_device
def _cloud_laplacian_launch(points, nbr, frames):
    """Every device step of ``cloud_laplacian`` without a host read: star, emit, stable sort of the keys (torch), segment sums.
    -> (partner [N, k] int32, rowptr [N + 1] int32, col, val [9 N k] (the first ``count`` entries are the matrix), mass [N] fp32,
    count [1] int32, status [1] int32)."""
    L = _hip.lib()
    n, k = nbr.shape
    dev = points.device
    slots = n * k
    m = 9 * slots
    st = _hip.stream_of(points)
    partner = torch.empty(n, k, dtype=torch.int32, device=dev)
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    val = torch.empty(max(m, 1), dtype=torch.float32, device=dev)
    mass = torch.zeros(n, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if n == 0:
        return partner, rowptr, col[:0], val[:0], mass, count, status
    _hip.check(L.dn_cloud_star_f32(points.data_ptr(), n, nbr.data_ptr(), k, frames.data_ptr(), partner.data_ptr(), status.data_ptr(), st),
               "dn_cloud_star_f32")
    nbytes = L.dn_cloud_laplacian_workspace_bytes(n, k)
    ws = _hip.workspace(dev, nbytes)
    _hip.check(L.dn_cloud_laplacian_emit_f32(points.data_ptr(), n, nbr.data_ptr(), k, partner.data_ptr(), ws.data_ptr(), ws.numel(), st),
               "dn_cloud_laplacian_emit_f32")
    # the workspace layout of include/diffnet_hip.h
    key_l, val_l = ws[:72 * slots].view(torch.int64), ws[72 * slots:144 * slots].view(torch.float64)
    key_m, val_m = ws[144 * slots:168 * slots].view(torch.int64), ws[168 * slots:192 * slots].view(torch.float64)
    skey, perm = torch.sort(key_l, stable=True)
    head = torch.ones(m, dtype=torch.bool, device=dev)
    torch.ne(skey[1:], skey[:-1], out=head[1:])
    rank = torch.cumsum(head, 0, dtype=torch.int64)
    _hip.check(L.dn_segment_sum_f64_f32(skey.data_ptr(), perm.data_ptr(), val_l.data_ptr(), m, rank.data_ptr(), n, rowptr.data_ptr(),
                                        col.data_ptr(), val.data_ptr(), count.data_ptr(), st), "dn_segment_sum_f64_f32")
    skey_m, perm_m = torch.sort(key_m, stable=True)
    _hip.check(L.dn_segment_sum_f64_f32(skey_m.data_ptr(), perm_m.data_ptr(), val_m.data_ptr(), 3 * slots, None, n, None, None,
                                        mass.data_ptr(), None, st), "dn_segment_sum_f64_f32")
    return partner, rowptr, col, val, mass, count, status


def cloud_laplacian(points, nbr, frames):
    """Laplacian and lumped mass of a point cloud from the local Delaunay star of every point among its projected neighbours (Sharp &
    Crane 2020, section 5.7, without the intrinsic / tufted re-triangulation; include/diffnet_hip.h: dn_cloud_star_f32), forward only.
    ``points`` [N, 3] fp32, ``nbr`` [N, k] int64 as ``ops.knn(points, points, k, omit_diagonal=True)`` returns them, ``frames`` [N, 3, 3]
    fp32 as ``ops.cloud_operators`` returns them (rows basisX, basisY are read).
    -> (partner [N, k] int32, rowptr [N + 1] int32, col [nnz] int32, val [nnz] fp32, mass [N] fp32): ``partner[i, a]`` is the slot b of the
    triangle (i, nbr[i, a], nbr[i, b]) of the star of i, or -1; L is CSR with ascending columns, symmetric bit for bit, and repeats bit for
    bit from call to call.  Raises ``IndexError`` if a row of ``nbr`` holds an index outside [0, N) (reading the status word and the
    number of entries waits for the kernels)."""
    _hip.require_device(points)
    _hip.require_device(nbr)
    _hip.require_device(frames)
    points, frames = _f32c(points), _f32c(frames)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("cloud_laplacian takes [N, 3] points (got %s)" % (tuple(points.shape),))
    if nbr.dim() != 2 or nbr.shape[0] != points.shape[0]:
        raise ValueError("cloud_laplacian takes [N, k] neighbour indices for [N, 3] points (got %s for %s)" % (tuple(nbr.shape), tuple(points.shape)))
    if nbr.dtype != torch.int64:
        raise TypeError("cloud_laplacian takes int64 neighbour indices (got %s)" % nbr.dtype)
    n, k = nbr.shape
    if tuple(frames.shape) != (n, 3, 3):
        raise ValueError("cloud_laplacian takes [N, 3, 3] frames (got %s)" % (tuple(frames.shape),))
    if nbr.device != points.device or frames.device != points.device:
        raise RuntimeError("cloud_laplacian: points on %s, neighbour indices on %s, frames on %s" % (points.device, nbr.device, frames.device))
    if not 1 <= k <= _hip.KNN_MAX_K:
        raise ValueError("cloud_laplacian kernel takes 1 <= k <= %d neighbours (got %d)" % (_hip.KNN_MAX_K, k))
    if 9 * n * k > 2 ** 31 - 1:
        raise ValueError("cloud_laplacian: 9 x %d x %d matrix terms do not fit a 32-bit count" % (n, k))
    partner, rowptr, col, val, mass, count, status = _cloud_laplacian_launch(points, nbr.contiguous(), frames)
    bad, nnz = torch.cat((status, count)).tolist()
    if bad:
        raise IndexError("cloud_laplacian: %d row(s) of the neighbour table hold an index outside [0, %d)" % (bad, n))
    return partner, rowptr, col[:nnz].clone(), val[:nnz].clone(), mass


# ----------------------------------------------------------------------------------------------
# triangle-mesh operators: cotan Laplacian, mass, normal sums, frames, gradients (include/diffnet_hip.h: dn_mesh_emit_f32)
# ----------------------------------------------------------------------------------------------
@_on_device
def _mesh_assemble_launch(verts, faces):
    """Every device step of ``mesh_assemble`` without a host read: emit, stable sort of the keys (torch), segment sums.
    -> (rowptr [V + 1] int32, col, lval [9 F] (the first ``count`` entries are the matrix; fp64), vrec [V, 4] fp64 (mass, normal sum),
    count [1] int32, status [1] int32)."""
    L = _hip.lib()
    V, F = verts.shape[0], faces.shape[0]
    dev = verts.device
    m = 9 * F
    st = _hip.stream_of(verts)
    rowptr = torch.zeros(V + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    lval = torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    vrec = torch.zeros(V, 4, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if F == 0:
        return rowptr, col[:0], lval[:0], vrec, count, status
    ws = _hip.workspace(dev, L.dn_mesh_workspace_bytes(V, F))
    _hip.check(L.dn_mesh_emit_f32(verts.data_ptr(), V, faces.data_ptr(), F, ws.data_ptr(), ws.numel(), status.data_ptr(), st), "dn_mesh_emit_f32")
    # the workspace layout of include/diffnet_hip.h
    Fe = (F + 1) // 2 * 2
    key_l, val_l = ws[:72 * F].view(torch.int64), ws[72 * Fe:72 * Fe + 72 * F].view(torch.float64)
    key_v, val_v = ws[144 * Fe:144 * Fe + 24 * F].view(torch.int64), ws[168 * Fe:168 * Fe + 96 * F].view(torch.float64)
    skey, perm = torch.sort(key_l, stable=True)
    head = torch.ones(m, dtype=torch.bool, device=dev)
    torch.ne(skey[1:], skey[:-1], out=head[1:])
    rank = torch.cumsum(head, 0, dtype=torch.int64)
    _hip.check(L.dn_segment_sum_f64_f64(skey.data_ptr(), perm.data_ptr(), val_l.data_ptr(), m, rank.data_ptr(), V, rowptr.data_ptr(),
                                        col.data_ptr(), lval.data_ptr(), count.data_ptr(), st), "dn_segment_sum_f64_f64")
    if V:                                     # (no vertex: every face is out of range and the status word says so)
        skey_v, perm_v = torch.sort(key_v, stable=True)
        _hip.check(L.dn_segment_sum4_f64_f64(skey_v.data_ptr(), perm_v.data_ptr(), val_v.data_ptr(), 3 * F, V, vrec.data_ptr(), st),
                   "dn_segment_sum4_f64_f64")
    return rowptr, col, lval, vrec, count, status


def _mesh_check_verts(verts, what):
    _hip.require_device(verts)
    verts = _f32c(verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("%s takes [V, 3] vertex positions (got %s)" % (what, tuple(verts.shape)))
    if verts.shape[0] > 2 ** 31 - 1:
        raise ValueError("%s: %d vertices do not fit a 32-bit index" % (what, verts.shape[0]))
    return verts


def mesh_assemble(verts, faces):
    """Cotan Laplacian, lumped mass and vertex normal sums of a triangle mesh (geometry.py:114-148, 306-335; include/diffnet_hip.h:
    dn_mesh_emit_f32), forward only.  ``verts`` [V, 3] fp32, ``faces`` [F, 3] int64.
    -> (rowptr [V + 1] int32, col [nnz] int32, lval [nnz] fp64, mass [V] fp64, normal_sum [V, 3] fp64): L is CSR with ascending columns,
    per corner w = 0.5 (a.b) / (|a x b| + 1e-10) (explicit zeros stay entries), symmetric bit for bit; the mass is a third of the area of
    the incident faces, ``normal_sum`` the sum of their n / (|n| + 1e-6).  fp64 from the coordinate differences on, no floating-point
    atomics: the result repeats bit for bit from call to call.  Raises ``IndexError`` if a face holds an index outside [0, V) (reading
    the status word and the number of entries waits for the kernels)."""
    verts = _mesh_check_verts(verts, "mesh_assemble")
    _hip.require_device(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("mesh_assemble takes [F, 3] faces (got %s)" % (tuple(faces.shape),))
    if faces.dtype != torch.int64:
        raise TypeError("mesh_assemble takes int64 faces (got %s)" % faces.dtype)
    if faces.device != verts.device:
        raise RuntimeError("mesh_assemble: vertices on %s, faces on %s" % (verts.device, faces.device))
    V, F = verts.shape[0], faces.shape[0]
    if 9 * F > 2 ** 31 - 1:
        raise ValueError("mesh_assemble: 9 x %d matrix terms do not fit a 32-bit count" % F)
    rowptr, col, lval, vrec, count, status = _mesh_assemble_launch(verts, faces.contiguous())
    bad, nnz = torch.cat((status, count)).tolist()
    if bad:
        raise IndexError("mesh_assemble: %d face(s) hold an index outside [0, %d)" % (bad, V))
    return rowptr, col[:nnz].clone(), lval[:nnz].clone(), vrec[:, 0].contiguous(), vrec[:, 1:].contiguous()


@_on_device
def _mesh_frames_gradients_launch(verts, rowptr, col, normals):
    """The vertex pass without a host read -> (frames [V, 3, 3], gx [nnz], gy [nnz] fp64, status [1] int32)."""
    V, nnz = verts.shape[0], col.numel()
    dev = verts.device
    frames = torch.empty(V, 3, 3, dtype=torch.float64, device=dev)
    gx = torch.zeros(nnz, dtype=torch.float64, device=dev)
    gy = torch.zeros(nnz, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if V == 0:
        return frames, gx, gy, status
    _hip.check(_hip.lib().dn_mesh_frames_gradients_f64(verts.data_ptr(), V, rowptr.data_ptr(), _hip.ptr(col) if nnz else None, nnz,
                                                       normals.data_ptr(), frames.data_ptr(), _hip.ptr(gx) if nnz else None,
                                                       _hip.ptr(gy) if nnz else None, status.data_ptr(), _hip.stream_of(verts)),
               "dn_mesh_frames_gradients_f64")
    return frames, gx, gy, status


def _mesh_check_pattern(verts, rowptr, col, normals, what="mesh_frames_gradients"):
    verts = _mesh_check_verts(verts, what)
    for t in (rowptr, col, normals):
        _hip.require_device(t)
    V = verts.shape[0]
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32:
        raise TypeError("%s takes int32 rowptr and col (got %s, %s)" % (what, rowptr.dtype, col.dtype))
    if normals.dtype != torch.float64:
        raise TypeError("%s takes fp64 normals (got %s)" % (what, normals.dtype))
    if rowptr.dim() != 1 or rowptr.numel() != V + 1 or col.dim() != 1:
        raise ValueError("%s takes CSR arrays rowptr [V + 1], col [nnz] for [V, 3] positions (got %s, %s for %s)"
                         % (what, tuple(rowptr.shape), tuple(col.shape), tuple(verts.shape)))
    if tuple(normals.shape) != (V, 3):
        raise ValueError("%s takes [V, 3] normals (got %s)" % (what, tuple(normals.shape)))
    if not (rowptr.device == col.device == normals.device == verts.device):
        raise RuntimeError("%s: vertices on %s, rowptr on %s, col on %s, normals on %s" % (what, verts.device, rowptr.device, col.device, normals.device))
    if col.numel() > 2 ** 31 - 1:
        raise ValueError("%s: %d entries do not fit a 32-bit row pointer" % (what, col.numel()))
    return verts, rowptr.contiguous(), col.contiguous(), normals.contiguous()


def mesh_frames_gradients(verts, rowptr, col, normals):
    """Tangent frames of given normals and the least-squares gradient operator on a CSR pattern -- L's own, as ``mesh_assemble`` returns
    it (geometry.py:151-177, 209-273; include/diffnet_hip.h: dn_mesh_frames_gradients_f64), forward only.  ``verts`` [V, 3] fp32,
    ``rowptr`` [V + 1] and ``col`` [nnz] int32, ``normals`` [V, 3] fp64.
    -> (frames [V, 3, 3] fp64, gx [nnz] fp64, gy [nnz] fp64): row i of gx + i gy is the stencil of vertex i over the off-diagonal entries
    of its row, its own coefficient in the diagonal entry.  Raises ``IndexError`` if a row pointer or a column is out of range or a
    non-empty row has no diagonal entry (reading the status word waits for the kernel)."""
    verts, rowptr, col, normals = _mesh_check_pattern(verts, rowptr, col, normals)
    frames, gx, gy, status = _mesh_frames_gradients_launch(verts, rowptr, col, normals)
    bad = int(status.item())
    if bad:
        raise IndexError("mesh_frames_gradients: %d row(s) of the pattern are out of range or lack their diagonal entry" % bad)
    return frames, gx, gy


# ----------------------------------------------------------------------------------------------
# all-pairs graph distances: (min, +) relaxation sweeps (include/diffnet_hip.h: dn_minplus_sweeps_f64)
# ----------------------------------------------------------------------------------------------
@_on_device
def _minplus_block(rowptr, col, w, src, n_nodes, sweeps_per_check):
    """Distances [n_nodes, len(src)] (node-major) from the nodes ``src`` (int64, on the graph's device): swept in groups of
    ``sweeps_per_check`` until a group's last sweep lowers nothing."""
    L = _hip.lib()
    dev = w.device
    S = src.numel()
    dist = torch.full((n_nodes, S), float("inf"), dtype=torch.float64, device=dev)
    dist[src, torch.arange(S, device=dev)] = 0.0
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    done = 0
    while True:
        n = min(sweeps_per_check, n_nodes - done)
        if n <= 0:
            raise RuntimeError("minplus_distances: no fixed point after %d sweeps of %d nodes" % (done, n_nodes))
        _hip.check(L.dn_minplus_sweeps_f64(rowptr.data_ptr(), col.data_ptr(), w.data_ptr(), n_nodes, dist.data_ptr(), S, n, changed.data_ptr(),
                                           _hip.stream_of(w)), "dn_minplus_sweeps_f64")
        done += n
        if not int(changed.item()):          # the one host read per group of sweeps
            return dist


def minplus_distances(rowptr, col, w, sources, *, sweeps_per_check=8, max_block_bytes=1 << 30):
    """Shortest-path distances on a graph by (min, +) relaxation sweeps (dn_geodesic.hip), forward only.  ``rowptr`` [n_nodes + 1] and
    ``col`` [nnz] int32: CSR arcs; ``w`` [nnz] fp64 arc lengths, non-negative; ``sources`` int64 node indices (duplicates allowed).
    -> [len(sources), n_nodes] fp64 on the graph's device, ``inf`` where no path exists: for every pair the minimum over paths of the
    left-to-right fp64 sum of the arc lengths -- the bits ``scipy.sparse.csgraph.dijkstra`` returns.

    The sources are cut into blocks whose node-major distance block fits ``max_block_bytes``; a block is swept ``sweeps_per_check`` sweeps
    at a time and the device's changed word read after each group (this op synchronises with the host by design: it is evaluation code).
    ``ValueError`` before any launch for a negative or NaN length and for a column or source outside [0, n_nodes); ``RuntimeError`` if
    n_nodes sweeps reach no fixed point (impossible with non-negative lengths)."""
    for t in (rowptr, col, w):
        _hip.require_device(t)
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32:
        raise TypeError("minplus_distances takes int32 rowptr and col (got %s, %s)" % (rowptr.dtype, col.dtype))
    if w.dtype != torch.float64:
        raise TypeError("minplus_distances takes fp64 arc lengths (got %s)" % w.dtype)
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or w.dim() != 1 or col.numel() != w.numel():
        raise ValueError("minplus_distances takes CSR arrays rowptr [n + 1], col [nnz], w [nnz]")
    if not (rowptr.device == col.device == w.device):
        raise RuntimeError("minplus_distances: the CSR arrays are on %s, %s and %s" % (rowptr.device, col.device, w.device))
    dev = w.device
    rowptr, col, w = rowptr.contiguous(), col.contiguous(), w.contiguous()
    n_nodes, nnz = rowptr.numel() - 1, col.numel()
    sources = torch.as_tensor(sources, dtype=torch.int64).reshape(-1).to(dev)
    sweeps_per_check, max_block_bytes = int(sweeps_per_check), int(max_block_bytes)
    if sweeps_per_check < 1:
        raise ValueError("sweeps_per_check must be >= 1")
    rp = rowptr.to(torch.int64)
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_nodes and bool((rp[1:] < rp[:-1]).any())):
        raise ValueError("minplus_distances: rowptr is not a non-decreasing row pointer of %d entries" % nnz)
    if nnz:
        if bool(torch.isnan(w).any()) or bool((w < 0).any()):
            raise ValueError("minplus_distances takes non-negative arc lengths (negative or NaN found)")
        if int(col.min()) < 0 or int(col.max()) >= n_nodes:
            raise ValueError("minplus_distances: a column index is outside [0, %d)" % n_nodes)
    if sources.numel() and (int(sources.min()) < 0 or int(sources.max()) >= n_nodes):
        raise ValueError("minplus_distances: a source is outside [0, %d)" % n_nodes)
    S = sources.numel()
    out = torch.empty(S, n_nodes, dtype=torch.float64, device=dev)
    if S == 0 or n_nodes == 0:
        return out
    per_block = max(1, min(S, max_block_bytes // (8 * n_nodes), 65535 * 64))
    for s0 in range(0, S, per_block):
        src = sources[s0:s0 + per_block]
        out[s0:s0 + src.numel()] = _minplus_block(rowptr, col, w, src, n_nodes, sweeps_per_check).t()
    return out


# ----------------------------------------------------------------------------------------------
# Laplacian eigenbasis: one Chebyshev recurrence step on a block of vectors (include/diffnet_hip.h: dn_cheb_step_f64)
# ----------------------------------------------------------------------------------------------
_cheb_checked = None      # (weakref rowptr, weakref col, their versions): the CSR pattern the last call validated


def _cheb_check_pattern(rowptr, col, n_rows):
    """Row pointer and column range of a CSR pattern, read back from the device ONCE per pattern: the calls of a solve share one."""
    global _cheb_checked
    seen = _cheb_checked
    if seen is not None and seen[0]() is rowptr and seen[1]() is col and seen[2] == (rowptr._version, col._version, n_rows):
        return
    nnz = col.numel()
    rp = rowptr.to(torch.int64)
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_rows and bool((rp[1:] < rp[:-1]).any())):
        raise ValueError("cheb_step: rowptr is not a non-decreasing row pointer of %d entries" % nnz)
    if nnz and (int(col.min()) < 0 or int(col.max()) >= n_rows):
        raise ValueError("cheb_step: a column index is outside [0, %d)" % n_rows)
    _cheb_checked = (weakref.ref(rowptr), weakref.ref(col), (rowptr._version, col._version, n_rows))


def _cheb_block(name, t, n_rows, like):
    if (t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != n_rows or (t.shape[1] > 1 and t.stride(1) != 1)
            or (n_rows > 1 and t.stride(0) < t.shape[1])):
        raise TypeError("cheb_step: %s must be an fp64 block [%d, nb] with unit column stride (got %s %s, strides %s)"
                        % (name, n_rows, t.dtype, tuple(t.shape), t.stride()))
    if like is not None and (t.shape != like.shape or _cheb_ld(t) != _cheb_ld(like) or t.device != like.device):
        raise ValueError("cheb_step: %s %s (leading dimension %d, %s) does not match Y %s (%d, %s)"
                         % (name, tuple(t.shape), _cheb_ld(t), t.device, tuple(like.shape), _cheb_ld(like), like.device))


def _cheb_ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


@_on_device
def _cheb_launch(rowptr, col, val, Y, Z, out, alpha, beta, gamma):
    _hip.check(_hip.lib().dn_cheb_step_f64(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), Y.shape[0], Y.data_ptr(), _hip.ptr(Z),
                                           out.data_ptr(), Y.shape[1], _cheb_ld(Y), alpha, beta, gamma, _hip.stream_of(Y)), "dn_cheb_step_f64")
    return out


def cheb_step(rowptr, col, val, Y, Z, alpha, beta, gamma, out=None):
    """``out = alpha * S @ Y + beta * Y + gamma * Z`` for S in CSR (dn_eigen.hip), forward only: one step of the Chebyshev three-term
    recurrence on a block of vectors.  ``rowptr`` [n + 1], ``col`` [nnz] int32, ``val`` [nnz] fp64; ``Y``, ``Z``, ``out`` fp64 blocks
    [n, nb] with unit column stride and ONE row stride (the leading dimension, >= nb: column slices of wider blocks are taken as they
    are, what lies beside them is neither read nor written).  ``Z`` may be None when ``gamma == 0``; a term whose scalar is 0 is not formed.
    ``out`` None: a new contiguous block; ``out`` may be ``Z``, never ``Y``.  One fma per entry in CSR order, no atomics: two calls give the
    same bits.  No synchronisation, except that the pattern (rowptr, col) is validated on its first use (``ValueError``)."""
    for t in (rowptr, col, val, Y):
        _hip.require_device(t)
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or val.dtype != torch.float64:
        raise TypeError("cheb_step takes int32 rowptr and col and fp64 values (got %s, %s, %s)" % (rowptr.dtype, col.dtype, val.dtype))
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.dim() != 1 or col.numel() != val.numel():
        raise ValueError("cheb_step takes CSR arrays rowptr [n + 1], col [nnz], val [nnz]")
    if not (rowptr.is_contiguous() and col.is_contiguous() and val.is_contiguous()):
        raise ValueError("cheb_step takes contiguous CSR arrays")
    n_rows = rowptr.numel() - 1
    alpha, beta, gamma = float(alpha), float(beta), float(gamma)
    _cheb_block("Y", Y, n_rows, None)
    if not (rowptr.device == col.device == val.device == Y.device):
        raise RuntimeError("cheb_step: the operands are on %s, %s, %s and %s" % (rowptr.device, col.device, val.device, Y.device))
    if Z is None and gamma != 0.0:
        raise ValueError("cheb_step: gamma = %g needs Z" % gamma)
    if Z is not None:
        _hip.require_device(Z)
        _cheb_block("Z", Z, n_rows, Y)
    if out is None:
        if _cheb_ld(Y) == Y.shape[1]:
            out = torch.empty_like(Y)
        else:                                    # Y is a column slice: a block of its leading dimension, sliced alike
            out = torch.empty(n_rows, _cheb_ld(Y), dtype=torch.float64, device=Y.device)[:, :Y.shape[1]]
    else:
        _hip.require_device(out)
        _cheb_block("out", out, n_rows, Y)
        if out.data_ptr() == Y.data_ptr() and out.numel():
            raise ValueError("cheb_step: out must not be Y (other rows of Y are read while out is written)")
    if n_rows == 0 or Y.shape[1] == 0:
        return out
    if col.numel() == 0:
        raise ValueError("cheb_step: S has no entries")
    _cheb_check_pattern(rowptr, col, n_rows)
    return _cheb_launch(rowptr, col, val, Y, Z, out, alpha, beta, gamma)


# ----------------------------------------------------------------------------------------------
# implicit diffusion: (diag(m) + t_c L) x_c = m u_c per mesh and channel by Jacobi-preconditioned conjugate gradients
# (include/diffnet_hip.h: dn_implicit_*_f32; the recurrence in numpy: precompute.implicit_diffusion_host)
# ----------------------------------------------------------------------------------------------
_implicit_tables = {}
_implicit_checked = []        # [(weakref rowptr, weakref col, their versions)]: the CSR patterns validated last, newest first


def _implicit_check_pattern(rowptr, col, n_rows):
    """Row pointer and column range of a CSR pattern, read back from the device ONCE per pattern (as ``_cheb_check_pattern``); the last eight
    patterns are remembered, by the identity and version of their tensors."""
    stamp = (rowptr._version, col._version, n_rows)
    for seen in _implicit_checked:
        if seen[0]() is rowptr and seen[1]() is col and seen[2] == stamp:
            return
    nnz = col.numel()
    rp = rowptr.to(torch.int64)
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_rows and bool((rp[1:] < rp[:-1]).any())):
        raise ValueError("implicit_solve: rowptr is not a non-decreasing row pointer of %d entries" % nnz)
    if nnz and (int(col.min()) < 0 or int(col.max()) >= n_rows):
        raise ValueError("implicit_solve: a column index is outside [0, %d)" % n_rows)
    _implicit_checked.insert(0, (weakref.ref(rowptr), weakref.ref(col), stamp))
    del _implicit_checked[8:]


def _implicit_tables_on(device, sizes):
    """(tiles [n_tiles, 4] int32, mesh_tile_off [n_mesh + 1] int32) on ``device``: runs of at most ``dn_implicit_rows_per_tile()`` rows that
    never straddle two meshes, built from the mesh sizes once per (device, sizes)."""
    import numpy as np
    R = int(_hip.lib().dn_implicit_rows_per_tile())
    key = (str(device), tuple(sizes), R)
    hit = _implicit_tables.get(key)
    if hit is None:
        if len(_implicit_tables) > 256:
            _implicit_tables.clear()
        tiles, off, row0 = [], [0], 0
        for m, v in enumerate(sizes):
            tiles += [(row0 + r, min(R, v - r), m, 0) for r in range(0, v, R)]
            off.append(len(tiles))
            row0 += v
        hit = (torch.from_numpy(np.array(tiles, dtype=np.int32).reshape(-1, 4)).to(device), torch.from_numpy(np.array(off, dtype=np.int32)).to(device))
        _implicit_tables[key] = hit
    return hit


class ImplicitOperator:
    """The operands of the implicit diffusion that do not change from call to call: L in CSR (int32 ``rowptr`` [V + 1] and ``col`` [nnz], fp32
    ``val`` [nnz], block diagonal over the meshes), ``mass`` [V] fp32, the rows of every mesh (``sizes``, default one mesh) and the tile
    tables made from them.  ``validate=False``: the pattern comes from ``batch.coo_to_csr``, which has checked it."""

    def __init__(self, rowptr, col, val, mass, sizes=None, *, validate=True):
        for t in (rowptr, col, val, mass):
            _hip.require_device(t)
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or val.dtype != torch.float32 or mass.dtype != torch.float32:
            raise TypeError("implicit_solve takes int32 rowptr and col and fp32 values and mass (got %s, %s, %s, %s)"
                            % (rowptr.dtype, col.dtype, val.dtype, mass.dtype))
        if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.dim() != 1 or col.numel() != val.numel() or mass.dim() != 1:
            raise ValueError("implicit_solve takes CSR arrays rowptr [V + 1], col [nnz], val [nnz] and mass [V]")
        V = rowptr.numel() - 1
        if mass.numel() != V:
            raise ValueError("implicit_solve: mass has %d entries for %d rows" % (mass.numel(), V))
        if not (rowptr.device == col.device == val.device == mass.device):
            raise RuntimeError("implicit_solve: the operands are on %s, %s, %s and %s" % (rowptr.device, col.device, val.device, mass.device))
        if mass.requires_grad or val.requires_grad:
            raise RuntimeError("implicit_solve has no gradient for mass or L")
        self.sizes = [V] if sizes is None else [int(s) for s in sizes]
        if sum(self.sizes) != V or any(s < 1 for s in self.sizes):
            raise ValueError("implicit_solve: sizes %s are not positive row counts that sum to %d" % (self.sizes if len(self.sizes) < 9 else "[...]", V))
        self.rowptr, self.col, self.val, self.mass = rowptr.contiguous(), col.contiguous(), val.contiguous(), mass.contiguous()
        self.V, self.device = V, mass.device
        if validate and V:
            _implicit_check_pattern(self.rowptr, self.col, V)
        self.tiles, self.mesh_tile_off = _implicit_tables_on(self.device, self.sizes) if V else (None, None)
        self.n_tiles = int(self.tiles.shape[0]) if V else 0

    @property
    def n_mesh(self):
        return len(self.sizes)


def _implicit_block(name, t, op, C=None):
    _hip.require_device(t)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != op.V or (C is not None and t.shape[1] != C):
        raise TypeError("implicit_solve: %s must be an fp32 block [%d, %s] (got %s %s)" % (name, op.V, "C" if C is None else C, t.dtype, tuple(t.shape)))
    if t.device != op.device:
        raise RuntimeError("implicit_solve: %s is on %s, the operator on %s" % (name, t.device, op.device))
    return t.contiguous()


@_on_device
def _implicit_run(rhs, time, x0, lx_x, op, rhs_mass, rtol, max_iter, iters_per_check, check):
    """One solve on a packed operator.  ``rhs_mass``: the right side is m (.) rhs and the result x (forward); else the right side is rhs and
    the result m (.) x (backward: d_u), and with ``lx_x`` (the forward's x) the gradient of the times is returned too.
    -> (out [V, C] fp32, info, d_time [C] fp32 or None)."""
    L, dev = _hip.lib(), op.device
    V, Cc, nm = op.V, rhs.shape[1], op.n_mesh
    out = torch.empty_like(rhs)
    iters = torch.zeros(nm, Cc, dtype=torch.int32, device=dev)
    res = torch.zeros(nm, Cc, dtype=torch.float64, device=dev)
    info = {"iterations": iters, "residual": res, "launches": 0}
    d_time = torch.zeros(Cc, dtype=torch.float32, device=dev) if lx_x is not None else None
    if V == 0 or Cc == 0:
        return out, info, d_time
    ws = _hip.workspace(dev, max(int(L.dn_implicit_workspace_bytes(V, Cc, op.n_tiles, nm)), 1024))
    st = _hip.stream_of(rhs)
    table = (op.tiles.data_ptr(), op.n_tiles, op.mesh_tile_off.data_ptr(), nm, V, Cc)
    csr = (op.rowptr.data_ptr(), _hip.ptr(op.col) if op.col.numel() else None, _hip.ptr(op.val) if op.val.numel() else None)
    if op.col.numel() == 0:                      # L = 0 (every row empty): the library takes non-NULL arrays
        pad = torch.zeros(1, dtype=torch.int32, device=dev)
        csr = (csr[0], pad.data_ptr(), pad.data_ptr())
    _hip.check(L.dn_implicit_init_f32(*csr, op.mass.data_ptr(), time.data_ptr(), *table, rhs.data_ptr(), 1 if rhs_mass else 0, _hip.ptr(x0),
                                      float(rtol), ws.data_ptr(), ws.numel(), st), "dn_implicit_init_f32")
    info["launches"] += 2
    unfinished = torch.empty(1, dtype=torch.int32, device=dev)
    done = 0
    while True:
        n = max(0, min(iters_per_check if check else max_iter, max_iter - done))
        _hip.check(L.dn_implicit_iterate_f32(*csr, op.mass.data_ptr(), time.data_ptr(), *table, n, unfinished.data_ptr(), ws.data_ptr(), ws.numel(),
                                             st), "dn_implicit_iterate_f32")
        done += n
        info["launches"] += 4 * n + 1
        if not check:
            break
        left = int(unfinished.item())            # the one host read per group of iterations
        if left == 0:
            break
        if done >= max_iter:
            raise RuntimeError("implicit_solve: %d iterations did not reach rtol = %g (%d of %d systems left)" % (done, rtol, left, nm * Cc))
    _hip.check(L.dn_implicit_finish_f32(op.mass.data_ptr(), *table, 0 if rhs_mass else 1, out.data_ptr(), iters.data_ptr(), res.data_ptr(),
                                        ws.data_ptr(), ws.numel(), st), "dn_implicit_finish_f32")
    info["launches"] += 1
    if lx_x is not None:
        _hip.check(L.dn_implicit_lx_dot_f32(*csr, *table, lx_x.data_ptr(), d_time.data_ptr(), ws.data_ptr(), ws.numel(), st), "dn_implicit_lx_dot_f32")
        info["launches"] += 2
    return out, info, d_time


def _implicit_settings(rtol, max_iter, iters_per_check):
    rtol, max_iter, iters_per_check = float(rtol), int(max_iter), int(iters_per_check)
    if not rtol >= 0.0:
        raise ValueError("rtol must be >= 0")
    if max_iter < 0 or iters_per_check < 1:
        raise ValueError("max_iter must be >= 0 and iters_per_check >= 1")
    return rtol, max_iter, iters_per_check


def _implicit_time(time, op, Cc):
    _hip.require_device(time)
    if time.dtype != torch.float32 or time.dim() != 1 or time.numel() != Cc:
        raise TypeError("implicit_solve: time must be fp32 [%d] (got %s %s)" % (Cc, time.dtype, tuple(time.shape)))
    if time.device != op.device:
        raise RuntimeError("implicit_solve: time is on %s, the operator on %s" % (time.device, op.device))
    return time.contiguous()


def implicit_solve(rowptr, col, val, mass, time, rhs, sizes=None, *, x0=None, rtol=1e-9, max_iter=1000, iters_per_check=16, check=True,
                   return_info=False):
    """Implicit (backward-Euler) diffusion, forward only (dn_implicit.hip): for every mesh b and channel c
    ``x_bc = (diag(m_b) + time[c] L_b)^-1 (m_b * rhs_bc)`` by Jacobi-preconditioned conjugate gradients started at ``x0`` (default ``rhs``: for
    small times no iteration is needed).  ``rowptr`` [V + 1], ``col`` [nnz] int32, ``val`` [nnz] fp32: L in CSR, block diagonal over the
    meshes; ``mass`` [V], ``time`` [C] (positive: the caller clamps), ``rhs`` and ``x0`` [V, C] fp32; ``sizes``: the rows of every mesh
    (default one mesh).  -> [V, C] fp32.  All solver state is fp64; a system is done when ||r|| <= ``rtol`` ||m * rhs|| over its mesh's
    rows and is frozen from then on; norms and scalars are per (mesh, channel), sums have one fixed order: two calls give the same bits.

    ``check=True``: the device's count of unfinished systems is read after every ``iters_per_check`` iterations (this form synchronises with
    the host), the loop stops on 0 and ``RuntimeError`` ("did not reach rtol") is raised when ``max_iter`` iterations leave a system
    unfinished.  ``check=False``: exactly ``max_iter`` iterations, no host read -- the capturable form; the caller reads ``info``.
    ``return_info``: also a dict ``iterations`` [n_mesh, C] int32, ``residual`` [n_mesh, C] fp64 (the recurrence's final ||r|| / ||b||),
    ``launches``.  ``ValueError`` before any launch for a rowptr or col out of range or sizes that do not sum to V; ``RuntimeError`` for
    host tensors.  The pattern is validated on its first use, which reads the device (the last eight patterns are remembered by the identity
    of their ``rowptr`` / ``col`` tensors): call once eagerly with the same tensors before capturing the check=False form in a graph."""
    op = ImplicitOperator(rowptr, col, val, mass, sizes)
    rhs = _implicit_block("rhs", rhs, op)
    time = _implicit_time(time, op, rhs.shape[1])
    if x0 is not None:
        x0 = _implicit_block("x0", x0, op, rhs.shape[1])
    rtol, max_iter, iters_per_check = _implicit_settings(rtol, max_iter, iters_per_check)
    out, info, _ = _implicit_run(rhs.detach(), time.detach(), x0.detach() if x0 is not None else None, None, op, True, rtol, max_iter,
                                 iters_per_check, bool(check))
    return (out, info) if return_info else out


class ImplicitDiffusionFn(torch.autograd.Function):
    """x = (diag(m) + t_c L)^-1 (m u_c) on a packed ``ImplicitOperator`` with gradients for u and the times (A symmetric, g = A^-1 d_x by the
    same solver started at d_x / m):  d_u = m g,  d_t[c] = - sum_b g_bc . (L_b x_bc), L x from an explicit product.  Saves the fp32 x."""

    @staticmethod
    def forward(ctx, u, time, operator, rtol=1e-9, max_iter=1000, check=True, iters_per_check=16):
        u = _implicit_block("u", u, operator)
        time = _implicit_time(time, operator, u.shape[1])
        ctx.settings = _implicit_settings(rtol, max_iter, iters_per_check) + (bool(check),)
        x, ctx.info, _ = _implicit_run(u, time, None, None, operator, True, *ctx.settings)
        ctx.operator = operator
        ctx.save_for_backward(x, time)
        return x

    @staticmethod
    def backward(ctx, d_x):
        x, time = ctx.saved_tensors
        d_u, _, d_t = _implicit_run(_implicit_block("d_x", d_x, ctx.operator, x.shape[1]), time, None, x, ctx.operator, False, *ctx.settings)
        return d_u, d_t, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# functional maps: the regularised spectral solve (include/diffnet_hip.h: dn_fmap_solve_*_f32)
# ----------------------------------------------------------------------------------------------
def _fmap_ws(A):
    P, K, F = A.shape
    return _hip.workspace(A.device, max(int(_hip.lib().dn_fmap_workspace_bytes(P, K, F)), 1024))


@_on_device
def fmap_solve_fwd(A, B, evals_x, evals_y, lam, status=None):
    """A, B [P, K, F], evals [P, K] (fp32, contiguous) -> C [P, K, K]; ``status``: an int32 word that receives the number of singular rows."""
    P, K, F = A.shape
    Cm = torch.empty(P, K, K, dtype=torch.float32, device=A.device)
    ws = _fmap_ws(A)
    _hip.check(_hip.lib().dn_fmap_solve_fwd_f32(A.data_ptr(), B.data_ptr(), evals_x.data_ptr(), evals_y.data_ptr(), P, K, F, float(lam),
                                                Cm.data_ptr(), ws.data_ptr(), ws.numel(), _hip.ptr(status), _hip.stream_of(A)),
               "dn_fmap_solve_fwd_f32")
    return Cm


@_on_device
def fmap_solve_bwd(A, B, evals_x, evals_y, lam, d_C):
    """-> (dA, dB) [P, K, F]; recomputes the factorisations from A, B and the eigenvalues."""
    P, K, F = A.shape
    dA, dB = torch.empty_like(A), torch.empty_like(B)
    ws = _fmap_ws(A)
    _hip.check(_hip.lib().dn_fmap_solve_bwd_f32(A.data_ptr(), B.data_ptr(), evals_x.data_ptr(), evals_y.data_ptr(), d_C.data_ptr(), P, K, F,
                                                float(lam), dA.data_ptr(), dB.data_ptr(), ws.data_ptr(), ws.numel(), None, _hip.stream_of(A)),
               "dn_fmap_solve_bwd_f32")
    return dA, dB


class FmapSolveFn(torch.autograd.Function):
    """C[p, i, :] = (A_p A_p^T + lam diag_j (evals_x[p, j] - evals_y[p, i])^2)^-1 (B_p A_p^T)[i, :]; gradients for A and B only."""

    @staticmethod
    def forward(ctx, A, B, evals_x, evals_y, lam, status):
        ctx.lam = lam
        ctx.save_for_backward(A, B, evals_x, evals_y)
        return fmap_solve_fwd(A, B, evals_x, evals_y, lam, status)

    @staticmethod
    def backward(ctx, d_C):
        A, B, evals_x, evals_y = ctx.saved_tensors
        dA, dB = fmap_solve_bwd(A, B, evals_x, evals_y, ctx.lam, _f32c(d_C))
        return dA, dB, None, None, None, None


def _fmap_operands(A, B, evals_x, evals_y, lam):
    """The checks of ``fmap_solve``: -> contiguous fp32 [P, K, F], [P, K] operands, the host float of lam and whether the call was unbatched."""
    for t in (A, B, evals_x, evals_y):
        _hip.require_device(t)
    A, B, evals_x, evals_y = _f32c(A), _f32c(B), _f32c(evals_x), _f32c(evals_y)
    if A.dim() not in (2, 3) or A.shape != B.shape or A.shape[-1] < 1:
        raise ValueError("fmap_solve takes two [K, F] or [P, K, F] coefficient tensors of one shape (got %s and %s)" % (tuple(A.shape), tuple(B.shape)))
    if tuple(evals_x.shape) != tuple(A.shape[:-1]) or tuple(evals_y.shape) != tuple(A.shape[:-1]):
        raise ValueError("fmap_solve takes square maps: %s eigenvalues for both shapes (got %s and %s)" % (
            tuple(A.shape[:-1]), tuple(evals_x.shape), tuple(evals_y.shape)))
    if len({t.device for t in (A, B, evals_x, evals_y)}) != 1:
        raise RuntimeError("fmap_solve: operands on %s" % ", ".join(str(t.device) for t in (A, B, evals_x, evals_y)))
    if not 1 <= A.shape[-2] <= _hip.FMAP_MAX_K:
        raise ValueError("fmap_solve kernel takes 1 <= K <= %d (got %d)" % (_hip.FMAP_MAX_K, A.shape[-2]))
    if evals_x.requires_grad or evals_y.requires_grad or (isinstance(lam, torch.Tensor) and lam.requires_grad):
        raise ValueError("fmap_solve has gradients for the coefficients only, not for the eigenvalues or lam")
    squeeze = A.dim() == 2
    if squeeze:
        A, B, evals_x, evals_y = A[None], B[None], evals_x[None], evals_y[None]
    return A, B, evals_x, evals_y, float(lam), squeeze


def fmap_solve(A, B, evals_x, evals_y, lam, check=False):
    """Functional map of spectral coefficients ``A``, ``B`` [K, F] or [P, K, F] and eigenvalues [K] or [P, K] (fp32) -> C [K, K] or
    [P, K, K]: row i is (A A^T + lam diag_j (evals_x[j] - evals_y[i])^2)^-1 (B A^T)[i, :] (include/diffnet_hip.h: dn_fmap_solve_fwd_f32),
    differentiable in A and B.  A singular row comes back as NaN; ``check=True`` reads the device's count of them -- which waits for the
    kernels -- and raises ``RuntimeError`` instead.  The default reads nothing back."""
    A, B, evals_x, evals_y, lam, squeeze = _fmap_operands(A, B, evals_x, evals_y, lam)
    status = torch.empty(1, dtype=torch.int32, device=A.device) if check else None
    Cm = FmapSolveFn.apply(A, B, evals_x, evals_y, lam, status)
    if check:
        bad = int(status.item()) if A.shape[0] else 0
        if bad:
            raise RuntimeError("fmap_solve: %d row(s) of the map have a singular system" % bad)
    return Cm[0] if squeeze else Cm


# ----------------------------------------------------------------------------------------------
# gradient sinks: a parameter may carry ``_dn_grad_sink`` (set by dist.FlatParams: its slice of the flat
# gradient bucket).  Backward then ACCUMULATES the parameter gradients of a whole op into their sinks with
# one multi-tensor add and returns None for them, instead of handing ~10 small tensors per block to
# autograd's AccumulateGrad (one 5 us add kernel each: 40 launches per step of the 4-block network).
# ----------------------------------------------------------------------------------------------
def _sinks(params):
    """The sink of a parameter counts only while the parameter still owns it: it requires grad and its ``.grad`` IS the sink
    (``zero_grad(set_to_none=True)`` or a frozen parameter switch back to returning the gradient to autograd)."""
    out = []
    for p in params:
        s = getattr(p, "_dn_grad_sink", None) if p is not None else None
        if s is not None and not (p.requires_grad and p.grad is not None and p.grad.data_ptr() == s.data_ptr()):
            s = None
        out.append(s)
    return out


def _grad_out(sink, like):
    """Output buffer for a parameter gradient.  A sink that is known to hold zeros (``dist.FlatParams.zero_grad`` marks it fresh) is
    handed to the kernel itself: its plain store IS the accumulation (0 + g), and the add launch of ``_deliver`` disappears.  The
    mark is consumed, so a second gradient for the same parameter before the next zero_grad (shared weights, several backward
    passes) goes through a temporary and is added."""
    if like is None:
        return None
    if sink is not None and getattr(sink, "_dn_fresh", False) and sink.shape == like.shape and sink.is_contiguous() \
            and sink.dtype == torch.float32 and sink.data_ptr() % 16 == 0:
        sink._dn_fresh = False
        return sink
    return torch.empty_like(like, dtype=torch.float32)


def _deliver(sinks, grads):
    pairs = [(s, g) for s, g in zip(sinks, grads) if s is not None and g is not None and g is not s]
    if pairs:
        torch._foreach_add_([s for s, g in pairs], [g for s, g in pairs])
    return [g if s is None else None for s, g in zip(sinks, grads)]


def linear_fwd(mb, x, W, b):
    """-> (out, word | None).  first_lin (thin input -> block width): its kernel leaves max |out| in a device word for block 0's
    split-fp16 engine for free"""
    out = torch.empty(x.shape[0], W.shape[0], dtype=torch.float32, device=x.device)
    word = torch.zeros(1, dtype=torch.float32, device=x.device) if (W.shape[1] <= 16 and W.shape[0] >= 128 and _amax_tags_on()) else None
    _hip.check(_hip.lib().dn_linear_fwd_amax_f32(mb.ref(), x.data_ptr(), W.shape[1], W.data_ptr(), b.data_ptr(), W.shape[0],
                                                 0, None, out.data_ptr(), _hip.ptr(word), _hip.stream_of(x)), "dn_linear_fwd_amax_f32")
    return out, word


def linear_bwd(mb, d_out, x, W, dW, db, want_dx=True):
    """dW, db: the caller's output buffers -> (d_x | None, word | None).  last_lin (block width -> a few classes): the input
    gradient's magnitude for the last block's backward, likewise for free"""
    L = _hip.lib()
    C_out, C_in = W.shape
    d_x = torch.empty_like(x) if want_dx else None
    ws, n = _ws(mb, L.dn_linear_workspace_bytes(mb.ref(), C_in, C_out))
    word = torch.zeros(1, dtype=torch.float32, device=x.device) if (want_dx and C_out <= 16 and C_in >= 128 and _amax_tags_on()) else None
    _hip.check(L.dn_linear_bwd_amax_f32(mb.ref(), d_out.data_ptr(), x.data_ptr(), W.data_ptr(), C_in, C_out, _hip.ptr(d_x),
                                        dW.data_ptr(), db.data_ptr(), _hip.ptr(word), ws.data_ptr(), n, _hip.stream_of(d_out)),
               "dn_linear_bwd_amax_f32")
    return d_x, word


class LinearFn(torch.autograd.Function):
    @staticmethod
    @_on_device
    def forward(ctx, x, W, b, mb):
        _require(x, mb)
        ctx.sinks = _sinks([W, b])
        x, W = _f32c(x), _f32c(W)
        out, word = linear_fwd(mb, x, W, _f32c(b))
        ctx.mb = mb
        ctx.save_for_backward(x, W)
        return _tag_amax(out, word)

    @staticmethod
    @_on_device
    def backward(ctx, d_out):
        x, W = ctx.saved_tensors
        dW = _grad_out(ctx.sinks[0], W)
        db = _grad_out(ctx.sinks[1], W.new_empty(W.shape[0]))
        d_x, word = linear_bwd(ctx.mb, _f32c(d_out), x, W, dW, db, ctx.needs_input_grad[0])
        dW, db = _deliver(ctx.sinks, [dW, db])
        return _tag_amax(d_x, word), dW, db, None


# ----------------------------------------------------------------------------------------------
# fused DiffusionNetBlock (layers.py:200-241)
# ----------------------------------------------------------------------------------------------
class BlockConfig:
    """Static description of one block: channel width, MiniMLP sizes, feature switches.  No call writes to it."""

    def __init__(self, C, widths, with_grad, with_rot):
        self.C, self.widths, self.with_grad, self.with_rot = int(C), [int(w) for w in widths], bool(with_grad), bool(with_rot)
        self.n_mlp = len(self.widths) - 1
        self.handle = register_handle(self)
        self.grad_hook = None        # dist.FlatParams: called after the block's gradients were delivered
        self.grad_pre_hook = None    # ... and before they are written
        self.clamp_time = False      # True: the block forward clamps diffusion_time to >= 1e-8 in place inside its first launch (layers.py:48-49)
        self.flags = 0               # per-call engine choice (include/diffnet_hip.h: DN_BLOCK_*), 0 = follow the library's option table
        if self.n_mlp > _hip.MAX_MLP:
            raise ValueError("MiniMLP deeper than %d layers is not supported by the HIP block" % _hip.MAX_MLP)


def _params_struct(cfg: BlockConfig, time, A_re, A_im, Ws, bs, masks, x_amax=None, out_amax=None):
    p = _hip.BlockParamsStruct()
    p.x_amax, p.out_amax = _hip.ptr(x_amax), _hip.ptr(out_amax)
    p.C, p.n_mlp, p.with_grad, p.with_rot = cfg.C, cfg.n_mlp, int(cfg.with_grad), int(cfg.with_rot)
    p.flags = int(cfg.flags)
    for i, w in enumerate(cfg.widths):
        p.widths[i] = w
    p.time, p.A_re, p.A_im = time.data_ptr(), _hip.ptr(A_re), _hip.ptr(A_im)
    dev_seed = None
    if isinstance(masks, tuple):      # (host seed, device seed word): in-kernel dropout under a captured graph
        masks, dev_seed = masks
    seeded = isinstance(masks, int)   # in-kernel dropout: `masks` is the 64-bit seed
    p.drop_seed = masks if seeded else 0
    p.drop_seed_dev = dev_seed.data_ptr() if dev_seed is not None else None
    for i in range(cfg.n_mlp):
        p.W[i], p.b[i] = Ws[i].data_ptr(), bs[i].data_ptr()
        p.mask[i] = _hip.ptr(masks[i]) if (masks is not None and not seeded) else None
    return p


def keep_mask_reference(seed: int, layer: int, n_rows: int, width: int):
    """numpy restatement of the in-kernel dropout bits (dn_common.h: dn_keep_bits, dn_api.hip: layer_seed) -- what
    ``mask[layer]`` would have to be for the explicit-mask path to reproduce the seeded one.  Test infrastructure."""
    import numpy as np
    M64, M32 = (1 << 64) - 1, np.uint64(0xFFFFFFFF)
    s = (seed + 0x9E3779B97F4A7C15 * (layer + 1)) & M64
    s = s or 0x9E3779B97F4A7C15
    groups = (width + 3) // 4
    rows = np.arange(n_rows, dtype=np.uint64)[:, None]
    c4 = np.arange(groups, dtype=np.uint64)[None, :]
    x = ((rows * np.uint64(groups) + c4) & M32) ^ np.uint64(s & 0xFFFFFFFF)
    x = (x + np.uint64(((s >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    bits = (x >> np.uint64(28)).astype(np.uint8)
    keep = np.stack([(bits >> e) & 1 for e in range(4)], axis=-1).reshape(n_rows, groups * 4)[:, :width]
    return torch.from_numpy(np.ascontiguousarray(keep))


def _tag_amax(t, word):
    """Attach the device word holding max |t| to the tensor object (a plain attribute: it lives and dies with that object, so it can
    never describe other data).  Autograd hands the same object on when a gradient has a single consumer; otherwise the tag is simply
    absent and the consumer measures the tensor itself.  -> t; no word (the call did not track magnitudes): no tag."""
    if word is not None:
        try:
            t._dn_amax = (word, t.data_ptr(), t._version)
        except Exception:      # noqa: BLE001
            pass
    return t


def _amax_tags_on():
    return not os.environ.get("DN_NO_AMAX_TAGS")      # diagnostic: every block measures its input itself


def _amax_of(t):
    if not _amax_tags_on():
        return None
    tag = getattr(t, "_dn_amax", None)
    if tag is None or tag[1] != t.data_ptr() or tag[2] != t._version or tag[0].device != t.device:
        return None
    return tag[0]


# Debug hook for the parity tests (off = None): a list that receives, per BlockFn.forward call with gradients wanted, a dict of the
# activations the call saved for its backward, BY NAME -- {"xs", "xd", "gx", "gy", "g", "bre", "bim", "h": [post-ReLU hidden activations]}
# (the flip-aware gradient criterion of tests/parity_cases.py needs the hidden activations the HIP forward actually produced).
debug_saved = None


class BlockSaved(NamedTuple):
    """What the block forward leaves for its backward besides the inputs: the one place that knows the flat tensor order
    (``save_for_backward``, the output list of ``torch.ops.diffusion_net.block``) and that fills a ``BlockSavedStruct``."""
    xs: torch.Tensor
    xd: torch.Tensor
    words: torch.Tensor      # [magnitude words of the saved activations | max |out|]
    feats: list              # gx, gy, g, bre, bim with gradient features, else empty
    hs: list                 # post-ReLU hidden activations of the MiniMLP
    hbits: torch.Tensor = None   # int32 [n_mlp - 1, V, 4] at C = 64, 128 (else [0, V, 4]: no words exist): their signs as bit words (dn_block_saved_t.hbits); None: not passed

    def flat(self):
        return [self.xs, self.xd, self.words, self.hbits, *self.feats, *self.hs]

    @classmethod
    def from_flat(cls, cfg, ts):
        n_feat = 5 if cfg.with_grad else 0
        return cls(ts[0], ts[1], ts[2], list(ts[4:4 + n_feat]), list(ts[4 + n_feat:]), ts[3])

    def struct(self):
        sv = _hip.BlockSavedStruct()
        sv.xs, sv.xd = self.xs.data_ptr(), self.xd.data_ptr()
        if self.feats:
            sv.gx, sv.gy, sv.g, sv.bre, sv.bim = (t.data_ptr() for t in self.feats)
        for i, h in enumerate(self.hs):
            sv.h[i] = h.data_ptr()
        sv.amax = self.words.data_ptr()
        if self.hbits is not None:
            base, step = self.hbits.data_ptr(), 4 * self.hbits.stride(0)      # (no per-layer tensor view: this runs once per block call on the host)
            for i in range(self.hbits.shape[0]):
                sv.hbits[i] = base + i * step
        return sv

    def named(self):
        return {"xs": self.xs, "xd": self.xd, **dict(zip(("gx", "gy", "g", "bre", "bim"), self.feats)), "h": list(self.hs), "words": self.words, "hbits": self.hbits}


def block_fwd(mb, cfg, masks, x, time, A_re, A_im, Ws, bs, x_amax=None, save=True, clamp=False):
    """-> (out, BlockSaved | None, out_amax | None).  ``save``: the training forward, which writes what the backward needs; ``clamp``:
    clamp ``time`` to >= 1e-8 in place inside the first launch."""
    L = _hip.lib()
    V, Cc = x.shape[0], cfg.C
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
    # magnitude words of the split-fp16 engine (dn_api.hip): the input's (``x_amax``) travels with the tensor from the block that produced it,
    # this block's output gets one for the next block; a tensor without one is measured by the library (one extra pass).
    # words = [saved-activation words | max |out|].  Uninitialised on purpose (a fill per block and step is a launch): a call that tracks
    # magnitudes zeroes and writes them itself; one that does not leaves them alone, and then nothing reads them -- ``out_amax`` is handed
    # back, and the backward reads the words, only where dn_block_tracks_amax says so
    words = new(_hip.BLOCK_AMAX_WORDS + 1)
    out_amax = words[_hip.BLOCK_AMAX_WORDS:]
    p = _params_struct(cfg, time, A_re, A_im, Ws, bs, masks, x_amax, out_amax)
    p.clamp_time = int(clamp)
    out = new(V, Cc)
    saved = sv = None
    if save:
        saved = BlockSaved(new(mb.n_mesh, mb.k_eig, Cc), new(V, Cc), words, [new(V, Cc) for _ in range(5)] if cfg.with_grad else [],
                           [new(V, cfg.widths[i + 1]) for i in range(cfg.n_mlp - 1)],
                           torch.empty(cfg.n_mlp - 1 if Cc in (64, 128) else 0, V, 4, dtype=torch.int32, device=x.device))
        sv = saved.struct()
    ws, n = _ws(mb, L.dn_block_fwd_workspace_bytes(mb.ref(), C.byref(p), int(save)))
    _hip.check(L.dn_block_fwd_f32(mb.ref(), C.byref(p), x.data_ptr(), out.data_ptr(), C.byref(sv) if save else None, ws.data_ptr(), n,
                                  _hip.stream_of(x)), "dn_block_fwd_f32")
    return out, saved, (out_amax if L.dn_block_tracks_amax(mb.ref(), C.byref(p), int(save)) else None)


def block_bwd(mb, cfg, masks, d_out, x, time, A_re, A_im, Ws, bs, saved, grads, d_out_amax=None):
    """grads: the caller's output buffers [d_time, dA_re | None, dA_im | None, dW_0, db_0, dW_1, ...] -> (d_x, d_x_amax | None)"""
    L = _hip.lib()
    p = _params_struct(cfg, time, A_re, A_im, Ws, bs, masks)
    sv, gr = saved.struct(), _hip.BlockGradsStruct()
    d_x = torch.empty_like(x)
    dx_amax = torch.empty(1, dtype=torch.float32, device=d_x.device)      # (written only, and returned only, when the call tracks magnitudes)
    gr.d_x, gr.d_time, gr.dA_re, gr.dA_im = d_x.data_ptr(), grads[0].data_ptr(), _hip.ptr(grads[1]), _hip.ptr(grads[2])
    gr.d_out_amax, gr.d_x_amax = _hip.ptr(d_out_amax), dx_amax.data_ptr()
    for i in range(cfg.n_mlp):
        gr.dW[i], gr.db[i] = grads[3 + 2 * i].data_ptr(), grads[4 + 2 * i].data_ptr()
    ws, n = _ws(mb, L.dn_block_bwd_workspace_bytes(mb.ref(), C.byref(p)))
    _hip.check(L.dn_block_bwd_f32(mb.ref(), C.byref(p), x.data_ptr(), C.byref(sv), d_out.data_ptr(), C.byref(gr),
                                  ws.data_ptr(), n, _hip.stream_of(d_out)), "dn_block_bwd_f32")
    return d_x, (dx_amax if L.dn_block_tracks_amax(mb.ref(), C.byref(p), 2) else None)


class BlockFn(torch.autograd.Function):
    """forward(x, time, A_re, A_im, *W_and_b) with non-tensor (mb, cfg, masks, grad_enabled) first."""

    @staticmethod
    @_on_device
    def forward(ctx, mb, cfg, masks, grad_enabled, x, time, A_re, A_im, *wb):
        _require(x, mb)
        ctx.sinks = _sinks([time, A_re, A_im, *wb])
        time_param = time
        x, time = _f32c(x), _f32c(time)
        clamp = cfg.clamp_time
        if clamp and time.data_ptr() != time_param.data_ptr():     # a converted copy: the library would clamp the copy, not the Parameter
            time_param.data.clamp_(min=1e-8)
            time, clamp = _f32c(time_param), False
        A_re = _f32c(A_re) if A_re is not None else None
        A_im = _f32c(A_im) if A_im is not None else None
        Ws = [_f32c(w) for w in wb[0::2]]
        bs = [_f32c(b) for b in wb[1::2]]
        # ctx.needs_input_grad is True for every Parameter even under torch.no_grad() (torch 2.10), and grad mode is always off inside a
        # Function's forward: the caller samples torch.is_grad_enabled() and passes it as ``grad_enabled`` (layers.forward_packed).  Until
        # round 6 every "inference" call through the package ran the TRAINING forward (eight saved arrays of [V, C] written per block: +11 %
        # at BASELINE config 4's shape) -- and with it never took the inference-only kernel choices.
        need_grad = any(ctx.needs_input_grad) and grad_enabled
        out, saved, out_amax = block_fwd(mb, cfg, masks, x, time, A_re, A_im, Ws, bs, _amax_of(x), need_grad, clamp)
        if need_grad:
            ctx.mb, ctx.cfg, ctx.masks = mb, cfg, masks
            ctx.has = (A_re is not None, A_im is not None)
            ctx.save_for_backward(x, time, *Ws, *bs, *saved.flat(), *(t for t in (A_re, A_im) if t is not None))
            if debug_saved is not None:
                debug_saved.append(saved.named())
        return _tag_amax(out, out_amax)  # the next block reads it off its input (a call that does not track magnitudes leaves the word alone: no tag)

    @staticmethod
    @_on_device
    def backward(ctx, d_out):
        mb, cfg, masks = ctx.mb, ctx.cfg, ctx.masks
        if cfg.grad_pre_hook is not None:
            cfg.grad_pre_hook()
        sav, n = list(ctx.saved_tensors), cfg.n_mlp
        A_im = sav.pop() if ctx.has[1] else None
        A_re = sav.pop() if ctx.has[0] else None
        x, time, Ws, bs = sav[0], sav[1], sav[2:2 + n], sav[2 + n:2 + 2 * n]
        d_out = _f32c(d_out)
        likes = [time, A_re, A_im]
        for w, b in zip(Ws, bs):
            likes += [w, b]
        grads = [_grad_out(s, t) for s, t in zip(ctx.sinks, likes)]      # order: time, A_re, A_im, W0, b0, W1, b1, ...
        d_x, dx_amax = block_bwd(mb, cfg, masks, d_out, x, time, A_re, A_im, Ws, bs, BlockSaved.from_flat(cfg, sav[2 + 2 * n:]), grads,
                                 _amax_of(d_out))
        grads = _deliver(ctx.sinks, grads)
        if cfg.grad_hook is not None:          # dist.FlatParams: this block's gradient range may go out now
            cfg.grad_hook()
        # (the tag: the block before this one finds it on the gradient it receives)
        return (None, None, None, None, _tag_amax(d_x, dx_amax), *grads)


# ----------------------------------------------------------------------------------------------
# output remaps (layers.py:379-397)
# ----------------------------------------------------------------------------------------------
def _csr_mean(x, rowptr, col, n_out, n_per):
    out = torch.empty(n_out, x.shape[1], dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().dn_csr_mean_f32(rowptr.data_ptr(), col.data_ptr(), n_out, x.data_ptr(), x.shape[1], float(n_per), out.data_ptr(),
                                          _hip.stream_of(x)), "dn_csr_mean_f32")
    return out


def gather_mean_fwd(x, pat: GatherPattern):
    return _csr_mean(x, pat.rowptr, pat.col, pat.n_out, pat.n_per)


def gather_mean_bwd(d_out, pat: GatherPattern):
    return _csr_mean(d_out, pat.t_rowptr, pat.t_col, pat.n_src, pat.n_per)


class GatherMeanFn(torch.autograd.Function):
    """out[i] = mean_j x[index[i, j]]  (faces: 3 rows, edges: 2 rows)"""

    @staticmethod
    @_on_device
    def forward(ctx, x, pat: GatherPattern):
        _require(x)
        ctx.pat = pat
        return gather_mean_fwd(_f32c(x), pat)

    @staticmethod
    @_on_device
    def backward(ctx, d_out):
        return gather_mean_bwd(_f32c(d_out), ctx.pat), None


def mass_mean_fwd(mb, x):
    """-> (out, msum): the per-mesh mass sums are what the backward needs"""
    out = torch.empty(mb.n_mesh, x.shape[1], dtype=torch.float32, device=x.device)
    msum = torch.empty(mb.n_mesh, dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().dn_mass_mean_fwd_f32(mb.ref(), x.data_ptr(), x.shape[1], out.data_ptr(), msum.data_ptr(),
                                               _hip.stream_of(x)), "dn_mass_mean_fwd_f32")
    return out, msum


def mass_mean_bwd(mb, msum, d_out):
    d_x = torch.empty(mb.v_total, d_out.shape[1], dtype=torch.float32, device=d_out.device)
    _hip.check(_hip.lib().dn_mass_mean_bwd_f32(mb.ref(), msum.data_ptr(), d_out.data_ptr(), d_out.shape[1],
                                               d_x.data_ptr(), _hip.stream_of(d_out)), "dn_mass_mean_bwd_f32")
    return d_x


class MassMeanFn(torch.autograd.Function):
    """out[m] = sum_v mass_v x_v / sum_v mass_v over the vertices of mesh m (layers.py:397)"""

    @staticmethod
    @_on_device
    def forward(ctx, x, mb):
        _require(x, mb)
        out, msum = mass_mean_fwd(mb, _f32c(x))
        ctx.mb = mb
        ctx.save_for_backward(msum)
        return out

    @staticmethod
    @_on_device
    def backward(ctx, d_out):
        return mass_mean_bwd(ctx.mb, ctx.saved_tensors[0], _f32c(d_out)), None


# ----------------------------------------------------------------------------------------------
# the head on the far side of the path (dn_head.hip): [gather-mean] -> [log_softmax] -> log-probabilities -> [NLL / smoothed loss]
# ----------------------------------------------------------------------------------------------
def head_fwd(x, pat, labels, log_softmax, smoothing, need_logp):
    """-> (logp | None, loss | None, count | None, labels as the kernel read them: flat int64 | None)"""
    L = _hip.lib()
    n_src, Cc = x.shape
    if Cc > _hip.HEAD_MAX_CLASSES:
        raise ValueError("the fused head handles up to %d classes (got %d); DiffusionNet.forward_packed composes the remap and the "
                         "activation from separate ops above that" % (_hip.HEAD_MAX_CLASSES, Cc))
    n_out = pat.n_out if pat is not None else n_src
    if labels is not None:
        if labels.dtype != torch.int64:
            raise TypeError("labels must be int64")
        labels = labels.reshape(-1).contiguous()
        if labels.numel() != n_out:
            raise ValueError("expected %d labels, got %d" % (n_out, labels.numel()))
    logp = torch.empty(n_out, Cc, dtype=torch.float32, device=x.device) if need_logp else None
    loss = torch.empty((), dtype=torch.float32, device=x.device) if labels is not None else None
    count = torch.empty((), dtype=torch.float32, device=x.device) if labels is not None else None
    ws = _hip.workspace(x.device, L.dn_head_workspace_bytes())
    _hip.check(L.dn_head_fwd_f32(x.data_ptr(), n_src, Cc, _hip.ptr(pat.rowptr) if pat is not None else None,
                                 _hip.ptr(pat.col) if pat is not None else None, n_out, float(pat.n_per) if pat is not None else 1.0,
                                 int(bool(log_softmax)), _hip.ptr(labels), float(smoothing), _hip.ptr(logp), _hip.ptr(loss), _hip.ptr(count),
                                 ws.data_ptr(), ws.numel(), _hip.stream_of(x)), "dn_head_fwd_f32")
    return logp, loss, count, labels


def head_bwd(pat, log_softmax, smoothing, shape, logp, labels, count, d_logp, d_loss):
    """shape: (n_src, n_out, classes); any combination of incoming d_logp / d_loss -> d_x"""
    n_src, n_out, Cc = shape
    ref = d_logp if d_logp is not None else d_loss
    d_x = torch.empty(n_src, Cc, dtype=torch.float32, device=ref.device)
    _hip.check(_hip.lib().dn_head_bwd_f32(_hip.ptr(logp), n_out, Cc, _hip.ptr(pat.t_rowptr) if pat is not None else None,
                                          _hip.ptr(pat.t_col) if pat is not None else None, n_src, float(pat.n_per) if pat is not None else 1.0,
                                          int(log_softmax), _hip.ptr(labels) if d_loss is not None else None, float(smoothing), _hip.ptr(d_logp),
                                          _hip.ptr(d_loss), _hip.ptr(count), d_x.data_ptr(), _hip.stream_of(ref)), "dn_head_bwd_f32")
    return d_x


class HeadFn(torch.autograd.Function):
    """forward(x, pat, labels, log_softmax, smoothing, want_logp) -> (logp or None, loss or None)

    x: [n_src, C] logits (log-probabilities when ``log_softmax`` is False); pat: GatherPattern of the faces/edges remap or None
    (output i = row i); labels: int64 [n_out] or None.  One kernel forward (+ a 1-block finish when there is a loss), one kernel
    backward for any combination of incoming d_logp / d_loss."""

    @staticmethod
    @_on_device
    def forward(ctx, x, pat, labels, log_softmax, smoothing, want_logp):
        _require(x)
        need_logp = want_logp or (log_softmax and ctx.needs_input_grad[0])   # the backward of log_softmax needs the probabilities
        logp, loss, count, labels = head_fwd(_f32c(x), pat, labels, log_softmax, smoothing, need_logp)
        ctx.args = (pat, bool(log_softmax), float(smoothing), (x.shape[0], pat.n_out if pat is not None else x.shape[0], x.shape[1]))
        ctx.has = (logp is not None, labels is not None)
        ctx.save_for_backward(*[t for t in (logp, labels, count) if t is not None])
        return (logp if want_logp else None), loss

    @staticmethod
    @_on_device
    def backward(ctx, d_logp, d_loss):
        sav = list(ctx.saved_tensors)
        logp = sav.pop(0) if ctx.has[0] else None
        labels, count = sav if ctx.has[1] else (None, None)
        d_logp = _f32c(d_logp) if d_logp is not None else None
        d_loss = _f32c(d_loss) if d_loss is not None else None
        return head_bwd(*ctx.args, logp, labels, count, d_logp, d_loss), None, None, None, None, None

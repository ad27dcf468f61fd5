"""``torch.library`` registration of the hot ops ("called from the Python torch.library op implementations").

The eager path calls the ``torch.autograd.Function``s of ``ops.py`` directly.  They take Python objects (a packed ``MeshBatch``, a
``BlockConfig``) and call the C ABI through ctypes -- opaque to ``torch.compile`` / ``torch.export``, which would either try to trace
into the ctypes calls or break the graph around them.  Here every op of the packed forward is ALSO registered as a custom operator
(``torch.ops.diffusion_net.*``) with a fake (meta) kernel and an autograd formula whose backward is itself a registered op, so that a
compiled ``DiffusionNet.forward_packed`` is one graph with the ops as opaque nodes (``tests/test_gpu_parity.py::
test_torch_compile_packed_forward``: ``fullgraph=True``).  The implementations are the SAME code: each custom op calls the
plain launch function (``ops.*_fwd`` / ``ops.*_bwd``) that the matching ``ops.*Fn`` wraps.  ``layers.py`` routes through these ops only
while a compiler is tracing (``torch.compiler.is_compiling()``); eager execution keeps its direct path (gradient sinks, dist hooks).  The
magnitude tags of ``ops._tag_amax`` travel here too, wherever the tensor object an op returned is the one the next op receives.

Non-tensor operands travel as integer handles into a weak registry (the caller owns the objects, as with the eager path).  The eager
autograd formulas pin the objects their backward looks up for as long as the autograd node lives (``_hold``); a COMPILED graph calls the
forward and backward ops directly and holds only the integers: there the caller must keep ``mb`` / ``gather`` alive until the backward has
run (a dead handle raises a RuntimeError that says so).  Handles are graph constants for ``torch.compile``: a compiled
``forward_packed`` is specialised to its ``MeshBatch`` and recompiles for another one -- compile per static batch (as
``graphs.GraphedTrainStep`` captures per batch), not inside a loop over meshes.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor
from torch.library import custom_op, infer_schema

from . import _hip, ops
import weakref

from .batch import handle_object as _obj   # handles are attributes of the objects (MeshBatch.handle, ...), assigned at construction
from .batch import pin_handle as _pin, unpin_handle as _unpin


def _hold(ctx, *handles):
    """Keep the objects behind ``handles`` alive as long as the autograd context ``ctx`` is (no-op while a compiler traces with fake tensors:
    nothing will look the handles up through this context)."""
    if torch.compiler.is_compiling():
        return
    for k in handles:
        if isinstance(k, int) and k:
            try:
                _pin(k)
                weakref.finalize(ctx, _unpin, k)
            except TypeError:          # a context type that cannot be weakly referenced: fall back to the caller-owns rule
                _unpin(k)


def _op(name):
    """A custom operator that mutates no argument and runs with its tensors' device current, as the eager Functions do."""
    return lambda fn: custom_op(name, mutates_args=(), schema=infer_schema(fn, mutates_args=()))(ops._on_device(fn))


def _e(like: Tensor) -> Tensor:
    return like.new_empty(0)


def _c(t: Optional[Tensor]) -> Optional[Tensor]:
    return ops._f32c(t) if t is not None else None


def _in(x: Tensor, mb=None) -> Tensor:
    """The checks and conversions the eager Functions make on their leading operand."""
    ops._require(x, mb)
    return _c(x)


# ------------------------------------------------------------------------------------------------ nn.Linear on the row axis
@_op("diffusion_net::linear")
def linear(x: Tensor, W: Tensor, b: Tensor, mb: int) -> Tensor:
    return ops._tag_amax(*ops.linear_fwd(_obj(mb), _in(x, _obj(mb)), _c(W), _c(b)))


@linear.register_fake
def _(x, W, b, mb):
    return x.new_empty(x.shape[0], W.shape[0])


@_op("diffusion_net::linear_bwd")
def linear_bwd(d_out: Tensor, x: Tensor, W: Tensor, mb: int) -> List[Tensor]:
    dW, db = torch.empty_like(W), W.new_empty(W.shape[0])
    return [ops._tag_amax(*ops.linear_bwd(_obj(mb), _c(d_out), x, W, dW, db)), dW, db]


@linear_bwd.register_fake
def _(d_out, x, W, mb):
    return [torch.empty_like(x), torch.empty_like(W), W.new_empty(W.shape[0])]


def _linear_setup(ctx, inputs, output):
    x, W, b, mb = inputs
    ctx.save_for_backward(x, W)
    ctx.mb = mb
    _hold(ctx, mb)


def _linear_backward(ctx, g):
    x, W = ctx.saved_tensors
    d_x, dW, db = linear_bwd(g.contiguous(), x, W, ctx.mb)
    return d_x, dW, db, None


linear.register_autograd(_linear_backward, setup_context=_linear_setup)


# ------------------------------------------------------------------------------------------------ fused DiffusionNetBlock
def _masks(seed: int, seed_dev: Optional[Tensor]):
    if seed == 0:
        return None
    return (seed, seed_dev) if seed_dev is not None else seed


@_op("diffusion_net::block")
def block(x: Tensor, time: Tensor, A_re: Optional[Tensor], A_im: Optional[Tensor], wb: List[Tensor], mb: int, cfg: int, seed: int,
          seed_dev: Optional[Tensor], n_mesh: int, k_eig: int) -> List[Tensor]:
    """-> [out, xs, xd, words, hbits, (gx, gy, g, bre, bim), h_0 ...]: the output and what the backward needs besides the inputs."""
    # save on: this op always returns what its backward op needs; clamp off: `time` is an input of a custom op that declares no mutation,
    # the caller has clamped it (layers.forward_packed)
    x = _in(x, _obj(mb))
    out, saved, out_amax = ops.block_fwd(_obj(mb), _obj(cfg), _masks(seed, seed_dev), x, _c(time), _c(A_re), _c(A_im), [_c(w) for w in wb[0::2]],
                                         [_c(b) for b in wb[1::2]], ops._amax_of(x), save=True, clamp=False)
    return [ops._tag_amax(out, out_amax)] + saved.flat()


@block.register_fake
def _(x, time, A_re, A_im, wb, mb, cfg, seed, seed_dev, n_mesh, k_eig):
    # (shapes from the operands alone: the handles may be symbolic while tracing)
    V, Cw = x.shape[0], x.shape[1]
    new = lambda *s: x.new_empty(*s)
    outs = [new(V, Cw), new(n_mesh, k_eig, Cw), new(V, Cw), new(_hip.BLOCK_AMAX_WORDS + 1),
            x.new_empty(len(wb) // 2 - 1 if Cw in (64, 128) else 0, V, 4, dtype=torch.int32)]
    outs += [new(V, Cw) for _ in range(5 if A_re is not None else 0)]
    outs += [new(V, w.shape[0]) for w in wb[0:-2:2]]
    return outs


@_op("diffusion_net::block_bwd")
def block_bwd(d_out: Tensor, x: Tensor, time: Tensor, A_re: Optional[Tensor], A_im: Optional[Tensor], wb: List[Tensor], saved: List[Tensor],
              mb: int, cfg: int, seed: int, seed_dev: Optional[Tensor]) -> List[Tensor]:
    """-> [d_x, d_time, dA_re | empty, dA_im | empty, dW_0, db_0, ...]"""
    c, d_out = _obj(cfg), _c(d_out)
    grads = [torch.empty_like(t) if t is not None else None for t in (time, A_re, A_im, *wb)]
    d_x, dx_amax = ops.block_bwd(_obj(mb), c, _masks(seed, seed_dev), d_out, x, time, A_re, A_im, wb[0::2], wb[1::2],
                                 ops.BlockSaved.from_flat(c, saved), grads, ops._amax_of(d_out))
    return [ops._tag_amax(d_x, dx_amax)] + [g if g is not None else _e(x) for g in grads]


@block_bwd.register_fake
def _(d_out, x, time, A_re, A_im, wb, saved, mb, cfg, seed, seed_dev):
    return [torch.empty_like(x), torch.empty_like(time), torch.empty_like(A_re) if A_re is not None else _e(x),
            torch.empty_like(A_im) if A_im is not None else _e(x)] + [torch.empty_like(t) for t in wb]


def _block_setup(ctx, inputs, output):
    x, time, A_re, A_im, wb, mb, cfg, seed, seed_dev, _n_mesh, _k_eig = inputs
    ctx.n_wb = len(wb)
    ctx.has = (A_re is not None, A_im is not None, seed_dev is not None)
    ctx.ints = (mb, cfg, seed)
    _hold(ctx, mb, cfg)
    ctx.save_for_backward(x, time, *([A_re] if A_re is not None else []), *([A_im] if A_im is not None else []), *wb, *output[1:],
                          *([seed_dev] if seed_dev is not None else []))


def _block_backward(ctx, grads):
    sav = list(ctx.saved_tensors)
    x, time = sav[0], sav[1]
    pos = 2
    A_re = A_im = seed_dev = None
    if ctx.has[0]:
        A_re = sav[pos]; pos += 1
    if ctx.has[1]:
        A_im = sav[pos]; pos += 1
    wb = sav[pos:pos + ctx.n_wb]; pos += ctx.n_wb
    if ctx.has[2]:
        seed_dev = sav[-1]
        saved = sav[pos:-1]
    else:
        saved = sav[pos:]
    mb, cfg, seed = ctx.ints
    g = block_bwd(grads[0].contiguous(), x, time, A_re, A_im, wb, saved, mb, cfg, seed, seed_dev)
    return (g[0], g[1], g[2] if ctx.has[0] else None, g[3] if ctx.has[1] else None, list(g[4:]), None, None, None, None, None, None)


block.register_autograd(_block_backward, setup_context=_block_setup)


# ------------------------------------------------------------------------------------------------ output remaps
@_op("diffusion_net::gather_mean")
def gather_mean(x: Tensor, pat: int, n_out: int) -> Tensor:
    return ops.gather_mean_fwd(_in(x), _obj(pat))


@gather_mean.register_fake
def _(x, pat, n_out):
    return x.new_empty(n_out, x.shape[1])


@_op("diffusion_net::gather_mean_bwd")
def gather_mean_bwd(d_out: Tensor, pat: int, n_src: int) -> Tensor:
    return ops.gather_mean_bwd(_c(d_out), _obj(pat))


@gather_mean_bwd.register_fake
def _(d_out, pat, n_src):
    return d_out.new_empty(n_src, d_out.shape[1])


def _gm_setup(ctx, inputs, output):
    ctx.pat, ctx.n_src = inputs[1], inputs[0].shape[0]
    _hold(ctx, ctx.pat)


gather_mean.register_autograd(lambda ctx, g: (gather_mean_bwd(g.contiguous(), ctx.pat, ctx.n_src), None, None), setup_context=_gm_setup)


@_op("diffusion_net::mass_mean")
def mass_mean(x: Tensor, mb: int, n_mesh: int) -> List[Tensor]:
    return list(ops.mass_mean_fwd(_obj(mb), _in(x, _obj(mb))))


@mass_mean.register_fake
def _(x, mb, n_mesh):
    return [x.new_empty(n_mesh, x.shape[1]), x.new_empty(n_mesh)]


@_op("diffusion_net::mass_mean_bwd")
def mass_mean_bwd(d_out: Tensor, msum: Tensor, mb: int, v_total: int) -> Tensor:
    return ops.mass_mean_bwd(_obj(mb), msum, _c(d_out))


@mass_mean_bwd.register_fake
def _(d_out, msum, mb, v_total):
    return d_out.new_empty(v_total, d_out.shape[1])


def _mm_setup(ctx, inputs, output):
    ctx.mb, ctx.v_total = inputs[1], inputs[0].shape[0]
    _hold(ctx, ctx.mb)
    ctx.save_for_backward(output[1])


mass_mean.register_autograd(lambda ctx, grads: (mass_mean_bwd(grads[0].contiguous(), ctx.saved_tensors[0], ctx.mb, ctx.v_total), None, None),
                            setup_context=_mm_setup)


# ------------------------------------------------------------------------------------------------ fused head (remap + log_softmax + loss)
@_op("diffusion_net::head")
def head(x: Tensor, pat: int, labels: Optional[Tensor], log_softmax: bool, smoothing: float, n_out: int) -> List[Tensor]:
    """-> [log-probabilities, loss | empty, valid-row count | empty]"""
    logp, loss, count, _ = ops.head_fwd(_in(x), _obj(pat), labels, log_softmax, smoothing, True)
    return [logp, loss if loss is not None else _e(x), count if count is not None else _e(x)]


@head.register_fake
def _(x, pat, labels, log_softmax, smoothing, n_out):
    sc = lambda: x.new_empty(()) if labels is not None else _e(x)
    return [x.new_empty(n_out, x.shape[1]), sc(), sc()]


@_op("diffusion_net::head_bwd")
def head_bwd(d_logp: Optional[Tensor], d_loss: Optional[Tensor], logp: Tensor, labels: Optional[Tensor], count: Optional[Tensor], pat: int,
             log_softmax: bool, smoothing: float, n_src: int) -> Tensor:
    return ops.head_bwd(_obj(pat), log_softmax, smoothing, (n_src, logp.shape[0], logp.shape[1]), logp, labels, count if labels is not None else None,
                        _c(d_logp), _c(d_loss))


@head_bwd.register_fake
def _(d_logp, d_loss, logp, labels, count, pat, log_softmax, smoothing, n_src):
    return logp.new_empty(n_src, logp.shape[1])


def _head_setup(ctx, inputs, output):
    x, pat, labels, lsm, smoothing, _n_out = inputs
    ctx.meta = (pat, lsm, smoothing, x.shape[0], labels is not None)
    _hold(ctx, pat)
    ctx.save_for_backward(output[0], *([labels, output[2]] if labels is not None else []))


def _head_backward(ctx, grads):
    pat, lsm, smoothing, n_src, has_lab = ctx.meta
    sav = ctx.saved_tensors
    d_logp = grads[0].contiguous() if grads[0] is not None else None
    d_loss = grads[1].contiguous() if (has_lab and grads[1] is not None) else None
    d_x = head_bwd(d_logp, d_loss, sav[0], sav[1] if has_lab else None, sav[2] if has_lab else None, pat, lsm, smoothing, n_src)
    return d_x, None, None, None, None, None


head.register_autograd(_head_backward, setup_context=_head_setup)


# ------------------------------------------------------------------------------------------------ nearest neighbours (forward only)
@_op("diffusion_net::knn")
def knn(src: Tensor, tgt: Tensor, k: int, largest: bool, omit_diagonal: bool) -> Tuple[Tensor, Tensor]:
    return ops.knn(src, tgt, k, largest, omit_diagonal)


@knn.register_fake
def _(src, tgt, k, largest, omit_diagonal):
    return src.new_empty(src.shape[0], k, dtype=torch.float32), src.new_empty(src.shape[0], k, dtype=torch.int64)   # ops.knn is fp32


@_op("diffusion_net::knn_grid")
def knn_grid(src: Tensor, tgt: Tensor, k: int, omit_diagonal: bool, cells_per_axis: int) -> Tuple[Tensor, Tensor]:
    return ops.knn_grid(src, tgt, k, omit_diagonal, cells_per_axis)


@knn_grid.register_fake
def _(src, tgt, k, omit_diagonal, cells_per_axis):
    return src.new_empty(src.shape[0], k, dtype=torch.float32), src.new_empty(src.shape[0], k, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ farthest point sampling (forward only)
@_op("diffusion_net::fps")
def fps(points: Tensor, n_sample: int) -> Tuple[Tensor, Tensor]:
    order, radii = ops.fps(points, n_sample)
    return order[0], radii[0]


@fps.register_fake
def _(points, n_sample):
    return points.new_empty(n_sample, dtype=torch.int64), points.new_empty(n_sample, dtype=torch.float32)   # ops.fps is fp32


# ------------------------------------------------------------------------------------------------ point-cloud Laplacian (forward only)
@_op("diffusion_net::cloud_laplacian")
def cloud_laplacian(points: Tensor, nbr: Tensor, frames: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.cloud_laplacian(points, nbr, frames)


@cloud_laplacian.register_fake
def _(points, nbr, frames):
    n, k = nbr.shape
    nnz = torch.library.get_ctx().new_dynamic_size()       # the number of entries depends on the data
    return (points.new_empty(n, k, dtype=torch.int32), points.new_empty(n + 1, dtype=torch.int32), points.new_empty(nnz, dtype=torch.int32),
            points.new_empty(nnz, dtype=torch.float32), points.new_empty(n, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ triangle-mesh operators (forward only)
@_op("diffusion_net::mesh_assemble")
def mesh_assemble(verts: Tensor, faces: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.mesh_assemble(verts, faces)


@mesh_assemble.register_fake
def _(verts, faces):
    V = verts.shape[0]
    nnz = torch.library.get_ctx().new_dynamic_size()       # the number of entries depends on the data
    return (verts.new_empty(V + 1, dtype=torch.int32), verts.new_empty(nnz, dtype=torch.int32), verts.new_empty(nnz, dtype=torch.float64),
            verts.new_empty(V, dtype=torch.float64), verts.new_empty(V, 3, dtype=torch.float64))


@_op("diffusion_net::mesh_frames_gradients")
def mesh_frames_gradients(verts: Tensor, rowptr: Tensor, col: Tensor, normals: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    return ops.mesh_frames_gradients(verts, rowptr, col, normals)


@mesh_frames_gradients.register_fake
def _(verts, rowptr, col, normals):
    V, nnz = verts.shape[0], col.shape[0]
    return (verts.new_empty(V, 3, 3, dtype=torch.float64), verts.new_empty(nnz, dtype=torch.float64), verts.new_empty(nnz, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ functional maps (regularised spectral solve)
@_op("diffusion_net::fmap_solve")
def fmap_solve(A: Tensor, B: Tensor, evals_x: Tensor, evals_y: Tensor, lam: float) -> Tensor:
    A, B, evals_x, evals_y, lam, squeeze = ops._fmap_operands(A, B, evals_x, evals_y, lam)
    Cm = ops.fmap_solve_fwd(A, B, evals_x, evals_y, lam, None)
    return Cm[0] if squeeze else Cm


@fmap_solve.register_fake
def _(A, B, evals_x, evals_y, lam):
    return A.new_empty(*A.shape[:-1], A.shape[-2], dtype=torch.float32)   # ops.fmap_solve is fp32


@_op("diffusion_net::fmap_solve_bwd")
def fmap_solve_bwd(d_C: Tensor, A: Tensor, B: Tensor, evals_x: Tensor, evals_y: Tensor, lam: float) -> Tuple[Tensor, Tensor]:
    A3, B3, evals_x, evals_y, lam, _ = ops._fmap_operands(A, B, evals_x, evals_y, lam)
    dA, dB = ops.fmap_solve_bwd(A3, B3, evals_x, evals_y, lam, _c(d_C))
    return dA.reshape(A.shape), dB.reshape(B.shape)


@fmap_solve_bwd.register_fake
def _(d_C, A, B, evals_x, evals_y, lam):
    return A.new_empty(A.shape, dtype=torch.float32), B.new_empty(B.shape, dtype=torch.float32)


def _fmap_setup(ctx, inputs, output):
    ctx.lam = inputs[4]
    ctx.save_for_backward(*inputs[:4])


fmap_solve.register_autograd(lambda ctx, grad: (*fmap_solve_bwd(grad.contiguous(), *ctx.saved_tensors, ctx.lam), None, None, None),
                             setup_context=_fmap_setup)


# ------------------------------------------------------------------------------------------------ Laplacian eigenbasis (forward only)
@_op("diffusion_net::cheb_step")
def cheb_step(rowptr: Tensor, col: Tensor, val: Tensor, Y: Tensor, Z: Optional[Tensor], alpha: float, beta: float, gamma: float) -> Tensor:
    """``alpha * S @ Y + beta * Y + gamma * Z`` into a new block (``ops.cheb_step`` without ``out``: a custom operator mutates nothing)."""
    return ops.cheb_step(rowptr, col, val, Y, Z, alpha, beta, gamma)


@cheb_step.register_fake
def _(rowptr, col, val, Y, Z, alpha, beta, gamma):
    return Y.new_empty(Y.shape, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ implicit diffusion (sparse per-channel PCG)
def _implicit_op(rowptr, col, val, mass, sizes):
    return ops.ImplicitOperator(rowptr, col, val, mass, list(sizes) if sizes else None)


@_op("diffusion_net::implicit_solve")
def implicit_solve(rowptr: Tensor, col: Tensor, val: Tensor, mass: Tensor, time: Tensor, rhs: Tensor, sizes: List[int], x0: Optional[Tensor],
                   rtol: float, max_iter: int) -> Tensor:
    """``ops.implicit_solve(..., check=False)``: exactly ``max_iter`` iterations, no host read (``sizes`` empty: one mesh) -- once the pattern
    has been validated: the first call with given ``rowptr`` / ``col`` tensors reads their range back, so make it outside a graph capture."""
    return ops.implicit_solve(rowptr, col, val, mass, time, rhs, list(sizes) if sizes else None, x0=x0, rtol=rtol, max_iter=max_iter, check=False)


@implicit_solve.register_fake
def _(rowptr, col, val, mass, time, rhs, sizes, x0, rtol, max_iter):
    return rhs.new_empty(rhs.shape, dtype=torch.float32)


@_op("diffusion_net::implicit_solve_bwd")
def implicit_solve_bwd(d_x: Tensor, x: Tensor, rowptr: Tensor, col: Tensor, val: Tensor, mass: Tensor, time: Tensor, sizes: List[int], rtol: float,
                       max_iter: int) -> Tuple[Tensor, Tensor]:
    """-> (d_rhs, d_time): g = A^-1 d_x by the same solver, d_rhs = m g, d_time[c] = - sum_b g_bc . (L_b x_bc)."""
    op = _implicit_op(rowptr, col, val, mass, sizes)
    d_u, _, d_t = ops._implicit_run(ops._implicit_block("d_x", d_x, op, x.shape[1]), ops._implicit_time(time, op, x.shape[1]), None,
                                    ops._implicit_block("x", x, op), op, False, *ops._implicit_settings(rtol, max_iter, 16), False)
    return d_u, d_t


@implicit_solve_bwd.register_fake
def _(d_x, x, rowptr, col, val, mass, time, sizes, rtol, max_iter):
    return torch.empty_like(x), time.new_empty(time.shape, dtype=torch.float32)


def _implicit_setup(ctx, inputs, output):
    rowptr, col, val, mass, time, rhs, sizes, x0, rtol, max_iter = inputs
    if mass.requires_grad or val.requires_grad:
        raise RuntimeError("implicit_solve has no gradient for mass or L")
    ctx.sizes, ctx.rtol, ctx.max_iter = sizes, rtol, max_iter
    ctx.save_for_backward(output, rowptr, col, val, mass, time)


def _implicit_backward(ctx, g):
    x, rowptr, col, val, mass, time = ctx.saved_tensors
    d_u, d_t = implicit_solve_bwd(g.contiguous(), x, rowptr, col, val, mass, time, ctx.sizes, ctx.rtol, ctx.max_iter)
    return None, None, None, None, d_t, d_u, None, None, None, None        # (x0 is only where the iteration starts)


implicit_solve.register_autograd(_implicit_backward, setup_context=_implicit_setup)

"""The input projection's GroupNorm written straight into the token pyramid on the MI355X (``csrc/group_norm_tokens.hip``).

For each pyramid level the head runs ``nn.Sequential(Conv2d, GroupNorm(32, 256))`` (dino_detr_ssod_head.py:251-259,
dino_detr_head.py:223-231); the transformer then does ``src.flatten(2).transpose(1, 2)``, ``torch.cat(src_flatten, 1)`` and
``src + pos`` in front of encoder layer 0 (detr_od/models/utils/transformer.py:1276-1287, 635).  Here the convs stay torch
modules and everything behind them is one op: two launches forward for the whole pyramid (statistics; normalise + transpose into
complete 256-channel token rows, optionally also ``q = tokens + pos``), three backward (two where no ``GroupNorm`` parameter
needs a gradient), on the current stream, no host synchronisation, bitwise reproducible.

``group_norm_to_tokens(feats, norms, pos=None)`` is the op on a list of NCHW tensors and their ``nn.GroupNorm`` modules;
``project_pyramid(input_proj, mlvl_feats, num_feature_levels, pos=None)`` mirrors dino_detr_ssod_head.py:359-377 for ``srcs``;
``add_norm.encoder_forward(..., query=q)`` hands the ``q`` written here to layer 0.

Dtypes.  ``x`` is fp32, fp16 or bf16 and is read in place (no fp32 copy under autocast, where ``group_norm`` is on the fp32 list:
the kernels up-cast exactly while loading).  The tokens have the dtype stock torch gives ``GroupNorm``: fp32 for fp32 input or
under enabled CUDA autocast, ``x``'s dtype in a ``.half()`` / ``.bfloat16()`` module; ``q`` has the tokens' dtype (``pos`` may
be any of the three).  Arithmetic is fp32; a 16-bit result is rounded once.  Every gradient has the dtype of its tensor; the
gradient of ``pos`` is the upstream gradient of ``q`` itself where their dtypes agree.

Layout.  A level is read in place where every image is a contiguous ``(256, H, W)`` block (the batch stride is free, so a batch
slice is read in place); anything else -- channels_last, a spatial slice -- is made contiguous first, with bit-identical results.

Not built: other group or channel counts, ``affine=False``, channels_last read in place, folding the
conv bias into the norm.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

CHANNELS, GROUPS, MAX_LEVELS = 256, 32, _lib.GN_MAX_LEVELS
# csrc/group_norm_tokens.hip: kChunk (elements of a group per statistics workgroup), kTile (pixels of a transpose tile),
# kUnit (pixels of one backward slot), kSlot (floats of a slot)
CHUNK, TILE, UNIT, SLOT = 8192, 64, 128, 2 * CHANNELS + 2 * GROUPS
_F32 = torch.float32
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _why_not(norm):
    """Why a module cannot go through the fused op, or ``None``."""
    if not isinstance(norm, nn.GroupNorm):
        return f"{type(norm).__name__} is not nn.GroupNorm"
    if norm.num_channels != CHANNELS:
        return f"{norm.num_channels} channels (only {CHANNELS} is built)"
    if norm.num_groups != GROUPS:
        return f"{norm.num_groups} groups (only {GROUPS} is built)"
    if not norm.affine or norm.weight is None or norm.bias is None:
        return "no affine parameters (affine=False is not built)"
    return None


def pyramid_index(shapes, device):
    """``spatial_shapes`` and ``level_start_index`` of the levels' ``(H, W)``, as transformer.py:1290-1291 builds them -- on the
    host, then two pinned asynchronous copies: ``torch.as_tensor(list, device=...)`` would drain the stream on every call."""
    spatial_shapes = torch.as_tensor([tuple(int(v) for v in s) for s in shapes], dtype=torch.long)
    level_start_index = torch.cat((spatial_shapes.new_zeros((1, )), spatial_shapes.prod(1).cumsum(0)[:-1]))
    device = torch.device(device)
    if device.type != "cuda":
        return spatial_shapes.to(device), level_start_index.to(device)
    return (spatial_shapes.pin_memory().to(device, non_blocking=True), level_start_index.pin_memory().to(device, non_blocking=True))


def _planes(x):
    """A level as the kernels read it: detached, every image a contiguous (256, H, W) block that starts 16-byte (fp32) or 8-byte
    (16-bit) aligned, batch stride a non-negative multiple of 4 elements; copied only where it is not."""
    x = x.detach()
    stride0 = x.stride(0) if x.shape[0] > 1 else 0
    if not x[0].is_contiguous() or x.data_ptr() % (16 if x.dtype == _F32 else 8) or stride0 % 4 or stride0 < 0:
        x = x.contiguous()
    return x


def _vector(t):
    t = t.detach()
    if t.dtype != _F32:
        t = t.float()
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(xs, weights, biases, pos, rows, start):
    if not 1 <= len(xs) <= MAX_LEVELS:
        raise NotImplementedError(f"group_norm_tokens: {len(xs)} levels (1 .. {MAX_LEVELS})")
    if len(weights) != len(xs) or (biases is not None and len(biases) != len(xs)):
        raise ValueError("group_norm_tokens: one weight and one bias per level")
    x0 = xs[0]
    for l, x in enumerate(xs):
        if x.dim() != 4 or x.shape[1] != CHANNELS:
            raise NotImplementedError(f"group_norm_tokens: level {l} is {tuple(x.shape)}; (N, {CHANNELS}, H, W) is built")
        if not x.is_cuda:
            raise RuntimeError(f"group_norm_tokens: level {l} must live on the GPU (no CPU fallback)")
        if x.dtype not in _DTYPES:
            raise NotImplementedError(f"group_norm_tokens: level {l} is {x.dtype}; float32, float16 and bfloat16 are built")
        if x.shape[0] != x0.shape[0] or x.dtype != x0.dtype or x.device != x0.device or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
            raise ValueError(f"group_norm_tokens: level {l} is {tuple(x.shape)} {x.dtype} on {x.device}; the levels share a "
                             f"non-empty batch, the dtype and the device (level 0: {tuple(x0.shape)} {x0.dtype} on {x0.device})")
        for t, what in ((weights[l], "weight"),) + (((biases[l], "bias"),) if biases is not None else ()):
            if tuple(t.shape) != (CHANNELS,) or t.device != x0.device:
                raise ValueError(f"group_norm_tokens: {what} of level {l} must be ({CHANNELS},) on {x0.device}")
    need = start + sum(x.shape[2] * x.shape[3] for x in xs)
    if rows < need:
        raise ValueError(f"group_norm_tokens: {rows} token rows per image, the levels need {need}")
    if pos is not None:
        if tuple(pos.shape) != (x0.shape[0], rows, CHANNELS) or pos.device != x0.device or pos.dtype not in _DTYPES:
            raise ValueError(f"group_norm_tokens: pos is {tuple(pos.shape)} {pos.dtype}; expected {(x0.shape[0], rows, CHANNELS)} "
                             "of float32, float16 or bfloat16 on the levels' device")
    if x0.shape[0] * rows * CHANNELS >= 2 ** 31:
        raise ValueError("group_norm_tokens: too large (batch * rows * 256 < 2^31)")


def _block(xs, weights, eps, rows, start):
    """The parameter block with the level table: sizes, ``x``, ``weight`` and the rows of each level from row ``start`` on.
    Returns the block and the tensors whose pointers it holds."""
    p = _lib.GnTokens()
    p.batch, p.levels, p.channels, p.groups, p.eps, p.tokens_per_image = xs[0].shape[0], len(xs), CHANNELS, GROUPS, eps, rows
    p.x_type = _lib.row_type(xs[0].dtype)
    keep = []
    for l, x in enumerate(xs):
        xr, w = _planes(x), _vector(weights[l])
        keep += [xr, w]
        p.hw[l], p.start[l] = x.shape[2] * x.shape[3], start
        start += p.hw[l]
        p.x[l], p.x_batch_stride[l], p.weight[l] = xr.data_ptr(), xr.stride(0) if xr.shape[0] > 1 else 0, w.data_ptr()
    return p, keep


def _workspace(p, backward, dev):
    nbytes = _lib.lib().semidetr_gn_tokens_workspace_bytes(ctypes.byref(p), int(backward))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def out_dtype(x_dtype):
    """The dtype stock torch gives ``GroupNorm`` of an ``x_dtype`` input in the caller's autocast state."""
    if x_dtype != _F32 and torch.is_autocast_enabled("cuda"):
        return _F32
    return x_dtype


def group_norm_tokens_forward(xs, weights, biases, eps=1e-5, pos=None, dtype=None, out=None, start=0, rows=None):
    """The two forward launches alone, without autograd: ``(tokens, q, mean, rstd)``.  ``xs``: the levels ``(N, 256, H, W)``;
    ``tokens`` and ``q`` are contiguous ``(N, rows, 256)`` (``q`` is ``None`` without ``pos``) of ``dtype`` (fp32, or the levels'
    16-bit dtype; default fp32), ``mean`` and ``rstd`` fp32 ``(N, levels, 32)``.  The levels fill the rows from ``start`` on;
    ``rows`` defaults to what they need.  ``out = (tokens, q)``: write into these tensors instead of new ones."""
    need = start + sum(x.shape[2] * x.shape[3] for x in xs if x.dim() == 4)
    rows = need if rows is None else rows
    _check(xs, weights, biases, pos, rows, start)
    return _forward(xs, weights, biases, float(eps), pos, dtype or _F32, out, start, rows)


def _forward(xs, weights, biases, eps, pos, dtype, out, start, rows):
    dev, n = xs[0].device, xs[0].shape[0]
    if out is None:
        tokens = torch.empty((n, rows, CHANNELS), dtype=dtype, device=dev)
        q = torch.empty((n, rows, CHANNELS), dtype=dtype, device=dev) if pos is not None else None
    else:
        tokens, q = out
    mean = torch.empty((n, len(xs), GROUPS), dtype=_F32, device=dev)
    rstd = torch.empty((n, len(xs), GROUPS), dtype=_F32, device=dev)
    p, keep = _block(xs, weights, eps, rows, start)
    for l, b in enumerate(biases):
        b = _vector(b)
        keep.append(b)
        p.bias[l] = b.data_ptr()
    p.tokens, p.mean, p.rstd, p.out_type = tokens.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _lib.row_type(tokens.dtype)
    if pos is not None:
        pr = _lib.rows_native(pos)
        _lib.set_rows(p, "pos", pr)
        p.q, p.pos_type = q.data_ptr(), _lib.row_type(pr.dtype)
    work, nbytes = _workspace(p, False, dev)
    _lib.call("semidetr_gn_tokens_forward", dev, ctypes.byref(p), work, nbytes)
    return tokens, q, mean, rstd


def group_norm_tokens_backward(gy, gq, xs, weights, mean, rstd, need_weight=True, need_bias=True, start=0):
    """The backward launches alone: ``(dxs, dweights, dbiases)`` from the upstream gradients of ``tokens`` and ``q`` (either may
    be ``None``; ``(N, rows, 256)`` of the tokens' dtype) and what the forward saved.  ``dxs[l]`` is contiguous in the shape and
    dtype of ``xs[l]``; ``dweights[l]`` / ``dbiases[l]`` are fp32, ``None`` where ``need_weight`` / ``need_bias`` (a bool, or one
    per level) says so."""
    g = gy if gy is not None else gq
    _check(xs, weights, None, None, g.shape[1], start)
    dev, levels = xs[0].device, len(xs)
    nw = [need_weight] * levels if isinstance(need_weight, bool) else list(need_weight)
    nb = [need_bias] * levels if isinstance(need_bias, bool) else list(need_bias)
    p, keep = _block(xs, weights, 0.0, g.shape[1], start)
    p.mean, p.rstd, p.out_type = mean.data_ptr(), rstd.data_ptr(), _lib.row_type(g.dtype)
    for name, t in (("gy", gy), ("gq", gq)):
        if t is not None:
            if t.dtype != g.dtype or t.shape != g.shape:
                raise ValueError("group_norm_tokens_backward: gy and gq share the shape and the dtype")
            tr = _lib.rows_native(t)
            keep.append(tr)
            _lib.set_rows(p, name, tr)
    dxs = [torch.empty(x.shape, dtype=x.dtype, device=dev) for x in xs]
    dws = [torch.empty((CHANNELS,), dtype=_F32, device=dev) if w else None for w in nw]
    dbs = [torch.empty((CHANNELS,), dtype=_F32, device=dev) if b else None for b in nb]
    for l in range(levels):
        p.grad_x[l] = dxs[l].data_ptr()
        p.grad_weight[l] = None if dws[l] is None else dws[l].data_ptr()
        p.grad_bias[l] = None if dbs[l] is None else dbs[l].data_ptr()
    work, nbytes = _workspace(p, True, dev)
    _lib.call("semidetr_gn_tokens_backward", dev, ctypes.byref(p), work, nbytes)
    return dxs, dws, dbs


class GroupNormTokensFunction(torch.autograd.Function):
    """``apply(eps, pos, tokens, q, start, rows, levels, *xs, *weights, *biases)`` -> ``tokens``, or ``(tokens, q)`` where ``pos``
    is a tensor.  ``tokens`` / ``q`` given: the levels are written into the rows from ``start`` on of these tensors, which an
    earlier call allocated with room for them (their other rows are left alone), and the tensors come back as the results, so
    that a level computed from an earlier level's rows joins the same pyramid; the gradient of ``pos`` then belongs to the call
    that allocated.  That write is deliberately not marked dirty (a view of other rows, saved by the conv in between, must pass
    autograd's version check): the rows must be ones nothing has read yet (``group_norm_to_tokens``' docstring)."""

    @staticmethod
    def forward(ctx, eps, pos, tokens, q, start, rows, levels, *rest):
        xs, weights, biases = rest[:levels], rest[levels:2 * levels], rest[2 * levels:]
        first = tokens is None
        dtype = out_dtype(xs[0].dtype) if first else tokens.dtype
        out = None if first else (tokens, q)
        tokens_out, q_out, mean, rstd = _forward(xs, weights, biases, eps, pos, dtype, out, start, rows)
        ctx.save_for_backward(mean, rstd, *xs, *weights)
        ctx.set_materialize_grads(False)
        ctx.levels, ctx.start, ctx.first = levels, start, first
        ctx.dtypes = [t.dtype for t in weights] + [t.dtype for t in biases] + [None if pos is None else pos.dtype]
        return tokens_out if pos is None else (tokens_out, q_out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gq=None):
        levels, need = ctx.levels, ctx.needs_input_grad
        mean, rstd = ctx.saved_tensors[:2]
        xs, weights = ctx.saved_tensors[2:2 + levels], ctx.saved_tensors[2 + levels:]
        none = (None,) * (7 + 3 * levels)
        if gy is None and gq is None:
            return none
        gpos = _lib.cast(gq, ctx.dtypes[-1]) if ctx.first and need[1] and gq is not None else None
        through = (None, gpos, None if ctx.first else gy, None if ctx.first else gq, None, None, None)
        if not any(need[7:]):
            return through + none[7:]
        nw, nb = list(need[7 + levels:7 + 2 * levels]), list(need[7 + 2 * levels:])
        dxs, dws, dbs = group_norm_tokens_backward(gy, gq, xs, weights, mean, rstd, nw, nb, ctx.start)
        dxs = [d if n else None for d, n in zip(dxs, need[7:7 + levels])]
        dws = [_lib.cast(d, t) for d, t in zip(dws, ctx.dtypes[:levels])]
        dbs = [_lib.cast(d, t) for d, t in zip(dbs, ctx.dtypes[levels:2 * levels])]
        return through + tuple(dxs) + tuple(dws) + tuple(dbs)


def group_norm_to_tokens(feats, norms, pos=None, into=None, start=0, rows=None):
    """``GroupNorm`` of every level, flattened, transposed and concatenated: ``feats`` is a list of ``(N, 256, H, W)`` tensors,
    ``norms`` the list of their ``nn.GroupNorm(32, 256)``.  Returns ``(tokens, spatial_shapes, level_start_index)``, or with
    ``pos`` of ``(N, S, 256)`` ``((tokens, tokens + pos), spatial_shapes, level_start_index)``; ``tokens`` is ``(N, S, 256)`` with
    the rows in the reference's ``cat`` order.  ``rows`` > S leaves room behind the levels for a later call, which passes what
    this one returned as ``into`` (``tokens``, or ``(tokens, q)``) and its first row as ``start``.

    ``into`` is what ``project_pyramid`` needs for a level that is computed from an earlier level's rows, and it comes with a
    duty.  The call writes rows ``[start, start + sum H W)`` of the given tensors in place WITHOUT telling autograd (no
    ``mark_dirty``, no version bump): that is what lets a conv that saved a view of OTHER rows of ``tokens`` still run its
    backward.  So those rows must be rows no earlier call wrote and nothing has read or saved -- the room a previous call left
    with ``rows`` -- or the gradients of whatever saved them are silently wrong; autograd cannot notice.  Rows that overlap an
    earlier call's, or a tensor that did not come from this function, are the caller's error."""
    feats, norms = list(feats), list(norms)
    if len(feats) != len(norms):
        raise ValueError(f"group_norm_to_tokens: {len(feats)} levels, {len(norms)} norms")
    for l, norm in enumerate(norms):
        reason = _why_not(norm)
        if reason:
            raise NotImplementedError(f"group_norm_to_tokens: level {l}: {reason}")
    if len({float(norm.eps) for norm in norms}) > 1:
        raise NotImplementedError(f"group_norm_to_tokens: the norms differ in eps ({[norm.eps for norm in norms]}); one per call is built")
    weights, biases = [norm.weight for norm in norms], [norm.bias for norm in norms]
    need = start + sum(x.shape[2] * x.shape[3] for x in feats if x.dim() == 4)
    rows = (need if into is None else (into[0] if isinstance(into, tuple) else into).shape[1]) if rows is None else rows
    _check(feats, weights, biases, pos, rows, start)
    tokens, q = (None, None) if into is None else into if isinstance(into, tuple) else (into, None)
    if into is not None and (q is None) != (pos is None):
        raise ValueError("group_norm_to_tokens: `into` holds q exactly where pos is given")
    out = GroupNormTokensFunction.apply(float(norms[0].eps), pos, tokens, q, start, rows, len(feats), *feats, *weights, *biases)
    spatial_shapes, level_start_index = pyramid_index([x.shape[2:] for x in feats], feats[0].device)
    return out, spatial_shapes, level_start_index


def nchw_view(tokens, start, shape):
    """Level rows ``[start, start + H * W)`` of ``tokens`` as a strided ``(N, 256, H, W)`` view: what the reference's ``srcs[l]``
    holds, without a copy."""
    h, w = int(shape[0]), int(shape[1])
    return tokens[:, start:start + h * w].transpose(1, 2).unflatten(2, (h, w))


def _conv_shape(conv, shape):
    def one(size, k):
        return (size + 2 * conv.padding[k] - conv.dilation[k] * (conv.kernel_size[k] - 1) - 1) // conv.stride[k] + 1
    return one(shape[0], 0), one(shape[1], 1)


def project_pyramid(input_proj, mlvl_feats, num_feature_levels, pos=None):
    """``srcs`` of dino_detr_ssod_head.py:359-377 as tokens.  ``input_proj`` is the head's ``ModuleList`` of
    ``Sequential(Conv2d, GroupNorm(32, 256))``; the convs run as torch modules, the norms of the backbone levels and of the first
    extra level (which reads ``mlvl_feats[-1]``) in one fused call.  Every further extra level chains on ``srcs[-1]``: it reads
    that level as the strided NCHW view of its token rows, so autograd adds its gradient into the tokens' gradient, and its norm
    runs in a fused call of its own that writes its rows into the same tensors.  ``pos``: ``(N, S, 256)`` for ALL levels.
    Returns ``(tokens, q, spatial_shapes, level_start_index, srcs)``: ``q`` is ``tokens + pos`` (``None`` without ``pos``) and
    ``srcs`` the per-level NCHW views of ``tokens`` for a caller that keeps the reference's ``transformer(srcs, ...)``."""
    mlvl_feats = list(mlvl_feats)
    convs = [input_proj[l][0](feat) for l, feat in enumerate(mlvl_feats)]
    if num_feature_levels > len(convs):
        convs.append(input_proj[len(convs)][0](mlvl_feats[-1]))
    shapes = [tuple(c.shape[2:]) for c in convs]
    for l in range(len(convs), num_feature_levels):
        shapes.append(_conv_shape(input_proj[l][0], shapes[-1]))
    starts = [0]
    for h, w in shapes:
        starts.append(starts[-1] + h * w)
    rows = starts[-1]
    out, _, _ = group_norm_to_tokens(convs, [input_proj[l][1] for l in range(len(convs))], pos, rows=rows)
    for l in range(len(convs), num_feature_levels):
        tokens = out[0] if pos is not None else out
        src = input_proj[l][0](nchw_view(tokens, starts[l - 1], shapes[l - 1]))
        if tuple(src.shape[2:]) != shapes[l]:
            raise RuntimeError(f"project_pyramid: level {l} is {tuple(src.shape[2:])}, planned {shapes[l]}")
        out, _, _ = group_norm_to_tokens([src], [input_proj[l][1]], pos, into=out, start=starts[l])
    tokens, q = out if pos is not None else (out, None)
    spatial_shapes, level_start_index = pyramid_index(shapes, tokens.device)
    srcs = [nchw_view(tokens, starts[l], shapes[l]) for l in range(num_feature_levels)]
    return tokens, q, spatial_shapes, level_start_index, srcs

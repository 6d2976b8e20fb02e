"""Residual add + LayerNorm + positional add on the MI355X (``csrc/add_norm.hip``): the end of every sub-block of the DINO
transformer, ``x = x + dropout(branch); x = norm(x)`` (detr_od/models/utils/transformer.py:628-629, 636-637, 789-790, 811-812,
838-839), and the ``with_pos_embed(x, pos)`` that opens the next one.

``add_layer_norm(x, residual, weight, bias, eps=1e-5, pos=None)`` is ``layer_norm(x + residual)`` and, with ``pos``, also
``layer_norm(x + residual) + pos``: one launch forward, two backward (one where neither ``weight`` nor ``bias`` needs a
gradient), on the current stream, with no host synchronisation and no ``.item()``.  The sum ``x + residual`` never reaches
memory: the op saves ``x``, ``residual``, ``weight`` and the per-row ``mean`` and ``rstd``.  ``x``, ``residual``, ``pos`` and the
upstream gradients are read through the strides of their two leading dimensions (last stride 1, fp32 rows 16-byte and 16-bit
rows 8-byte aligned, copied only where they are not: ``_lib.rows_native``), so the decoder's ``(nq, bs, 256)`` views and
transposes are read in place.  The gradient of ``residual`` is the tensor returned for ``x`` where their dtypes agree, and the
gradient of ``pos`` is the upstream gradient of the second output itself where theirs do.

``LayerNorm`` is the drop-in for ``nn.LayerNorm(256)`` (``weight`` / ``bias`` under the same names, so a reference
``state_dict`` loads with ``strict=True``); ``convert_layer_norms(module)`` replaces the qualifying children of a built model in
place, adopting their ``Parameter`` objects.  ``encoder_layer_forward``, ``encoder_forward`` and ``decoder_layer_forward*``
re-state the reference's layer control flow with the fused epilogue; ``registry.bind_layer_epilogues()`` binds them.

Dtypes.  ``x``, ``residual``, ``pos``, ``weight`` and ``bias`` may each be fp32, fp16 or bf16, in any mixture; every one is
up-cast exactly, the arithmetic is fp32, and each result is rounded once on its way out (``q`` from the unrounded ``y``).  The
rows are read and written in their own dtypes INSIDE the kernels (``semidetr_add_norm_*_mixed``; an all-fp32 call keeps the
``*_f32`` entry points): every result is allocated in its final dtype, the 16-bit tensors that were saved are what the backward
reads, and where ``x`` and ``residual`` differ in dtype the one ``dx`` of the backward launch leaves in both.  No cast pass
touches a ``(rows, 256)`` tensor; only the 256-element parameter vectors and their gradients are converted by torch.  What
comes back has the dtype stock torch gives ``F.layer_norm(x + residual, ...)`` and ``... + pos`` in the caller's autocast state:
under enabled CUDA autocast ``y`` and ``q`` are fp32 whatever came in (``layer_norm`` is on autocast's fp32 list), so the fp32
residual stream of a layer stays fp32 although the branch added to it is 16-bit; outside autocast ``y`` has the promoted type of
``x`` and ``residual`` and ``q`` that of ``y`` and ``pos`` (a ``.half()`` module: all fp16; the parameters' dtype plays no part).
Every gradient has the dtype of the tensor it belongs to.

Not built: widths other than 256, rows of other dtypes than fp32 / fp16 / bf16, ``normalize_before``,
fusing ``norm3`` with the decoder's final ``norm``, the bias of ``linear2`` / ``out_proj``.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib

DIM = 256
_Params = _lib.AddNorm
_F32 = torch.float32
_ROW_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _rows3(t):
    """A ``(..., 256)`` tensor as ``(rows0, rows1, 256)`` for the kernels, in its own dtype (``_lib.rows_native``); ``None``
    stays ``None``."""
    if t is None:
        return None
    if t.dim() == 2:
        t = t.unsqueeze(0)
    elif t.dim() != 3:
        t = t.reshape(1, -1, t.shape[-1])
    return _lib.rows_native(t)


def _vector(t):
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _check(x, residual, weight, bias, pos):
    if x.dim() < 1 or x.shape[-1] != DIM:
        raise NotImplementedError(f"add_layer_norm: row width {x.shape[-1] if x.dim() else 'of a scalar'}; only {DIM} is built")
    if tuple(weight.shape) != (DIM,) or tuple(bias.shape) != (DIM,):
        raise ValueError(f"add_layer_norm: weight {tuple(weight.shape)} and bias {tuple(bias.shape)} must be ({DIM},)")
    for t, what in ((residual, "residual"), (pos, "pos")):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"add_layer_norm: {what} is {tuple(t.shape)}, x is {tuple(x.shape)}")
    for t, what in ((x, "x"), (residual, "residual"), (weight, "weight"), (bias, "bias"), (pos, "pos")):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"add_layer_norm: {what} must live on the GPU (no CPU fallback)")
    for t, what in ((x, "x"), (residual, "residual"), (pos, "pos")):
        if t is not None and t.dtype not in _ROW_DTYPES:
            raise NotImplementedError(f"add_layer_norm: {what} is {t.dtype}; rows of float32, float16 and bfloat16 are built")
    if x.numel() // DIM >= 2 ** 31:
        raise ValueError("add_layer_norm: too many rows (rows < 2^31)")


def _result_dtypes(x, residual, pos):
    """The dtypes of ``y`` and ``q`` from those of ``x``, ``residual`` and ``pos`` (``None`` where absent): what stock torch
    returns for ``layer_norm(x + residual)`` and for that ``+ pos`` in the caller's autocast state.  The sum has the promoted
    type of its operands; under enabled CUDA autocast ``layer_norm`` is on the fp32 list, so a 16-bit sum still gives an
    fp32 ``y``; ``q`` has the promoted type of ``y`` and ``pos``.  Both are computed in fp32 from the up-cast operands and
    rounded once, ``q`` from the unrounded ``y``."""
    if x == torch.float32 and residual in (None, x) and pos in (None, x):
        return x, x
    y = x if residual is None else torch.promote_types(x, residual)
    if y in (torch.float16, torch.bfloat16) and torch.is_autocast_enabled("cuda"):
        y = torch.float32
    return y, y if pos is None else torch.promote_types(y, pos)


def _all_f32(*tensors_and_dtypes):
    """whether every tensor / dtype given (``None``: absent) is fp32: the call goes to the ``*_f32`` entry points"""
    return all(t is None or (t if isinstance(t, torch.dtype) else t.dtype) == _F32 for t in tensors_and_dtypes)


def _block(xr, eps, operands, mixed):
    """The parameter block of a launch -- ``semidetr_add_norm``, or ``semidetr_add_norm_mixed`` with the type code of every
    operand -- with sizes, ``eps`` and the row operands ``{name: (rows0, rows1, 256) tensor or None}`` set."""
    p = _lib.AddNormMixed() if mixed else _Params()
    p.rows0, p.rows1, p.dim, p.eps = xr.shape[0], xr.shape[1], DIM, eps
    for name, t in operands.items():
        _lib.set_rows(p, name, t)
        if mixed and t is not None:
            setattr(p, name + "_type", _lib.row_type(t.dtype))
    return p


def _set_results(p, results, mixed):
    """``results``: {name: contiguous result tensor or None}, each with its type code where the block is the mixed one"""
    for name, t in results.items():
        if t is not None:
            setattr(p, name, t.data_ptr())
            if mixed:
                setattr(p, name + "_type", _lib.row_type(t.dtype))


def add_layer_norm_forward(x, residual, weight, bias, eps=1e-5, pos=None, dtypes=(_F32, _F32)):
    """The forward launch alone, without autograd: ``(y, q, mean, rstd)``; ``y`` and ``q`` contiguous in the shape of ``x``
    (``q`` is ``None`` without ``pos``) and in fp32 unless ``dtypes = (dtype of y, dtype of q)`` asks for fp16 or bf16 (rounded
    once by the kernel); ``mean`` and ``rstd`` fp32 of ``rows`` elements."""
    _check(x, residual, weight, bias, pos)
    return _forward(x, residual, weight, bias, eps, pos, dtypes)


def _forward(x, residual, weight, bias, eps, pos, dtypes):
    dev = x.device
    rows = x.numel() // DIM
    y = torch.empty(x.shape, dtype=dtypes[0], device=dev)
    q = torch.empty(x.shape, dtype=dtypes[1], device=dev) if pos is not None else None
    mean = torch.empty((rows,), dtype=torch.float32, device=dev)
    rstd = torch.empty((rows,), dtype=torch.float32, device=dev)
    if rows == 0:
        return y, q, mean, rstd
    xr, rr, pr, w, b = _rows3(x), _rows3(residual), _rows3(pos), _vector(weight), _vector(bias)
    mixed = not _all_f32(xr, rr, pr, y, q)
    p = _block(xr, eps, dict(x=xr, residual=rr, pos=pr), mixed)
    p.weight, p.bias, p.mean, p.rstd = w.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    _set_results(p, dict(y=y, q=q), mixed)
    _lib.call("semidetr_add_norm_forward_mixed" if mixed else "semidetr_add_norm_forward_f32", dev, ctypes.byref(p), None, 0)
    return y, q, mean, rstd


def add_layer_norm_backward(gy, gq, x, residual, weight, mean, rstd, need_weight=True, need_bias=True, dtype=_F32):
    """The backward launches alone: ``(dx, dweight, dbias)`` from the upstream gradients of ``y`` and ``q`` (either may be
    ``None``) and what the forward saved; ``dx`` in fp32 unless ``dtype`` asks for fp16 or bf16 (rounded once by the kernel),
    ``dweight`` / ``dbias`` fp32, ``None`` where not needed."""
    dx, _, _, dw, db = _backward(gy, gq, x, residual, weight, mean, rstd, need_weight, need_bias, dtype, None, None)
    return dx, dw, db


def _backward(gy, gq, x, residual, weight, mean, rstd, need_weight, need_bias, x_dtype, residual_dtype, pos_dtype):
    """One call of the backward entry point: ``(grad_x, grad_residual, grad_pos, dweight, dbias)``.  The one fp32 ``dx`` leaves
    as ``grad_x`` in ``x_dtype`` and / or as ``grad_residual`` in ``residual_dtype``, ``gq`` as ``grad_pos`` in ``pos_dtype``;
    ``None``: not wanted (``x_dtype`` and ``residual_dtype`` not both)."""
    dev = x.device
    xr, rr, gyr, gqr, w = _rows3(x), _rows3(residual), _rows3(gy), _rows3(gq), _vector(weight)
    rows = xr.shape[0] * xr.shape[1]
    gx, gres, gpos = (None if d is None else torch.empty(x.shape, dtype=d, device=dev) for d in (x_dtype, residual_dtype, pos_dtype))
    dw = torch.empty((DIM,), dtype=torch.float32, device=dev) if need_weight else None
    db = torch.empty((DIM,), dtype=torch.float32, device=dev) if need_bias else None
    mixed = not (_all_f32(xr, rr, gyr, gqr, gx) and gres is None and gpos is None)
    p = _block(xr, 0.0, dict(x=xr, residual=rr, gy=gyr, gq=gqr), mixed)
    p.weight, p.mean, p.rstd = w.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    _set_results(p, dict(grad_x=gx, grad_residual=gres, grad_pos=gpos) if mixed else dict(grad_x=gx), mixed)
    work, nbytes = None, 0
    if need_weight or need_bias:
        p.grad_weight = dw.data_ptr() if need_weight else None
        p.grad_bias = db.data_ptr() if need_bias else None
        nbytes = _lib.lib().semidetr_add_norm_workspace_bytes(rows)
        work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.call("semidetr_add_norm_backward_mixed" if mixed else "semidetr_add_norm_backward_f32", dev, ctypes.byref(p), work, nbytes)
    return gx, gres, gpos, dw, db


class AddLayerNormFunction(torch.autograd.Function):
    """``apply(x, residual, weight, bias, eps, pos)`` -> ``y``, or ``(y, y + pos)`` where ``pos`` is a tensor."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, pos):
        dtypes = (x.dtype, None if residual is None else residual.dtype, weight.dtype, bias.dtype,
                  None if pos is None else pos.dtype)
        # add_layer_norm has checked the arguments; every result is allocated in, and written by the kernel in, its final dtype
        y, q, mean, rstd = _forward(x, residual, weight, bias, eps, pos, _result_dtypes(*dtypes[:2], dtypes[4]))
        ctx.save_for_backward(x, residual, weight, mean, rstd)
        ctx.set_materialize_grads(False)
        ctx.dtypes = dtypes
        return y if pos is None else (y, q)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gq=None):
        x, residual, weight, mean, rstd = ctx.saved_tensors
        need, dt = ctx.needs_input_grad, ctx.dtypes
        if gy is None and gq is None:
            return (None,) * 6
        want_pos = need[5] and gq is not None
        if not any(need[:4]) or x.numel() == 0:
            gpos = _lib.cast(gq, dt[4]) if want_pos else None            # no launch for the gradient of pos alone
        if not any(need[:4]):
            return None, None, None, None, None, gpos
        want_res = residual is not None and need[1]
        if x.numel() == 0:                   # no rows, no launch: empty dx, zero sums
            gx = torch.empty(x.shape, dtype=dt[0], device=x.device) if need[0] else None
            gres = (gx if gx is not None and dt[1] == dt[0] else torch.empty(x.shape, dtype=dt[1], device=x.device)) if want_res else None
            dw = torch.zeros((DIM,), dtype=torch.float32, device=x.device) if need[2] else None
            db = torch.zeros((DIM,), dtype=torch.float32, device=x.device) if need[3] else None
            return gx, gres, _lib.cast(dw, dt[2]), _lib.cast(db, dt[3]), None, gpos
        # dx leaves once per dtype asked for: the gradient of residual is the tensor of x's where the dtypes agree, and the
        # gradient of pos is gq itself where theirs do; a call for the parameters' gradients alone still writes x's
        both = need[0] and want_res and dt[1] != dt[0]
        gx, gres, gpos, dw, db = _backward(gy, gq, x, residual, weight, mean, rstd, need[2], need[3],
                                           dt[0] if need[0] or not want_res else dt[1], dt[1] if both else None,
                                           dt[4] if want_pos and gq.dtype != dt[4] else None)
        if want_pos and gpos is None:
            gpos = gq
        if want_res and not both:
            gres = gx
        return gx if need[0] else None, gres, _lib.cast(dw, dt[2]), _lib.cast(db, dt[3]), None, gpos


def add_layer_norm(x, residual, weight, bias, eps=1e-5, pos=None):
    """``y = layer_norm(x + residual, (256,), weight, bias, eps)``; with ``pos`` returns ``(y, y + pos)``.  ``residual`` may be
    ``None``; ``residual`` and ``pos`` have the shape of ``x`` (module docstring)."""
    _check(x, residual, weight, bias, pos)
    return AddLayerNormFunction.apply(x, residual, weight, bias, float(eps), pos)


class LayerNorm(nn.Module):
    """Drop-in for ``nn.LayerNorm(256)``: the same ``weight`` / ``bias`` parameters, ``eps``, ``normalized_shape`` and
    ``elementwise_affine`` attributes.  ``forward(x, residual=None, pos=None)`` is ``add_layer_norm``."""

    def __init__(self, normalized_shape=DIM, eps=1e-5, elementwise_affine=True):
        super().__init__()
        shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
        if shape != (DIM,):
            raise NotImplementedError(f"LayerNorm: normalized_shape {shape}; only ({DIM},) is built")
        if not elementwise_affine:
            raise NotImplementedError("LayerNorm: elementwise_affine=False is not built")
        self.normalized_shape, self.eps, self.elementwise_affine = shape, eps, True
        self.weight = nn.Parameter(torch.ones(DIM))
        self.bias = nn.Parameter(torch.zeros(DIM))

    @classmethod
    def adopt(cls, ln):
        """The mirror of a built ``nn.LayerNorm`` that holds the SAME ``Parameter`` objects."""
        reason = _why_not(ln)
        if reason:
            raise NotImplementedError(f"LayerNorm: {reason}")
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        new.normalized_shape, new.eps, new.elementwise_affine = tuple(ln.normalized_shape), ln.eps, True
        new.weight, new.bias = ln.weight, ln.bias
        new.train(ln.training)
        return new

    def forward(self, x, residual=None, pos=None):
        return add_layer_norm(x, residual, self.weight, self.bias, self.eps, pos)

    def extra_repr(self):
        return f"{self.normalized_shape}, eps={self.eps}, elementwise_affine=True"


def _why_not(ln):
    """Why a ``nn.LayerNorm`` cannot be replaced by the mirror, or ``None``."""
    if tuple(ln.normalized_shape) != (DIM,):
        return f"normalized_shape {tuple(ln.normalized_shape)}"
    if not ln.elementwise_affine or ln.weight is None or ln.bias is None:
        return "no elementwise affine (or no bias)"
    return None


def convert_layer_norms(module):
    """Replace, in place, every ``nn.LayerNorm`` below ``module`` that qualifies (``normalized_shape == (256,)``, affine) with
    ``LayerNorm.adopt`` of it: the same ``Parameter`` objects, so optimizer state, EMA pairs and ``state_dict`` keys are
    untouched.  Others are left alone.  Returns the number converted."""
    done = 0
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.LayerNorm and _why_not(child) is None:
                setattr(parent, name, LayerNorm.adopt(child))
                done += 1
    return done


# ---------------------------------------------------------------------------------------------
# the reference's layers with the fused epilogue
# ---------------------------------------------------------------------------------------------
def epilogue(norm, x, branch, dropout=None, pos=None):
    """``norm(x + dropout(branch))`` and, with ``pos``, that plus ``pos``.  A dropout with ``p > 0`` in training mode runs in
    torch on the branch first (DINOTransformer builds its layers with 0.0)."""
    if dropout is not None and dropout.p > 0.0 and dropout.training:
        branch = dropout(branch)
    return add_layer_norm(branch, x, norm.weight, norm.bias, norm.eps, pos)


def encoder_layer_forward(layer, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None,
                          query=None, want_next_query=False):
    """``DINOTransformerEncoderLayer.forward`` (transformer.py:632-642).  ``query``: ``src + pos`` where the caller already has
    it.  ``want_next_query``: return ``(src, src + pos)``, the second from the FFN epilogue, for the next layer."""
    if query is None:
        query = src if pos is None else src + pos
    src2 = layer.self_attn(query, reference_points, src, spatial_shapes, level_start_index, key_padding_mask)
    src = epilogue(layer.norm1, src, src2, layer.dropout1)
    src2 = layer.linear2(layer.dropout2(layer.activation(layer.linear1(src))))
    if want_next_query and pos is not None:
        return epilogue(layer.norm2, src, src2, layer.dropout3, pos)
    out = epilogue(layer.norm2, src, src2, layer.dropout3)
    return (out, out) if want_next_query else out


def encoder_layer_forward_ffn(layer, src):
    """``DINOTransformerEncoderLayer.forward_ffn`` (transformer.py:626-630)."""
    src2 = layer.linear2(layer.dropout2(layer.activation(layer.linear1(src))))
    return epilogue(layer.norm2, src, src2, layer.dropout3)


def encoder_forward(encoder, src, pos, spatial_shapes, level_start_index, valid_ratios, key_padding_mask,
                    ref_token_index=None, ref_token_coord=None, query=None, reference_points=None):
    """``DINOTransformerEncoder.forward`` (transformer.py:693-744): each layer's FFN epilogue also writes ``output + pos`` for
    the next layer, so the only stand-alone ``src + pos`` pass is the one in front of layer 0.  ``query``: ``src + pos`` where
    the caller already has it (``input_proj.project_pyramid`` writes it with the tokens); layer 0 then takes it and no
    stand-alone pass is left.  ``reference_points``: the ``(N, S, L, 2)`` tensor ``encoder.get_reference_points`` would return,
    where the caller already has it (``pyramid_inputs`` writes it); the call is then not made."""
    if encoder.two_stage_type != 'standard' or encoder.deformable_encoder is not True or ref_token_index is not None \
            or ref_token_coord is not None:
        raise NotImplementedError("encoder_forward: only the standard two-stage deformable encoder without reference tokens")
    output = src
    layers = list(encoder.layers)
    if layers and reference_points is None:
        reference_points = encoder.get_reference_points(spatial_shapes, valid_ratios, device=src.device)
    for i, layer in enumerate(layers):
        more = i + 1 < len(layers)
        res = encoder_layer_forward(layer, output, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask,
                                    query=query, want_next_query=more)
        output, query = res if more else (res, None)
    if encoder.norm is not None:
        output = encoder.norm(output)
    return output, None, None


def decoder_layer_forward_sa(layer, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None,
                             tgt_reference_points=None, memory=None, memory_key_padding_mask=None,
                             memory_level_start_index=None, memory_spatial_shapes=None, memory_pos=None, self_attn_mask=None,
                             cross_attn_mask=None, want_query=False):
    """``DINOTransformerDecoderLayer.forward_sa`` (transformer.py:793-816).  ``want_query``: return ``(tgt, tgt + query_pos)``,
    the second from the epilogue, for ``forward_ca``."""
    query = None
    if layer.self_attn is not None:
        if layer.decoder_sa_type != 'sa':
            raise NotImplementedError(f"decoder_layer_forward_sa: decoder_sa_type {layer.decoder_sa_type!r} (only 'sa' exists)")
        q = k = tgt if tgt_query_pos is None else tgt + tgt_query_pos
        tgt2 = layer.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]
        if want_query and tgt_query_pos is not None:
            tgt, query = epilogue(layer.norm2, tgt, tgt2, layer.dropout2, tgt_query_pos)
        else:
            tgt = epilogue(layer.norm2, tgt, tgt2, layer.dropout2)
    return (tgt, query) if want_query else tgt


def decoder_layer_forward_ca(layer, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None,
                             tgt_reference_points=None, memory=None, memory_key_padding_mask=None,
                             memory_level_start_index=None, memory_spatial_shapes=None, memory_pos=None, self_attn_mask=None,
                             cross_attn_mask=None, query=None):
    """``DINOTransformerDecoderLayer.forward_ca`` (transformer.py:818-841).  ``query``: ``tgt + tgt_query_pos`` where
    ``forward_sa``'s epilogue already wrote it."""
    if layer.key_aware_type is not None:
        raise NotImplementedError(f"decoder_layer_forward_ca: key_aware_type {layer.key_aware_type!r} (the reference has none)")
    if query is None:
        query = tgt if tgt_query_pos is None else tgt + tgt_query_pos
    tgt2 = layer.cross_attn(query.transpose(0, 1), tgt_reference_points.transpose(0, 1).contiguous(), memory.transpose(0, 1),
                            memory_spatial_shapes, memory_level_start_index, memory_key_padding_mask).transpose(0, 1)
    return epilogue(layer.norm1, tgt, tgt2, layer.dropout1)


def decoder_layer_forward_ffn(layer, tgt):
    """``DINOTransformerDecoderLayer.forward_ffn`` (transformer.py:787-791)."""
    tgt2 = layer.linear2(layer.dropout3(layer.activation(layer.linear1(tgt))))
    return epilogue(layer.norm3, tgt, tgt2, layer.dropout4)


def decoder_layer_forward(layer, tgt, tgt_query_pos=None, tgt_query_sine_embed=None, tgt_key_padding_mask=None,
                          tgt_reference_points=None, memory=None, memory_key_padding_mask=None, memory_level_start_index=None,
                          memory_spatial_shapes=None, memory_pos=None, self_attn_mask=None, cross_attn_mask=None):
    """``DINOTransformerDecoderLayer.forward`` (transformer.py:843-873): ``sa`` hands ``tgt + tgt_query_pos`` to a ``ca`` that
    follows it directly."""
    args = (tgt_query_pos, tgt_query_sine_embed, tgt_key_padding_mask, tgt_reference_points, memory, memory_key_padding_mask,
            memory_level_start_index, memory_spatial_shapes, memory_pos, self_attn_mask, cross_attn_mask)
    seq = list(layer.module_seq)
    query = None
    for i, funcname in enumerate(seq):
        if funcname == 'ffn':
            tgt, query = decoder_layer_forward_ffn(layer, tgt), None
        elif funcname == 'ca':
            tgt, query = decoder_layer_forward_ca(layer, tgt, *args, query=query), None
        elif funcname == 'sa':
            want = seq[i + 1:i + 2] == ['ca']
            res = decoder_layer_forward_sa(layer, tgt, *args, want_query=want)
            tgt, query = res if want else (res, None)
        else:
            raise ValueError(f"decoder_layer_forward: module_seq holds {funcname!r}; expected 'sa', 'ca' or 'ffn'")
    return tgt

"""The decoder's reference-point chain on the MI355X (``csrc/ref_points.hip``): sigmoid / box refinement, valid-ratio scaling
and the sine embedding of the query boxes.

Between two layers ``DINOTransformerDecoder.forward`` (detr_od/models/utils/transformer.py:947-1045) runs
``reference_points[:, :, None] * cat([valid_ratios, valid_ratios], -1)[None, :]`` (:980-984), ``gen_sineembed_for_position``
(:467-493) and the iterative update ``sigmoid(fc_reg(output) + inverse_sigmoid(reference_points))`` with its ``detach``
(:1029-1036); the head repeats the update for every layer to build ``outputs_coord`` (dino_detr_ssod_head.py:393-398,
dino_detr_head.py likewise).  In stock torch that is several dozen elementwise launches per layer.  Here it is one launch
forward and one backward, on the current stream, no host synchronisation, no workspace, bitwise reproducible:

``gen_sineembed_for_position(pos_tensor)``          the reference's function, name and contract
``refine_boxes(delta, reference, eps=1e-5)``        ``sigmoid(delta + inverse_sigmoid(reference, eps))``
``reference_inputs(reference_points, valid_ratios)``  ``(reference_points_input, query_sine_embed)``
``decoder_forward(decoder, tgt, memory, ...)``      the mirror of ``DINOTransformerDecoder.forward``
``box_outputs(fc_reg, hs, reference)``              the head's stacked ``outputs_coord`` from one segmented launch

Dtypes.  ``delta`` and ``reference`` are fp32, fp16 or bf16, read in place through the strides of their two leading dimensions
(the head's ``(bs, nq, 4)`` transposes are not copied).  Arithmetic is fp32; the refined points are rounded once to the dtype
torch's promotion gives the reference's op sequence: fp32 as soon as one operand is fp32, or the two 16-bit dtypes differ, or --
``log`` being on autocast's fp32 list -- CUDA autocast is enabled.  ``valid_ratios`` is fp32; ``reference_points_input`` and the
embedding are fp32.  Every gradient has the dtype of its tensor.  ``valid_ratios`` gets no gradient: one that requires grad is
refused.

Layout.  ``reference_points_input`` is written as contiguous ``(bs, nq, L, width)`` and returned as its ``(nq, bs, L, width)``
transpose, so the ``tgt_reference_points.transpose(0, 1).contiguous()`` of ``add_norm.decoder_layer_forward_ca`` copies nothing.

Not built: the non-deformable decoder branches (``query_pos_sine_scale``, ``modulate_hw_attn``,
``deformable_decoder=False``), ``dec_layer_dropout_prob``, ``rm_detach``, widths other than 2 and 4, more than 8 levels or
segments, the pyramid's ``SinePositionalEncodingHW``.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib, add_norm

MAX_SEGMENTS, MAX_LEVELS = _lib.REF_MAX_SEGMENTS, _lib.REF_MAX_LEVELS
NONE, SIGMOID, REFINE = (_lib.REF_MODES[k] for k in ("SEMIDETR_REF_NONE", "SEMIDETR_REF_SIGMOID", "SEMIDETR_REF_REFINE"))
BLOCK = 128                       # columns of one coordinate's block of the embedding
_F32 = torch.float32
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_tables = {}                      # device -> (dim_t, {images: valid ratios of exactly 1})


def dim_t(device):
    """The 128 divisors of the embedding, computed once per device with the reference's own expression (transformer.py:471-472);
    the kernel reads this table and evaluates no ``pow``."""
    return _table(device)[0]


def _table(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    hit = _tables.get(device)
    if hit is None:
        with torch.no_grad():
            t = torch.arange(BLOCK, dtype=_F32, device=device)
            t = 10000 ** (2 * (t // 2) / BLOCK)
            hit = _tables[device] = (t.contiguous(), {})
    return hit


def _ones(device, images):
    """Valid ratios of exactly 1 for ``images`` images and one level (``x * 1`` is ``x``): what the embedding alone runs with."""
    cache = _table(device)[1]
    if images not in cache:
        cache[images] = torch.ones((images, 1, 2), dtype=_F32, device=device)
    return cache[images]


def out_dtype(mode, delta_dtype, ref_dtype):
    """The dtype stock torch gives the refined points in the caller's autocast state."""
    if mode != REFINE:
        return ref_dtype
    if delta_dtype != ref_dtype or ref_dtype == _F32 or torch.is_autocast_enabled("cuda"):
        return _F32
    return ref_dtype


def _rows(t):
    """A ``(rows0, rows1, width)`` tensor as the kernels read it: detached, last stride 1, both leading strides non-negative;
    copied only where it is not."""
    t = t.detach()
    if t.stride(2) != 1 or t.stride(0) < 0 or t.stride(1) < 0:
        t = t.contiguous()
    return t


def _check(mode, deltas, refs, valid_ratios, what):
    if not 1 <= len(refs) <= MAX_SEGMENTS:
        raise NotImplementedError(f"{what}: {len(refs)} segments (1 .. {MAX_SEGMENTS})")
    if mode == REFINE and len(deltas) != len(refs):
        raise ValueError(f"{what}: {len(deltas)} deltas for {len(refs)} references")
    r0 = refs[0]
    if r0.dim() != 3 or r0.shape[-1] not in (2, 4):
        raise NotImplementedError(f"{what}: reference points of shape {tuple(r0.shape)}; (rows0, rows1, 2 or 4) is built")
    for s, r in enumerate(refs):
        pair = (r,) if mode != REFINE else (r, deltas[s])
        for t in pair:
            if t.dtype not in _DTYPES:
                raise NotImplementedError(f"{what}: segment {s} is {t.dtype}; float32, float16 and bfloat16 are built")
            if t.dim() != 3 or t.shape[-1] != r0.shape[-1] or t.shape != r.shape or t.numel() == 0 or t.device != r0.device:
                raise ValueError(f"{what}: segment {s} is {tuple(t.shape)} on {t.device}; delta and reference share a non-empty "
                                 f"(rows0, rows1, {r0.shape[-1]}) shape, the segments the width and the device")
        if r.dtype != r0.dtype or (mode == REFINE and deltas[s].dtype != deltas[0].dtype):
            raise ValueError(f"{what}: the segments share the dtype of delta and the dtype of reference")
        if r.shape[0] * r.shape[1] * BLOCK * r.shape[2] >= 2 ** 31:
            raise ValueError(f"{what}: segment {s} too large (rows0 * rows1 * 128 * width < 2^31)")
    if valid_ratios is not None:
        if len(refs) != 1:
            raise NotImplementedError(f"{what}: scale and embed take one segment, not {len(refs)}")
        v = valid_ratios
        if v.dim() != 3 or v.shape[0] != r0.shape[1] or v.shape[2] != 2 or v.device != r0.device:
            raise ValueError(f"{what}: valid_ratios is {tuple(v.shape)} on {v.device}; expected ({r0.shape[1]}, levels, 2) on "
                             f"{r0.device}")
        if not 1 <= v.shape[1] <= MAX_LEVELS:
            raise NotImplementedError(f"{what}: {v.shape[1]} levels (1 .. {MAX_LEVELS})")
        if v.dtype != _F32:
            raise NotImplementedError(f"{what}: valid_ratios is {v.dtype}; float32 is built")
        if v.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{what}: valid_ratios requires grad; no gradient to valid_ratios is built")
    if not r0.is_cuda:
        raise RuntimeError(f"{what}: the reference points must live on the GPU (no CPU fallback)")


def _block(mode, eps, deltas, refs, dtype, valid_ratios):
    """The parameter block with the segment table: sizes, types, ``ref`` and ``delta`` of every segment.  Returns the block and
    the tensors whose pointers it holds."""
    p = _lib.RefPoints()
    p.width, p.mode, p.num_segments, p.eps = refs[0].shape[-1], mode, len(refs), eps
    p.ref_type, p.out_type = _lib.row_type(refs[0].dtype), _lib.row_type(dtype)
    p.delta_type = _lib.row_type(deltas[0].dtype) if mode == REFINE else 0
    keep = []
    for s, r in enumerate(refs):
        sg = p.segment[s]
        sg.rows0, sg.rows1 = r.shape[0], r.shape[1]
        rr = _rows(r)
        keep.append(rr)
        _lib.set_rows(sg, "ref", rr)
        if mode == REFINE:
            dr = _rows(deltas[s])
            keep.append(dr)
            _lib.set_rows(sg, "delta", dr)
    if valid_ratios is not None:
        v = valid_ratios.detach().contiguous()
        keep.append(v)
        p.valid_ratios, p.levels = v.data_ptr(), v.shape[1]
        p.dim_t = dim_t(refs[0].device).data_ptr()
    return p, keep


def _forward(mode, deltas, refs, eps, valid_ratios, embed, dtype, stacked):
    """The forward launch: ``(new_refs, ref_input, embed)``.  ``new_refs``: one contiguous tensor of ``dtype`` per segment, or
    with ``stacked`` (equal shapes) one ``(segments, rows0, rows1, width)`` tensor; ``None`` for ``NONE``.  With ``valid_ratios``
    ``(rows1, L, 2)``: ``ref_input`` contiguous ``(rows1, rows0, L, width)`` and, with ``embed``, the ``(rows0, rows1,
    128 * width)`` embedding; both fp32."""
    dev, width = refs[0].device, refs[0].shape[-1]
    p, keep = _block(mode, eps, deltas, refs, dtype, valid_ratios)
    outs = None
    if mode != NONE:
        if stacked:
            if any(r.shape != refs[0].shape for r in refs):
                raise ValueError("ref_points: a stacked result needs segments of one shape")
            outs = torch.empty((len(refs),) + tuple(refs[0].shape), dtype=dtype, device=dev)
        else:
            outs = [torch.empty(r.shape, dtype=dtype, device=dev) for r in refs]
        for s in range(len(refs)):
            _lib.set_rows(p.segment[s], "new_ref", outs[s])
    ref_input = emb = None
    if valid_ratios is not None:
        rows0, rows1 = refs[0].shape[:2]
        ref_input = torch.empty((rows1, rows0, valid_ratios.shape[1], width), dtype=_F32, device=dev)
        p.ref_input = ref_input.data_ptr()
        if embed:
            emb = torch.empty((rows0, rows1, BLOCK * width), dtype=_F32, device=dev)
            p.embed = emb.data_ptr()
    _lib.call("semidetr_ref_points_forward", dev, ctypes.byref(p))
    return outs, ref_input, emb


def ref_points_backward(mode, deltas, refs, new_refs, g_new, eps=1e-5, valid_ratios=None, g_ref_input=None, g_embed=None,
                        need_delta=True, need_ref=True):
    """The backward launch alone: ``(g_deltas, g_refs)``, lists with one contiguous tensor per segment in the dtype of its
    operand (``None`` where not wanted, ``g_deltas`` all ``None`` outside ``REFINE``).  ``new_refs``: what the forward stored
    (ignored for ``NONE``); ``g_new``: one upstream gradient per segment or ``None``; ``g_ref_input`` ``(rows1, rows0, L, width)``
    and ``g_embed`` ``(rows0, rows1, 128 * width)``: fp32 or ``None``."""
    deltas, refs = list(deltas or ()), list(refs)
    _check(mode, deltas, refs, valid_ratios, "ref_points_backward")
    dev, n = refs[0].device, len(refs)
    g_new = [None] * n if g_new is None else list(g_new)
    dtype = refs[0].dtype if mode == NONE else new_refs[0].dtype
    with_scale = valid_ratios is not None and (g_ref_input is not None or g_embed is not None)
    p, keep = _block(mode, float(eps), deltas, refs, dtype, valid_ratios if with_scale else None)
    g_deltas, g_refs = [None] * n, [None] * n
    for s, r in enumerate(refs):
        sg = p.segment[s]
        if mode != NONE:
            y = _rows(new_refs[s])
            keep.append(y)
            _lib.set_rows(sg, "new_ref", y)
        if g_new[s] is not None:
            g = _rows(_lib.cast(g_new[s], dtype))
            keep.append(g)
            _lib.set_rows(sg, "g_new", g)
        if need_ref:
            g_refs[s] = torch.empty(r.shape, dtype=r.dtype, device=dev)
            sg.g_ref = g_refs[s].data_ptr()
        if mode == REFINE and need_delta:
            g_deltas[s] = torch.empty(r.shape, dtype=deltas[s].dtype, device=dev)
            sg.g_delta = g_deltas[s].data_ptr()
    if with_scale:
        for name, g in (("g_ref_input", g_ref_input), ("g_embed", g_embed)):
            if g is not None:
                g = _lib.cast(g.detach(), _F32).contiguous()
                keep.append(g)
                setattr(p, name, g.data_ptr())
    _lib.call("semidetr_ref_points_backward", dev, ctypes.byref(p))
    return g_deltas, g_refs


class RefPointsFunction(torch.autograd.Function):
    """``apply(mode, eps, valid_ratios, embed, detach, stacked, segments, *deltas, *refs)`` -> the tuple ``(*new_refs,
    ref_input, embed)`` without the entries the call does not produce: no ``new_refs`` for ``NONE``, one stacked tensor with
    ``stacked``, no ``ref_input`` / ``embed`` without ``valid_ratios`` / ``embed``.  ``detach``: ``ref_input`` and ``embed`` are
    computed from the detached refined points, as the decoder does from layer 1 on (transformer.py:1035)."""

    @staticmethod
    def forward(ctx, mode, eps, valid_ratios, embed, detach, stacked, segments, *rest):
        deltas, refs = (rest[:segments], rest[segments:]) if mode == REFINE else ((), rest)
        dtype = out_dtype(mode, deltas[0].dtype if mode == REFINE else None, refs[0].dtype)
        outs, ref_input, emb = _forward(mode, list(deltas), list(refs), eps, valid_ratios, embed, dtype, stacked)
        news = () if outs is None else (outs,) if stacked else tuple(outs)
        ctx.save_for_backward(valid_ratios, *deltas, *refs, *news)
        ctx.set_materialize_grads(False)
        ctx.cfg = (mode, eps, valid_ratios is not None, segments, len(deltas), stacked, len(news))
        extra = tuple(t for t in (ref_input, emb) if t is not None)
        if detach and extra:
            ctx.mark_non_differentiable(*extra)
        return news + extra

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        mode, eps, scaled, segments, ndelta, stacked, nnew = ctx.cfg
        saved = ctx.saved_tensors
        valid_ratios, deltas, refs = saved[0], saved[1:1 + ndelta], saved[1 + ndelta:1 + ndelta + segments]
        news = saved[1 + ndelta + segments:]
        none = (None,) * (7 + ndelta + segments)
        g_news, extra = grads[:nnew], list(grads[nnew:]) + [None, None]
        g_ref_input, g_embed = (extra[0], extra[1]) if scaled else (None, None)
        if all(g is None for g in grads):
            return none
        need = ctx.needs_input_grad[7:]
        need_delta, need_ref = any(need[:ndelta]), any(need[ndelta:])
        if not (need_delta or need_ref):
            return none
        if stacked:
            g_new = [None] * segments if g_news[0] is None else list(g_news[0].unbind(0))
            new_refs = list(news[0].unbind(0))
        else:
            g_new, new_refs = list(g_news) if nnew else [None] * segments, list(news)
        # a segment without any upstream gradient reads a zero one
        lacking = [s for s in range(segments) if g_new[s] is None and g_ref_input is None and g_embed is None]
        for s in lacking:
            g_new[s] = torch.zeros((1, 1, refs[s].shape[-1]), dtype=new_refs[s].dtype if mode != NONE else refs[s].dtype,
                                   device=refs[s].device).expand(refs[s].shape)
        g_deltas, g_refs = ref_points_backward(mode, deltas, refs, new_refs, g_new, eps, valid_ratios, g_ref_input, g_embed,
                                               need_delta, need_ref)
        g_deltas = [g if n else None for g, n in zip(g_deltas, need[:ndelta])]
        g_refs = [g if n else None for g, n in zip(g_refs, need[ndelta:])]
        return none[:7] + tuple(g_deltas) + tuple(g_refs)


def _apply(mode, eps, valid_ratios, embed, detach, stacked, deltas, refs, what):
    deltas, refs = list(deltas or ()), list(refs)
    _check(mode, deltas, refs, valid_ratios, what)
    return RefPointsFunction.apply(mode, float(eps), valid_ratios, embed, detach, stacked, len(refs), *deltas, *refs)


def gen_sineembed_for_position(pos_tensor):
    """``gen_sineembed_for_position`` of transformer.py:467-493: ``pos_tensor`` ``(nq, bs, 2 or 4)`` -> ``(nq, bs, 256 or 512)``
    fp32, blocks in the order ``(y, x[, w, h])``, even columns ``sin`` and odd columns ``cos`` of ``coord * 2 pi / dim_t``."""
    if pos_tensor.size(-1) not in (2, 4):
        raise ValueError("Unknown pos_tensor shape(-1):{}".format(pos_tensor.size(-1)))
    ones = _ones(pos_tensor.device, pos_tensor.shape[1] if pos_tensor.dim() == 3 else 1)
    return _apply(NONE, 0.0, ones, True, False, False, None, [pos_tensor], "gen_sineembed_for_position")[1]


def refine_boxes(delta, reference, eps=1e-5):
    """``sigmoid(delta + inverse_sigmoid(reference, eps))`` (transformer.py:1029-1032, :435-451) with gradients to both."""
    return _apply(REFINE, eps, None, False, False, False, [delta], [reference], "refine_boxes")[0]


def reference_inputs(reference_points, valid_ratios):
    """``(reference_points_input, query_sine_embed)`` of transformer.py:979-985 for ``reference_points`` ``(nq, bs, 2 or 4)`` and
    ``valid_ratios`` ``(bs, L, 2)``: ``(nq, bs, L, width)`` -- the transpose of contiguous ``(bs, nq, L, width)`` memory -- and
    ``(nq, bs, 128 * width)``."""
    ref_input, emb = _apply(NONE, 0.0, valid_ratios, True, False, False, None, [reference_points], "reference_inputs")
    return ref_input.transpose(0, 1), emb


def _why_not(decoder):
    """Why a decoder cannot go through ``decoder_forward``, or ``None``."""
    if not getattr(decoder, "deformable_decoder", False):
        return "deformable_decoder=False (only the deformable decoder is built)"
    if getattr(decoder, "query_pos_sine_scale", None) is not None:
        return "query_pos_sine_scale (a branch of the non-deformable decoder) is not built"
    if getattr(decoder, "modulate_hw_attn", False) and getattr(decoder, "ref_anchor_head", None) is not None:
        return "modulate_hw_attn with a ref_anchor_head (a branch of the non-deformable decoder) is not built"
    if getattr(decoder, "dec_layer_dropout_prob", None) is not None:
        return "dec_layer_dropout_prob is not built"
    if getattr(decoder, "rm_detach", None):
        return f"rm_detach={decoder.rm_detach!r} is not built"
    return None


def decoder_forward(decoder, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                    memory_key_padding_mask=None, pos=None, refpoints_unsigmoid=None, level_start_index=None, spatial_shapes=None,
                    valid_ratios=None, fc_reg=None, fc_cls=None):
    """``DINOTransformerDecoder.forward`` (transformer.py:947-1045), same arguments, same return structure: ``[[norm(output)
    .transpose(0, 1) per layer], [reference points .transpose(0, 1): the initial ones and one per layer]]``.  Each layer runs
    through ``add_norm.decoder_layer_forward``; ``ref_point_head``, ``query_scale``, ``fc_reg[i]`` and ``norm`` stay module calls.
    The reference-point chain is one launch in front of layer 0 (sigmoid, scale, embed), one between consecutive layers (refine,
    detach, scale, embed) and one after the last layer (refine); with ``fc_reg is None`` the points never change and the first
    launch's results serve every layer."""
    reason = _why_not(decoder)
    if reason:
        raise NotImplementedError(f"decoder_forward: {reason}")
    if refpoints_unsigmoid is None or valid_ratios is None:
        raise ValueError("decoder_forward: refpoints_unsigmoid and valid_ratios are needed")
    output, intermediate = tgt, []
    reference_points, ref_input, embed = _apply(SIGMOID, 0.0, valid_ratios, True, False, False, None, [refpoints_unsigmoid],
                                                "decoder_forward")
    ref_points = [reference_points]
    layers = list(decoder.layers)
    for layer_id, layer in enumerate(layers):
        query_pos = decoder.ref_point_head(embed)
        if decoder.query_scale is not None:
            query_pos = decoder.query_scale(output) * query_pos
        output = add_norm.decoder_layer_forward(layer, output, query_pos, embed, tgt_key_padding_mask, ref_input.transpose(0, 1),
                                                memory, memory_key_padding_mask, level_start_index, spatial_shapes, pos, tgt_mask,
                                                memory_mask)
        if fc_reg is not None:
            delta = fc_reg[layer_id](output)
            if layer_id + 1 < len(layers):
                new_reference_points, ref_input, embed = _apply(REFINE, 1e-5, valid_ratios, True, True, False, [delta],
                                                                [reference_points], "decoder_forward")
            else:
                new_reference_points = _apply(REFINE, 1e-5, None, False, False, False, [delta], [reference_points],
                                              "decoder_forward")[0]
            reference_points = new_reference_points.detach()
            ref_points.append(new_reference_points)
        intermediate.append(decoder.norm(output))
    return [[itm_out.transpose(0, 1) for itm_out in intermediate], [itm_refpoint.transpose(0, 1) for itm_refpoint in ref_points]]


def box_outputs(fc_reg, hs, reference, eps=1e-5):
    """The head's ``outputs_coord`` (dino_detr_ssod_head.py:393-398): ``stack([sigmoid(fc_reg[l](hs[l]) + inverse_sigmoid(
    reference[l])) for l])`` over ``zip(reference[:-1], fc_reg, hs)``, ``(layers, bs, nq, 4)``.  The ``fc_reg[l]`` stay module
    calls; the layers' updates are one segmented launch forward and one backward, the ``(bs, nq, 4)`` transposes read in place,
    with the gradient into ``reference[l]`` (undetached in the head: DINO's "look forward twice")."""
    pairs = list(zip(reference[:-1], fc_reg, hs))
    if not 1 <= len(pairs) <= MAX_SEGMENTS:
        raise NotImplementedError(f"box_outputs: {len(pairs)} layers (1 .. {MAX_SEGMENTS} segments)")
    deltas = [layer_fc_reg(layer_hs) for _, layer_fc_reg, layer_hs in pairs]
    return _apply(REFINE, eps, None, False, False, True, deltas, [r for r, _, _ in pairs], "box_outputs")[0]

"""Two-stage query selection of DINO on the MI355X (``csrc/query_select.hip``): what ``DINOTransformer.forward`` runs between
the encoder and the decoder (detr_od/models/utils/transformer.py:525-575, 1315-1346, 1398).

* ``gen_encoder_output_proposals`` replaces the function of the same name (transformer.py:525-575): same signature, same
  return pair, differentiable w.r.t. ``memory``.  One launch forward, one backward.
* ``select_queries`` replaces ``max(-1)`` + ``torch.topk`` + the three gathers + the ``ref_enc`` sigmoid
  (transformer.py:1325-1334, 1398): three launches forward (class max, select, gather), one backward.
* ``two_stage_queries`` binds as a helper of ``DINOTransformer`` and performs the whole ``two_stage_type == 'standard'``
  block; the ``enc_output`` / ``enc_output_norm`` / head GEMMs in it stay torch calls.

Selection order.  ``torch.topk`` leaves the order among equal keys open, and every padded or invalid token has the same
zeroed ``output_memory`` row, hence bit-identical logits.  Here the k tokens come sorted by (key descending, token index
ascending): a total order, so the choice among tied tokens is the lowest indices, run after run.  NaN ranks above +inf.

Dtypes.  Every floating operand may be fp32, fp16 or bf16, each on its own: under autocast ``fc_enc_cls`` hands
``select_queries`` 16-bit logits next to fp32 coordinates, proposals and memory; a ``.half()`` model hands over 16-bit memory.
16-bit operands are up-cast exactly and the kernels run in fp32, so the selected tokens are the first k of the total order on
the keys as given.  The results have the dtypes the reference's op sequence gives: ``output_memory`` that of ``memory``, the
proposals fp32, ``refpoint_embed_undetach`` and ``ref_enc`` that of ``enc_outputs_coord``, ``init_box_proposal`` that of
``output_proposals``, ``tgt_undetach`` that of ``output_memory``; copies are bitwise, a sigmoid that leaves in 16 bits is rounded
once.  Gradients have the dtype of the tensor they belong to.

``forward_with_query`` (transformer.py:1409-1481) has no two-stage block -- it takes its queries from the caller -- so only
``forward`` has a use for ``two_stage_queries``.
"""
import ctypes

import torch

from . import _lib

MAX_LEVELS, MAX_K = _lib.CONSTANTS["SEMIDETR_QSEL_MAX_LEVELS"], _lib.CONSTANTS["SEMIDETR_QSEL_MAX_K"]


def _require(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"query_select: {what} must live on the GPU (no CPU fallback)")


def _f32(t, what):
    """``t`` as the kernels read it: detached, contiguous, fp32.  fp16 and bf16 are up-cast (exact); other dtypes are refused."""
    if t.dtype != torch.float32:
        if t.dtype not in (torch.float16, torch.bfloat16):
            raise TypeError(f"query_select: {what} must be float32, float16 or bfloat16, got {t.dtype}")
        return t.detach().float().contiguous()
    return t if t.is_contiguous() and not t.requires_grad else t.detach().contiguous()


def _level_table(spatial_shapes, dev):
    """(host array or None, device tensor or None, number of levels).  A device tensor is handed to the kernel as it is
    (nothing is read back); lists, tuples and CPU tensors travel as kernel arguments."""
    if isinstance(spatial_shapes, torch.Tensor) and spatial_shapes.is_cuda:
        t = spatial_shapes.detach()
        if t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"query_select: spatial_shapes must be (levels, 2), got {tuple(t.shape)}")
        if t.dtype != torch.int64 or t.device != dev or not t.is_contiguous():
            t = t.to(device=dev, dtype=torch.int64).contiguous()
        return None, t, int(t.shape[0])
    rows = spatial_shapes.tolist() if isinstance(spatial_shapes, torch.Tensor) else [tuple(r) for r in spatial_shapes]
    if not rows or any(len(r) != 2 for r in rows):
        raise ValueError("query_select: spatial_shapes must be (levels, 2)")
    host = (ctypes.c_int64 * (2 * len(rows)))(*[int(v) for r in rows for v in r])
    return host, None, len(rows)


class _ProposalsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, memory, mask, spatial_shapes):
        mem = _f32(memory, "memory")
        N, S, D = mem.shape
        dev = mem.device
        m = mask.detach()
        if m.shape != (N, S):
            raise ValueError(f"query_select: memory_padding_mask is {tuple(m.shape)}, memory has {(N, S)} tokens")
        if m.dtype != torch.bool or m.device != dev:
            m = m.to(device=dev, dtype=torch.bool)
        m = m.contiguous()
        host, table, L = _level_table(spatial_shapes, dev)
        if L > MAX_LEVELS:
            raise ValueError(f"query_select: {L} levels (at most {MAX_LEVELS})")
        out = torch.empty_like(mem)
        prop = torch.empty((N, S, 4), dtype=torch.float32, device=dev)
        valid = torch.empty((N, S), dtype=torch.uint8, device=dev)
        _lib.call("semidetr_qsel_proposals_f32", dev, mem, m, host, table, L, N, S, D, out, prop, valid)
        ctx.save_for_backward(valid)
        ctx.mark_non_differentiable(prop)
        ctx.set_materialize_grads(False)
        ctx.dtype = memory.dtype
        return _lib.cast(out, memory.dtype), prop

    @staticmethod
    def backward(ctx, g_out, _g_prop):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (valid,) = ctx.saved_tensors
        g = _f32(g_out, "grad of output_memory")
        N, S, D = g.shape
        gm = torch.empty_like(g)
        _lib.call("semidetr_qsel_proposals_backward_f32", g.device, g, valid, N, S, D, gm)
        return _lib.cast(gm, ctx.dtype), None, None


def gen_encoder_output_proposals(memory, memory_padding_mask, spatial_shapes, learnedwh=None):
    """transformer.py:525-575 -> (output_memory (N, S, d), output_proposals (N, S, 4)).  ``spatial_shapes``: the (levels, 2)
    tensor the reference passes, or a list of (H, W)."""
    if learnedwh is not None:
        raise NotImplementedError("query_select.gen_encoder_output_proposals: learnedwh is not None; the reference's only call "
                                  "site, DINOTransformer.forward (transformer.py:1317-1318), passes None")
    _require(memory, "memory")
    if memory.dim() != 3:
        raise ValueError(f"query_select: memory must be (N, S, d_model), got {tuple(memory.shape)}")
    return _ProposalsFn.apply(memory, memory_padding_mask, spatial_shapes)


class _SelectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, coord, proposals, memory, k):
        lg, cd, pr, mem = (_f32(logits, "enc_outputs_class"), _f32(coord, "enc_outputs_coord"),
                           _f32(proposals, "output_proposals"), _f32(memory, "output_memory"))
        N, S, C = lg.shape
        D = mem.shape[2]
        dev = lg.device
        ws_bytes = _lib.lib().semidetr_qsel_topk_workspace_bytes(N, S)
        ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
        idx = torch.empty((N, k), dtype=torch.int64, device=dev)
        inv = torch.empty((N, S), dtype=torch.int32, device=dev)
        ref = torch.empty((N, k, 4), dtype=torch.float32, device=dev)
        init_box, ref_enc = torch.empty_like(ref), torch.empty_like(ref)
        tgt = torch.empty((N, k, D), dtype=torch.float32, device=dev)
        _lib.calls(dev, ("semidetr_qsel_topk_f32", lg, N, S, C, k, ws, ws_bytes, idx, inv),
                   ("semidetr_qsel_gather_f32", idx, cd, pr, mem, N, S, k, D, ref, init_box, tgt, ref_enc))
        ctx.sizes = (N, S, k, D)
        ctx.dtypes = (coord.dtype, memory.dtype)
        ctx.save_for_backward(inv, ref_enc)                        # the fp32 sigmoid, before any rounding on the way out
        ref, ref_enc = _lib.cast(ref, coord.dtype), _lib.cast(ref_enc, coord.dtype)
        init_box, tgt = _lib.cast(init_box, proposals.dtype), _lib.cast(tgt, memory.dtype)
        ctx.mark_non_differentiable(idx, init_box)
        ctx.set_materialize_grads(False)
        return idx, ref, init_box, tgt, ref_enc

    @staticmethod
    def backward(ctx, _g_idx, g_ref, _g_init, g_tgt, g_enc):
        inv, ref_enc = ctx.saved_tensors
        N, S, k, D = ctx.sizes
        dev = inv.device
        want_c = ctx.needs_input_grad[1] and (g_ref is not None or g_enc is not None)
        want_m = ctx.needs_input_grad[3] and g_tgt is not None
        if not (want_c or want_m):
            return None, None, None, None, None
        g_ref, g_tgt, g_enc = [None if g is None else _f32(g, "gradient") for g in (g_ref, g_tgt, g_enc)]
        gc = torch.empty((N, S, 4), dtype=torch.float32, device=dev) if want_c else None
        gm = torch.empty((N, S, D), dtype=torch.float32, device=dev) if want_m else None
        _lib.call("semidetr_qsel_gather_backward_f32", dev, inv, g_ref, g_tgt, g_enc, ref_enc, N, S, k, D, gc, gm)
        return None, _lib.cast(gc, ctx.dtypes[0]), None, _lib.cast(gm, ctx.dtypes[1]), None


def select_queries(enc_outputs_class, enc_outputs_coord, output_proposals, output_memory, num_queries):
    """transformer.py:1325-1334 + 1398 -> (topk_proposals (N, k) int64, refpoint_embed_undetach (N, k, 4), init_box_proposal
    (N, k, 4), tgt_undetach (N, k, d), ref_enc (N, k, 4) = refpoint_embed_undetach.sigmoid()).  Differentiable w.r.t.
    ``enc_outputs_coord`` and ``output_memory``."""
    for t, what in ((enc_outputs_class, "enc_outputs_class"), (enc_outputs_coord, "enc_outputs_coord"),
                    (output_proposals, "output_proposals"), (output_memory, "output_memory")):
        _require(t, what)
    N, S = enc_outputs_class.shape[:2]
    k = int(num_queries)
    if enc_outputs_class.dim() != 3 or enc_outputs_coord.shape != (N, S, 4) or output_proposals.shape != (N, S, 4) or \
            output_memory.dim() != 3 or output_memory.shape[:2] != (N, S):
        raise ValueError("query_select: expected enc_outputs_class (N, S, C), enc_outputs_coord / output_proposals (N, S, 4) and "
                         "output_memory (N, S, d_model)")
    if k > S or k < 0:
        raise RuntimeError("selected index k out of range")          # torch.topk's own error
    if k == 0 or k > MAX_K:
        raise ValueError(f"query_select: num_queries {k} (1..{MAX_K})")
    return _SelectFn.apply(enc_outputs_class, enc_outputs_coord, output_proposals, output_memory, k)


def two_stage_queries(self, memory, mask_flatten, spatial_shapes, fc_enc_cls, fc_enc_reg, refpoint_embed, tgt):
    """The ``two_stage_type == 'standard'`` block of ``DINOTransformer.forward`` (transformer.py:1315-1346) and what its
    postprocess takes from it (:1394-1398), as a helper of the transformer (``self``: ``enc_output``, ``enc_output_norm``,
    ``num_queries``, ``embed_init_tgt``, ``tgt_embed``).  ``refpoint_embed`` / ``tgt``: the dn part or None.
    Returns (refpoint_embed, tgt, hs_enc, ref_enc, init_box_proposal): the decoder's ``refpoints_unsigmoid`` and ``tgt``
    before their transposes, and the last three return values of ``forward``."""
    if self.two_stage_type != "standard":
        raise NotImplementedError(f"query_select.two_stage_queries: two_stage_type {self.two_stage_type!r}")
    if not self.embed_init_tgt:
        raise NotImplementedError("query_select.two_stage_queries: embed_init_tgt is False")
    output_memory, output_proposals = gen_encoder_output_proposals(memory, mask_flatten, spatial_shapes, None)
    output_memory = self.enc_output_norm(self.enc_output(output_memory))
    enc_outputs_class_unselected = fc_enc_cls(output_memory)
    enc_outputs_coord_unselected = fc_enc_reg(output_memory) + output_proposals
    _, refpoint_embed_undetach, init_box_proposal, tgt_undetach, ref_enc = select_queries(
        enc_outputs_class_unselected, enc_outputs_coord_unselected, output_proposals, output_memory, self.num_queries)
    refpoint_embed_ = refpoint_embed_undetach.detach()
    bs = memory.shape[0]
    tgt_ = self.tgt_embed.weight[:self.num_queries, None, :].repeat(1, bs, 1).transpose(0, 1)
    if refpoint_embed is not None:
        refpoint_embed = torch.cat([refpoint_embed, refpoint_embed_], dim=1)
        tgt = torch.cat([tgt, tgt_], dim=1)
    else:
        refpoint_embed, tgt = refpoint_embed_, tgt_
    return refpoint_embed, tgt, tgt_undetach.unsqueeze(0), ref_enc.unsqueeze(0), init_box_proposal

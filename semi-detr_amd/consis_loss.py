"""Cross-view query consistency loss on the MI355X (``csrc/consis_loss.hip``): the last block of ``DinoDetrSSOD.unsup_loss``
(detr_ssod/models/dino_detr_ssod.py:463-481), every decoder layer in one call.

``consistency_loss(hs_v1, hs_v2, dn_meta)`` returns ``{"consis_loss.d0": ..., ...}``, 0-d tensors under the reference's keys,
ready for ``losses.update(...)``.  ``hs_v1`` / ``hs_v2`` are the reference's lists of ``(B, Q, D)`` tensors (transposed views of
``(Q, B, D)`` buffers: they are read through their strides, nothing is copied) or stacked ``(L, B, Q, D)`` tensors; ``dn_meta`` is
what ``dn_query.prepare_unsup_cdn`` returns (``known_bid_1`` fp32 or int64, ``map_known_indice_1``, ``loss_weights``,
``pad_size_1``).  Only ``hs_v1`` receives a gradient (``hs_v2`` is detached, as in the reference).

A call is two launches forward and one backward, on the current stream, with no host synchronisation and no ``.item()``.  The
``L`` losses leave the autograd Function as one ``(L,)`` tensor and are split with ``unbind``, so their upstream gradients come
back as one tensor (a layer whose loss is unused gets 0) and the backward of all layers is one launch; it writes the dense
gradient of every ``hs_v1[l]`` -- zeros outside the selected rows included, no memset.

Contract: the ``(known_bid, map_known_indice)`` pairs are distinct (``idx = i + single_pad * g`` by construction).  A pair outside
``[0, B) x [0, pad_size)`` is never dereferenced: every layer's loss is NaN and the pair gets no gradient row (the reference
raises a device-side index error there).  ``K == 0`` gives NaN losses (torch's mean of an empty tensor) and zero gradients
without a launch of the library.

Weights: row ``k`` of every layer is weighted by ``loss_weights[k]`` (a ``(K,)`` vector or the ``(K, 1)`` column of
``prepare_unsup_cdn``).  The reference's ``(K, D) * loss_weights.unsqueeze(-1)`` does the same for a vector; for the column it
broadcasts to ``(K, K, D)`` and yields ``mean(w)`` times the unweighted mean, which is the same number for uniform weights and
differs where a batch mixes images with and without pseudo boxes.

``warm_up=False`` is the reference's ``loss_weights = zeros_like(loss_weights)`` past the warm-up step: the kernels are still
launched, with a NULL weight pointer that reads as zeros, so every loss is exactly 0.0 and every gradient element exactly 0
(written by the one backward launch) and no zero tensor is built.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_LAYERS = _lib.CONSTANTS["SEMIDETR_CONSIS_MAX_LAYERS"]
_Layer, _Params = _lib.ConsisLayer, _lib.ConsisLoss


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"consis_loss: {what} must live on the GPU (no CPU fallback)")


def _layers(hs, what):
    """The per-layer ``(B, Q, D)`` tensors of a list or of a stacked ``(L, B, Q, D)`` tensor."""
    if isinstance(hs, torch.Tensor):
        if hs.dim() != 4:
            raise ValueError(f"consis_loss: a stacked {what} is (L, B, Q, D), got {tuple(hs.shape)}")
        return [hs[l] for l in range(hs.shape[0])]
    hs = list(hs)
    if not hs or any(t.dim() != 3 or t.shape != hs[0].shape for t in hs):
        raise ValueError(f"consis_loss: {what} is a non-empty list of (B, Q, D) tensors of one shape")
    return hs


class ConsistencyLossFunction(torch.autograd.Function):
    """``apply(st, hs_v1)`` (stacked) or ``apply(st, *hs_v1)`` (list) -> the ``(L,)`` losses.  ``st``: the detached inputs and
    sizes (``consistency_loss`` builds it)."""

    @staticmethod
    def forward(ctx, st, *hs1):
        L, B, Q, D, K = st["L"], st["B"], st["Q"], st["D"], st["K"]
        v1 = _layers(hs1[0], "hs_v1") if st["stacked"] else list(hs1)
        dev = v1[0].device
        ctx.st = st
        ctx.dtypes = [t.dtype for t in hs1]
        if K == 0:
            return torch.full((L,), float("nan"), dtype=torch.float32, device=dev)
        v1 = [_lib.rows_f32(t) for t in v1]
        p = _Params()
        p.num_layers, p.batch, p.num_query, p.dim, p.pad_size, p.num_known = L, B, Q, D, st["pad_size"], K
        p.scale, p.eps = st["scale"], st["eps"]
        bid, idx, w = st["bid"], st["idx"], st["weights"]
        p.bid_is_int64 = int(bid.dtype == torch.int64)
        p.known_bid, p.map_known_indice = bid.data_ptr(), idx.data_ptr()
        p.loss_weights = w.data_ptr() if w is not None else None
        for l, (a, b) in enumerate(zip(v1, st["v2"])):
            ly = p.layer[l]
            _lib.set_rows(ly, "v1", a)
            _lib.set_rows(ly, "v2", b)
        nbytes = _lib.lib().semidetr_consis_loss_workspace_bytes(L, K, B, st["pad_size"])
        work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        losses = torch.empty((L,), dtype=torch.float32, device=dev)
        _lib.call("semidetr_consis_loss_forward_f32", dev, ctypes.byref(p), work, nbytes, losses)
        ctx.params, ctx.nbytes = p, nbytes
        ctx.save_for_backward(work, *v1)               # st keeps hs_v2, the indices and the weights alive
        return losses

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        st = ctx.st
        L, B, Q, D = st["L"], st["B"], st["Q"], st["D"]
        if not any(ctx.needs_input_grad[1:]):
            return (None,) * (1 + len(ctx.dtypes))
        dev = g.device
        if st["K"] == 0:
            grad = torch.zeros((L, B, Q, D), dtype=torch.float32, device=dev)
        else:
            work = ctx.saved_tensors[0]
            g = g.float().contiguous()
            grad = torch.empty((L, B, Q, D), dtype=torch.float32, device=dev)
            p = ctx.params
            for l in range(L):
                p.layer[l].grad_v1 = grad[l].data_ptr()
            _lib.call("semidetr_consis_loss_backward_f32", dev, ctypes.byref(p), work, ctx.nbytes, g)
        if st["stacked"]:
            return None, grad.to(ctx.dtypes[0])
        return (None,) + tuple(grad[l].to(dt) if need else None
                               for l, (dt, need) in enumerate(zip(ctx.dtypes, ctx.needs_input_grad[1:])))


def consistency_loss(hs_v1, hs_v2, dn_meta, warm_up=True, scale=10.0, eps=1e-12):
    """The reference's consistency-loss loop: ``{"consis_loss.d<l>": 0-d tensor}`` for every decoder layer (module docstring).
    ``warm_up=False`` past ``warm_up_step`` (all weights zero); ``eps`` is F.normalize's."""
    stacked = isinstance(hs_v1, torch.Tensor)
    v1 = _layers(hs_v1, "hs_v1")
    v2 = _layers(hs_v2, "hs_v2")
    for t in v1 + v2:
        _require_cuda(t, "hs_v1 / hs_v2")
    L, (B, Q, D) = len(v1), v1[0].shape
    if len(v2) != L or v2[0].shape != v1[0].shape:
        raise ValueError(f"consis_loss: hs_v1 has {L} layers of {tuple(v1[0].shape)}, hs_v2 {len(v2)} of {tuple(v2[0].shape)}")
    if L > MAX_LAYERS:
        raise ValueError(f"consis_loss: {L} decoder layers (at most {MAX_LAYERS})")
    if D % 4:
        raise ValueError(f"consis_loss: D = {D} is not a multiple of 4")
    dev = v1[0].device
    pad_size = int(dn_meta["pad_size_1"])
    if not 0 <= pad_size <= Q:
        raise ValueError(f"consis_loss: pad_size_1 = {pad_size} outside [0, Q = {Q}]")
    bid = dn_meta["known_bid_1"].detach().reshape(-1)
    _require_cuda(bid, "known_bid_1")
    if bid.dtype not in (torch.float32, torch.int64):
        bid = bid.to(torch.int64)
    idx = dn_meta["map_known_indice_1"].detach().reshape(-1)
    _require_cuda(idx, "map_known_indice_1")
    if idx.dtype != torch.int64:
        idx = idx.to(torch.int64)
    K = bid.numel()
    if idx.numel() != K:
        raise ValueError(f"consis_loss: {K} known_bid_1 entries but {idx.numel()} map_known_indice_1 entries")
    weights = None
    if warm_up:
        weights = dn_meta["loss_weights"].detach().reshape(-1)
        _require_cuda(weights, "loss_weights")
        if weights.numel() != K:
            raise ValueError(f"consis_loss: {K} pairs but {weights.numel()} loss weights")
        weights = (weights if weights.dtype == torch.float32 else weights.float()).contiguous()
    st = dict(L=L, B=B, Q=Q, D=D, K=K, pad_size=pad_size, scale=float(scale), eps=float(eps), stacked=stacked,
              bid=bid.contiguous(), idx=idx.contiguous(), weights=weights, v2=[_lib.rows_f32(t) for t in v2])
    losses = ConsistencyLossFunction.apply(st, hs_v1) if stacked else ConsistencyLossFunction.apply(st, *v1)
    return {f"consis_loss.d{l}": v for l, v in enumerate(losses.unbind(0))}

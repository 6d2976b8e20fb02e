"""Decoder self-attention on the MI355X (``csrc/self_attn.hip``): the dense attention of ``DINOTransformerDecoderLayer``
(detr_od/models/utils/transformer.py:765, 793-816), ``self.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]``.

``masked_attention(q, k, v, num_heads, attn_mask=None, scale=None, arithmetic="fp32")`` is the core ``softmax(scale * q k^T + mask) v`` on seq-first
``(L, B, E)`` tensors: forward two launches (one without a mask), backward three at most, on the current stream, with no host
synchronisation and no ``.item()``.  The ``(Lq, Lk)`` scores never reach memory; the op saves its inputs, ``out`` and the row
log-sum-exp ``(B, H, Lq)``.  ``q``, ``k`` and ``v`` are read through their first two strides (last stride 1, rows 16-byte
aligned, copied only where they are not), so slices of one in-projection output are read in place.  ``attn_mask`` is torch's
bool ``(Lq, Lk)`` mask, ``True`` = blocked; the mask that ``dn_query`` writes is block-structured and its fully blocked 32 x 32
tiles are skipped.  A row with every key blocked is NaN, as in torch.

``MultiheadAttention`` is the drop-in for the layer's ``nn.MultiheadAttention`` (same parameter names and shapes, so a
reference ``state_dict`` loads with ``strict=True``); the two projections stay GEMMs.  ``convert_self_attention(module)``
replaces the qualifying ``nn.MultiheadAttention`` children of a built model in place, adopting their ``Parameter`` objects.

Dtypes.  ``q``, ``k`` and ``v`` may be fp32, fp16 or bf16.  With ``arithmetic="fp32"`` (the default) 16-bit operands are up-cast
exactly, the arithmetic is fp32, and ``out`` comes back in the dtype of ``q`` (of the packed ``[q | k]`` buffer), rounded once;
each gradient has the dtype of its operand.  Under autocast the module's projections are 16-bit GEMMs, so the core receives and
returns 16-bit tensors and the module returns what ``nn.MultiheadAttention`` returns there: a 16-bit output, fp32 gradients for
fp32 inputs and parameters.

``arithmetic="operand"`` (``ArithH16`` of ``csrc/self_attn.hip``) computes fp16 / bf16 operands of one common dtype
on the 16-bit MFMA: the kernels read ``q``, ``k``, ``v``, ``grad_out`` and the saved ``out`` in place as 16-bit (rows 8-byte
aligned) and write ``out`` and the gradients as 16-bit, so nothing is allocated in fp32 but ``lse`` and the workspace and no
cast pass runs.  Its numerics contract is its own (include/semidetr_hip.h): scores, softmax statistics and ``lse`` in fp32 on the
unrounded probabilities; ``P`` and ``dS`` rounded once to the operand type before their products; every result rounded once.
fp32 operands take the fp32 kernels whatever ``arithmetic`` says; mixed dtypes are a ``ValueError``.  The module and
``convert_self_attention`` carry the choice as the plain attribute ``arithmetic``.

Not built: float and 3-D masks, ``key_padding_mask``, attention dropout, head dimensions other than 32
and the head-averaged attention weights.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn import functional as F

from . import _lib

HEAD_DIM = 32
ARITHMETICS = ("fp32", "operand")
_Params = _lib.SelfAttn
_Params16 = _lib.SelfAttnH16


def _split(x, y, z, packed_qk):
    if not packed_qk:
        return x, y, z
    E = y.shape[2]
    return x[..., :E], x[..., E:], y


def _params(q, k, v, mask, heads, scale, block=_Params):
    p = block()
    (Lq, B, E), Lk = q.shape, k.shape[0]
    p.batch, p.heads, p.head_dim, p.len_q, p.len_k, p.scale = B, heads, E // heads, Lq, Lk, scale
    _lib.set_rows(p, "q", q)
    _lib.set_rows(p, "k", k)
    _lib.set_rows(p, "v", v)
    p.mask = mask.data_ptr() if mask is not None else None
    return p


def _workspace(p, dev):
    nbytes = _lib.lib().semidetr_self_attn_workspace_bytes(p.batch, p.heads, p.len_q, p.len_k)
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def _operands(native, x, y, z, mask, num_heads, scale, packed_qk):
    """q, k, v as the kernels of one arithmetic read them and their parameter block.  ``native``: the 16-bit kernels, fp16 /
    bf16 rows in place; otherwise the fp32 kernels on exactly up-cast rows."""
    rows = _lib.rows_native if native else _lib.rows_f32
    q, k, v = (rows(t) for t in _split(x, y, z, packed_qk))
    p = _params(q, k, v, mask, num_heads, scale, _Params16 if native else _Params)
    if native:
        p.type = _lib.row_type(q.dtype)
    return q, k, v, p


def _forward(ctx, native, x, y, z, mask, num_heads, scale, packed_qk):
    q, k, v, p = _operands(native, x, y, z, mask, num_heads, scale, packed_qk)
    dev = q.device
    out = torch.empty(q.shape, dtype=q.dtype, device=dev)
    lse = torch.empty((p.batch, num_heads, p.len_q), dtype=torch.float32, device=dev)
    p.out, p.lse = out.data_ptr(), lse.data_ptr()
    work, nbytes = _workspace(p, dev)
    _lib.call("semidetr_self_attn_forward_h16" if native else "semidetr_self_attn_forward_f32", dev, ctypes.byref(p), work, nbytes)
    ctx.num_heads, ctx.scale, ctx.packed_qk = num_heads, scale, packed_qk
    ctx.dtypes = [t.dtype if t is not None else None for t in (x, y, z)]
    ctx.save_for_backward(x, y, z, mask, out, lse)
    return _lib.cast(out, x.dtype)


def _backward(ctx, native, g):
    x, y, z, mask, out, lse = ctx.saved_tensors
    need = ctx.needs_input_grad[:3]
    if not any(need):
        return (None,) * 7
    q, k, v, p = _operands(native, x, y, z, mask, ctx.num_heads, ctx.scale, ctx.packed_qk)
    dev, dt = q.device, q.dtype                    # fp32, or the operands' 16-bit type on the native route
    g = _lib.cast(g.detach(), dt).contiguous()
    p.out, p.lse, p.grad_out = out.data_ptr(), lse.data_ptr(), g.data_ptr()
    if ctx.packed_qk:
        need_q = need_k = need[0]
        need_v = need[1]
        gx = torch.empty(x.shape, dtype=dt, device=dev) if need[0] else None
        E = y.shape[2]
        gq, gk = (gx[..., :E], gx[..., E:]) if need[0] else (None, None)
    else:
        need_q, need_k, need_v = need
        gq = torch.empty(q.shape, dtype=dt, device=dev) if need_q else None
        gk = torch.empty(k.shape, dtype=dt, device=dev) if need_k else None
    gv = torch.empty(v.shape, dtype=dt, device=dev) if need_v else None
    _lib.set_rows(p, "grad_q", gq, "gq_stride")
    _lib.set_rows(p, "grad_k", gk, "gk_stride")
    _lib.set_rows(p, "grad_v", gv, "gv_stride")
    work, nbytes = _workspace(p, dev)
    _lib.call("semidetr_self_attn_backward_h16" if native else "semidetr_self_attn_backward_f32", dev, ctypes.byref(p), work, nbytes)
    if ctx.packed_qk:
        return _lib.cast(gx, ctx.dtypes[0]), _lib.cast(gv, ctx.dtypes[1]), None, None, None, None, None
    return _lib.cast(gq, ctx.dtypes[0]), _lib.cast(gk, ctx.dtypes[1]), _lib.cast(gv, ctx.dtypes[2]), None, None, None, None


class MaskedAttentionFunction(torch.autograd.Function):
    """``apply(x, y, z, mask, num_heads, scale, packed_qk)`` -> ``out (Lq, B, E)``.  ``packed_qk`` false: ``x, y, z`` are
    ``q, k, v``.  True: ``x`` is the ``(L, B, 2E)`` output of one GEMM that holds ``[q | k]``, ``y`` is ``v`` and ``z`` is
    ``None``; the backward then writes ``dq`` and ``dk`` side by side into ONE gradient buffer for ``x``, so autograd adds no
    slice-backward copies.  ``mask``: ``None`` or a contiguous ``(Lq, Lk)`` uint8 tensor, non-zero = blocked.  The fp32
    arithmetic: 16-bit operands are up-cast exactly, every result is rounded once into its operand's dtype."""

    @staticmethod
    def forward(ctx, *args):
        return _forward(ctx, False, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _backward(ctx, False, g)


class MaskedAttentionH16Function(torch.autograd.Function):
    """``MaskedAttentionFunction`` with the ``operand`` arithmetic: ``x, y, z`` are fp16 or bf16 tensors of one dtype, read in
    place (``_lib.rows_native``); ``out`` and the gradients are written in that dtype by the kernels.  Saved: the inputs, the
    16-bit ``out`` and the fp32 ``lse``; nothing but ``lse`` and the workspace is allocated in fp32."""

    @staticmethod
    def forward(ctx, *args):
        return _forward(ctx, True, *args)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _backward(ctx, True, g)


def _function(arithmetic, *operands):
    """The autograd function of ``arithmetic`` for these operands (``None`` entries are skipped): ``operand`` takes the 16-bit
    kernels where the operands are fp16 or bf16, of one dtype; fp32 operands take the fp32 kernels either way."""
    if arithmetic not in ARITHMETICS:
        raise ValueError(f"masked_attention: arithmetic is one of {ARITHMETICS}, got {arithmetic!r}")
    if arithmetic == "fp32":
        return MaskedAttentionFunction
    dtypes = {t.dtype for t in operands if t is not None}
    if len(dtypes) != 1:
        raise ValueError(f"masked_attention: arithmetic='operand' takes q, k and v of one dtype, got {sorted(map(str, dtypes))}")
    return MaskedAttentionFunction if dtypes == {torch.float32} else MaskedAttentionH16Function


def _byte_mask(attn_mask, Lq, Lk, dev):
    """torch's bool ``attn_mask`` as the kernel's ``(Lq, Lk)`` byte matrix (a view where it is contiguous)."""
    if attn_mask is None:
        return None
    if attn_mask.dim() != 2:
        raise NotImplementedError(f"masked_attention: attn_mask is (Lq, Lk), got {attn_mask.dim()} dimensions "
                                  "(per-head masks are not built)")
    if attn_mask.dtype not in (torch.bool, torch.uint8):
        raise NotImplementedError(f"masked_attention: attn_mask is a bool mask, got {attn_mask.dtype} (float masks are not built)")
    if tuple(attn_mask.shape) != (Lq, Lk):
        raise ValueError(f"masked_attention: attn_mask is {tuple(attn_mask.shape)}, expected {(Lq, Lk)}")
    if attn_mask.device != dev:
        raise RuntimeError("masked_attention: attn_mask must live on the GPU of q (no CPU fallback)")
    m = attn_mask.detach().contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _check(q, k, v, num_heads):
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        if t.dim() != 3:
            raise ValueError(f"masked_attention: {what} is (L, B, E), got {tuple(t.shape)}")
    Lq, B, E = q.shape
    if k.shape[1:] != (B, E) or v.shape != k.shape:
        raise ValueError(f"masked_attention: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not fit")
    if E != num_heads * HEAD_DIM:
        raise NotImplementedError(f"masked_attention: head dimension {E / num_heads:g} (E = {E}, {num_heads} heads); only "
                                  f"{HEAD_DIM} is built")
    if Lq == 0 or k.shape[0] == 0 or B == 0:
        raise ValueError("masked_attention: empty q / k")
    for t, what in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda:
            raise RuntimeError(f"masked_attention: {what} must live on the GPU (no CPU fallback)")


def masked_attention(q, k, v, num_heads, attn_mask=None, scale=None, arithmetic="fp32"):
    """``softmax(scale * q k^T + attn_mask) v`` per image and head (module docstring): ``q (Lq, B, E)``, ``k, v (Lk, B, E)`` ->
    ``(Lq, B, E)``, ``E = num_heads * 32``.  ``scale`` defaults to ``32 ** -0.5``.  ``arithmetic``: ``"fp32"`` or ``"operand"``
    (fp16 / bf16 operands of one dtype on the 16-bit MFMA)."""
    function = _function(arithmetic, q, k, v)
    mask = _byte_mask(attn_mask, q.shape[0], k.shape[0], q.device)
    _check(q, k, v, num_heads)
    scale = HEAD_DIM ** -0.5 if scale is None else float(scale)
    return function.apply(q, k, v, mask, num_heads, scale, False)


class MultiheadAttention(nn.Module):
    """Drop-in for the decoder layer's ``nn.MultiheadAttention(embed_dim, num_heads, dropout=0.0)``: the same parameters
    (``in_proj_weight (3E, E)``, ``in_proj_bias (3E)``, ``out_proj.weight``, ``out_proj.bias``) under the same names and the
    same ``_reset_parameters``; seq-first ``(L, B, E)`` tensors.

    ``forward`` returns ``(out, None)``: the reference takes ``[0]`` and never reads the head-averaged attention weights
    (transformer.py:810), so they are not computed whatever ``need_weights`` says.  With ``query is key`` (the layer's
    ``q = k = tgt + pos``) the in-projection is one GEMM for ``[q | k]`` and one for ``v``.

    ``arithmetic`` (``"fp32"`` / ``"operand"``, module docstring) is a plain attribute, no parameter or buffer: ``state_dict``
    keys are those of ``nn.MultiheadAttention``; it survives ``copy.deepcopy`` and pickling."""

    arithmetic = "fp32"                     # of instances pickled before the attribute existed

    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None,
                 vdim=None, batch_first=False, arithmetic="fp32"):
        super().__init__()
        self.arithmetic = _arithmetic(arithmetic)
        if add_bias_kv or add_zero_attn or batch_first:
            raise NotImplementedError("MultiheadAttention: add_bias_kv, add_zero_attn and batch_first are not built")
        if (kdim is not None and kdim != embed_dim) or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError("MultiheadAttention: kdim / vdim other than embed_dim are not built")
        if embed_dim != num_heads * HEAD_DIM:
            raise NotImplementedError(f"MultiheadAttention: head dimension {embed_dim / num_heads:g}; only {HEAD_DIM} is built")
        self.embed_dim, self.num_heads, self.dropout, self.head_dim = embed_dim, num_heads, float(dropout), HEAD_DIM
        self.batch_first = False
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            nn.init.constant_(self.in_proj_bias, 0.)
            nn.init.constant_(self.out_proj.bias, 0.)

    @classmethod
    def adopt(cls, mha, arithmetic="fp32"):
        """The mirror of a built ``nn.MultiheadAttention`` that holds the SAME ``Parameter`` objects (and ``out_proj`` module)."""
        reason = _why_not(mha)
        if reason:
            raise NotImplementedError(f"MultiheadAttention: {reason}")
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        new.arithmetic = _arithmetic(arithmetic)
        new.embed_dim, new.num_heads, new.dropout, new.head_dim = mha.embed_dim, mha.num_heads, float(mha.dropout), HEAD_DIM
        new.batch_first = False
        new.in_proj_weight = mha.in_proj_weight
        if mha.in_proj_bias is not None:
            new.in_proj_bias = mha.in_proj_bias
        else:
            new.register_parameter("in_proj_bias", None)
        new.out_proj = mha.out_proj
        new.train(mha.training)
        return new

    def __setstate__(self, state):
        super().__setstate__(state)
        self.arithmetic = _arithmetic(self.__dict__.get("arithmetic", "fp32"))

    def forward(self, query, key, value, attn_mask=None, need_weights=True, key_padding_mask=None):
        if key_padding_mask is not None:
            raise NotImplementedError("MultiheadAttention: key_padding_mask is not built")
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError("MultiheadAttention: attention dropout is not built (DINO builds its layers with 0.0)")
        E, W, b = self.embed_dim, self.in_proj_weight, self.in_proj_bias
        mask = _byte_mask(attn_mask, query.shape[0], key.shape[0], query.device)
        scale = HEAD_DIM ** -0.5
        if query is key:
            qk = F.linear(query, W[:2 * E], None if b is None else b[:2 * E])
            v = F.linear(value, W[2 * E:], None if b is None else b[2 * E:])
            _check(qk[..., :E], qk[..., E:], v, self.num_heads)
            out = _function(self.arithmetic, qk, v).apply(qk, v, None, mask, self.num_heads, scale, True)
        else:
            q = F.linear(query, W[:E], None if b is None else b[:E])
            k = F.linear(key, W[E:2 * E], None if b is None else b[E:2 * E])
            v = F.linear(value, W[2 * E:], None if b is None else b[2 * E:])
            _check(q, k, v, self.num_heads)
            out = _function(self.arithmetic, q, k, v).apply(q, k, v, mask, self.num_heads, scale, False)
        return self.out_proj(out), None


def _arithmetic(name):
    if name not in ARITHMETICS:
        raise ValueError(f"MultiheadAttention: arithmetic is one of {ARITHMETICS}, got {name!r}")
    return name


def _why_not(mha):
    """Why a ``nn.MultiheadAttention`` cannot be replaced by the mirror, or ``None``."""
    if not getattr(mha, "_qkv_same_embed_dim", True) or mha.in_proj_weight is None:
        return "kdim / vdim other than embed_dim"
    if mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
        return "bias_k / bias_v / add_zero_attn"
    if getattr(mha, "batch_first", False):
        return "batch_first"
    if mha.embed_dim != mha.num_heads * HEAD_DIM:
        return f"head dimension {mha.embed_dim / mha.num_heads:g}"
    if mha.dropout > 0.0:
        return "attention dropout"
    return None


def convert_self_attention(module, arithmetic="fp32"):
    """Replace, in place, every ``nn.MultiheadAttention`` below ``module`` that qualifies (embed_dim = 32 * heads, no dropout,
    seq-first, no bias_k / add_zero_attn) with ``MultiheadAttention.adopt`` of it: the same ``Parameter`` objects, so optimizer
    state, EMA pairs and ``state_dict`` keys are untouched.  ``arithmetic`` (``"fp32"`` / ``"operand"``) is set on what is
    converted.  Returns the number converted."""
    _arithmetic(arithmetic)
    done = 0
    for parent in list(module.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.MultiheadAttention and _why_not(child) is None:
                setattr(parent, name, MultiheadAttention.adopt(child, arithmetic))
                done += 1
    return done

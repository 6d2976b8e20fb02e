"""The transformer's position inputs on the MI355X (``csrc/pyramid_inputs.hip``): the pyramid's padding masks, the sine position
rows with the level row added, the valid ratios and the encoder's reference points.

For every forward pass the head builds ``img_masks`` from ``img_metas`` and runs ``F.interpolate(...).to(bool)`` and
``SinePositionalEncodingHW`` per level (dino_detr_ssod_head.py:351-377, positional_encoding.py:57-99); the transformer flattens,
transposes, adds ``level_embed[lvl]`` and concatenates (transformer.py:1271-1289), runs ``get_valid_ratio`` per level (:1237-1244,
1292) and the encoder ``get_reference_points`` (:676-691).  In stock torch that is one small launch per op and level (counted: profiles/pyramid_inputs_probe.txt).  Here
it is two launches forward for the whole pyramid and batch and two backward, on the current stream, no host synchronisation, no
memset, no staging copies (the image sizes travel by value in the parameter block), bitwise reproducible:

``pyramid_inputs(img_shapes, batch_input_shape, shapes, positional_encoding, level_embed=None, ...)``   from the image sizes
``pyramid_inputs_from_masks(mlvl_masks, positional_encoding, level_embed=None, ...)``                   from given level masks
``SinePositionalEncodingHW``                     the reference's module: kwargs, attributes, ``__repr__``, ``forward(mask)``
``head_inputs(head, mlvl_feats_shapes, img_metas)``   the call the head's ``forward`` makes in place of lines 351-377

Both return ``PyramidInputs(pos, mask_flatten, valid_ratios, reference_points, spatial_shapes, level_start_index, mlvl_masks)``:
``pos`` ``(N, S, 256)`` is the reference's ``lvl_pos_embed_flatten`` -- complete token rows in ``project_pyramid``'s order, the
``level_embed`` row added -- in fp32 (the reference's encoding is fp32 and promotes the sum) or the 16-bit ``dtype`` asked for,
rounded once; ``mask_flatten`` ``(N, S)`` bool with ``mlvl_masks`` its per-level ``(N, h, w)`` views; ``valid_ratios``
``(N, L, 2)`` fp32 in ``[w, h]`` order from the first row and first column of each level mask (count times the fp32 reciprocal
of the side: torch's division of a GPU tensor by a Python number); ``reference_points``
``(N, S, L, 2)`` fp32, what ``DINOTransformerEncoder.get_reference_points`` returns (``None`` unless asked for), for
``add_norm.encoder_forward(..., reference_points=)``.  Only ``level_embed`` is differentiable; its gradient has its dtype.

The two ``dim_t`` tables are built once per device, temperature and ``num_feats`` by torch with the reference's own expression;
the kernels read them and evaluate no ``pow``.

Not built: ``num_feats`` other than 128, more than 8 levels, more than 64 images per call, levels with a
side of 65536 or more, ``normalize`` with ``eps <= 0``.
"""
import collections
import ctypes
import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .input_proj import pyramid_index

MAX_LEVELS, MAX_BATCH = _lib.PYR_MAX_LEVELS, _lib.PYR_MAX_BATCH
NUM_FEATS, CHANNELS = 128, 256
_F32 = torch.float32
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_tables = {}                      # (device, temperature, num_feats) -> dim_t

PyramidInputs = collections.namedtuple(
    "PyramidInputs", "pos mask_flatten valid_ratios reference_points spatial_shapes level_start_index mlvl_masks")
Settings = collections.namedtuple("Settings", "temperatureH temperatureW normalize scale eps offset")


def dim_t(device, temperature, num_feats=NUM_FEATS):
    """The divisors of one half of the encoding, computed once per device, temperature and ``num_feats`` with the reference's
    own expression (positional_encoding.py:81-87); the kernels read this table."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, temperature, num_feats)
    hit = _tables.get(key)
    if hit is None:
        with torch.no_grad():
            t = torch.arange(num_feats, dtype=_F32, device=device)
            hit = _tables[key] = (temperature ** (2 * (t // 2) / num_feats)).contiguous()
    return hit


def nearest_source_index(dst, in_size, out_size):
    """``F.interpolate(mode="nearest")``'s source index of destination index ``dst``, in fp32 as the kernel evaluates it:
    ``min(int(floorf(dst * (float(in) / out))), in - 1)``.  Host-side statement of the rule (tests compare it with torch)."""
    import numpy as np
    ratio = np.float32(in_size) / np.float32(out_size)
    return min(int(np.floor(np.float32(dst) * ratio)), in_size - 1)


def level_mask(img_h, img_w, input_h, input_w, h, w):
    """The ``(h, w)`` level mask of one image by the rule above, as nested lists of bool (host-side; the kernel's statement)."""
    rows = [nearest_source_index(i, input_h, h) >= img_h for i in range(h)]
    cols = [nearest_source_index(j, input_w, w) >= img_w for j in range(w)]
    return [[r or c for c in cols] for r in rows]


def _settings(positional_encoding):
    """The settings of a ``SinePositionalEncodingHW`` (the reference's or the mirror below), checked."""
    pe = positional_encoding
    if pe.num_feats != NUM_FEATS:
        raise NotImplementedError(f"pyramid_inputs: num_feats={pe.num_feats} (only {NUM_FEATS} is built: 256-channel token rows)")
    normalize = bool(pe.normalize)
    if normalize and not float(pe.eps) > 0:
        raise NotImplementedError(f"pyramid_inputs: normalize with eps={pe.eps} (eps > 0 is built)")
    return Settings(pe.temperatureH, pe.temperatureW, normalize, float(pe.scale), float(pe.eps), float(pe.offset))


def _check(batch, shapes, level_embed, dtype, device, what):
    if not 1 <= len(shapes) <= MAX_LEVELS:
        raise NotImplementedError(f"{what}: {len(shapes)} levels (1 .. {MAX_LEVELS})")
    if not 1 <= batch <= MAX_BATCH:
        raise NotImplementedError(f"{what}: {batch} images (1 .. {MAX_BATCH}: the image sizes travel by value in the parameter block)")
    if device.type != "cuda":
        raise NotImplementedError(f"{what}: the levels must live on the GPU, not on {device} (no CPU fallback)")
    for l, (h, w) in enumerate(shapes):
        if not (1 <= h < 65536 and 1 <= w < 65536):
            raise NotImplementedError(f"{what}: level {l} is {(h, w)}; sides of 1 .. 65535 are built (16-bit counts)")
    if dtype not in _DTYPES:
        raise NotImplementedError(f"{what}: dtype {dtype}; float32, float16 and bfloat16 are built")
    if level_embed is not None:
        if level_embed.dim() != 2 or level_embed.shape[0] < len(shapes) or level_embed.shape[1] != CHANNELS \
                or level_embed.device != device or level_embed.dtype not in _DTYPES:
            raise ValueError(f"{what}: level_embed is {tuple(level_embed.shape)} {level_embed.dtype} on {level_embed.device}; "
                             f"expected (>= {len(shapes)}, {CHANNELS}) of float32, float16 or bfloat16 on {device}")
    rows = sum(h * w for h, w in shapes)
    if batch * rows * CHANNELS >= 2 ** 31:
        raise ValueError(f"{what}: too large (batch * rows * 256 < 2^31)")


def _block(batch, shapes):
    p = _lib.PyramidInputsBlock()
    p.batch, p.levels = batch, len(shapes)
    start = 0
    for l, (h, w) in enumerate(shapes):
        p.h[l], p.w[l], p.start[l] = h, w, start
        start += h * w
    p.tokens_per_image = start
    return p


def _workspace(p, backward, dev):
    nbytes = _lib.lib().semidetr_pyramid_inputs_workspace_bytes(ctypes.byref(p), int(backward))
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev), nbytes


def _forward(sizes, masks, shapes, cfg, level_embed, dtype, want_reference_points, dev):
    """The two forward launches alone, without autograd: ``(pos, mask_flatten, valid_ratios, reference_points)``.  ``sizes``:
    ``(batch_input_shape, img_shapes)`` on the host, or ``None`` with ``masks``: one contiguous ``(N, h, w)`` bool / uint8
    tensor per level."""
    batch = len(sizes[1]) if sizes is not None else masks[0].shape[0]
    p = _block(batch, shapes)
    rows, levels = p.tokens_per_image, len(shapes)
    if sizes is not None:
        p.from_sizes, (p.input_h, p.input_w) = 1, sizes[0]
        for n, (img_h, img_w) in enumerate(sizes[1]):
            p.img_h[n], p.img_w[n] = img_h, img_w
    else:
        for l, m in enumerate(masks):
            p.masks[l] = m.data_ptr()
    p.normalize, p.offset, p.eps, p.scale = int(cfg.normalize), cfg.offset, cfg.eps, cfg.scale
    ty, tx = dim_t(dev, cfg.temperatureH), dim_t(dev, cfg.temperatureW)
    p.dim_ty, p.dim_tx = ty.data_ptr(), tx.data_ptr()
    le = None
    if level_embed is not None:
        le = level_embed.detach()
        if not le.is_contiguous() or le.data_ptr() % 16:
            le = le.clone(memory_format=torch.contiguous_format)
        p.level_embed, p.level_embed_type = le.data_ptr(), _lib.row_type(le.dtype)
    pos = torch.empty((batch, rows, CHANNELS), dtype=dtype, device=dev)
    mask_flatten = torch.empty((batch, rows), dtype=torch.bool, device=dev)
    valid_ratios = torch.empty((batch, levels, 2), dtype=_F32, device=dev)
    ref = torch.empty((batch, rows, levels, 2), dtype=_F32, device=dev) if want_reference_points else None
    p.pos, p.pos_type, p.mask_flatten, p.valid_ratios = pos.data_ptr(), _lib.row_type(dtype), mask_flatten.data_ptr(), valid_ratios.data_ptr()
    if ref is not None:
        p.reference_points = ref.data_ptr()
    work, nbytes = _workspace(p, False, dev)
    _lib.call("semidetr_pyramid_inputs_forward", dev, ctypes.byref(p), work, nbytes)
    return pos, mask_flatten, valid_ratios, ref


def pyramid_inputs_backward(g, shapes, level_embed_dtype=_F32):
    """The two backward launches alone: the ``(levels, 256)`` gradient of ``level_embed`` in ``level_embed_dtype`` from the
    upstream gradient ``g`` ``(N, S, 256)`` of ``pos`` (fp32, fp16 or bf16, read in place through its strides)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    _check(g.shape[0], shapes, None, level_embed_dtype, g.device, "pyramid_inputs_backward")
    p = _block(g.shape[0], shapes)
    if g.dim() != 3 or tuple(g.shape[1:]) != (p.tokens_per_image, CHANNELS) or g.dtype not in _DTYPES:
        raise ValueError(f"pyramid_inputs_backward: g is {tuple(g.shape)} {g.dtype}; expected (N, {p.tokens_per_image}, {CHANNELS}) "
                         "of float32, float16 or bfloat16")
    gr = _lib.rows_native(g)
    _lib.set_rows(p, "g", gr)
    grad = torch.empty((len(shapes), CHANNELS), dtype=level_embed_dtype, device=g.device)
    p.g_type, p.level_embed_type, p.grad_level_embed = _lib.row_type(gr.dtype), _lib.row_type(level_embed_dtype), grad.data_ptr()
    work, nbytes = _workspace(p, True, g.device)
    _lib.call("semidetr_pyramid_inputs_backward", g.device, ctypes.byref(p), work, nbytes)
    return grad


class PyramidInputsFunction(torch.autograd.Function):
    """``apply(level_embed, sizes, masks, shapes, cfg, dtype, want_reference_points, device)`` -> ``(pos, mask_flatten,
    valid_ratios[, reference_points])``.  Only ``level_embed`` (a tensor or ``None``) is differentiable: its gradient is the sum
    of ``pos``'s over the images and the level's rows."""

    @staticmethod
    def forward(ctx, level_embed, sizes, masks, shapes, cfg, dtype, want_reference_points, device):
        pos, mask_flatten, valid_ratios, ref = _forward(sizes, masks, shapes, cfg, level_embed, dtype, want_reference_points, device)
        ctx.shapes = shapes
        ctx.embed = None if level_embed is None else (level_embed.shape[0], level_embed.dtype)
        ctx.set_materialize_grads(False)
        rest = (mask_flatten, valid_ratios) + (() if ref is None else (ref,))
        ctx.mark_non_differentiable(*rest)
        return (pos,) + rest

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *ignored):
        none = (None,) * 8
        if g is None or ctx.embed is None or not ctx.needs_input_grad[0]:
            return none
        rows, dtype = ctx.embed
        grad = pyramid_inputs_backward(g, ctx.shapes, dtype)
        if rows > grad.shape[0]:                     # rows of level_embed no level of this pyramid uses
            grad = torch.cat((grad, grad.new_zeros((rows - grad.shape[0], CHANNELS))))
        return (grad,) + none[1:]


def _result(out, shapes, want_reference_points, device):
    pos, mask_flatten, valid_ratios = out[:3]
    ref = out[3] if want_reference_points else None
    spatial_shapes, level_start_index = pyramid_index(shapes, device)
    mlvl_masks, start = [], 0
    for h, w in shapes:
        mlvl_masks.append(mask_flatten[:, start:start + h * w].unflatten(1, (h, w)))
        start += h * w
    return PyramidInputs(pos, mask_flatten, valid_ratios, ref, spatial_shapes, level_start_index, mlvl_masks)


def pyramid_inputs(img_shapes, batch_input_shape, shapes, positional_encoding, level_embed=None, dtype=None,
                   want_reference_points=False, device=None):
    """The position inputs of a batch from its image sizes.  ``img_shapes``: a host list of ``(img_h, img_w)`` (further entries,
    such as the channel count of ``img_metas[i]['img_shape']``, are ignored); ``batch_input_shape``: the padded ``(H, W)``;
    ``shapes``: the levels' ``(h, w)``; ``positional_encoding``: a ``SinePositionalEncodingHW`` (its settings are read);
    ``level_embed``: ``(levels, 256)`` or ``None`` (no level row); ``dtype``: of ``pos`` (default fp32); ``device``: where the
    results live (default: ``level_embed``'s, else the current GPU)."""
    what = "pyramid_inputs"
    shapes = [(int(s[0]), int(s[1])) for s in shapes]
    sizes = [(int(s[0]), int(s[1])) for s in img_shapes]
    input_h, input_w = int(batch_input_shape[0]), int(batch_input_shape[1])
    if device is None:
        device = level_embed.device if level_embed is not None else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    cfg = _settings(positional_encoding)
    _check(len(sizes), shapes, level_embed, dtype or _F32, device, what)
    if input_h < 1 or input_w < 1:
        raise ValueError(f"{what}: batch_input_shape {(input_h, input_w)}")
    for n, (img_h, img_w) in enumerate(sizes):
        if not (0 <= img_h <= input_h and 0 <= img_w <= input_w):
            raise ValueError(f"{what}: image {n} is {(img_h, img_w)}, outside batch_input_shape {(input_h, input_w)}")
    out = PyramidInputsFunction.apply(level_embed, ((input_h, input_w), sizes), None, shapes, cfg, dtype or _F32,
                                      want_reference_points, device)
    return _result(out, shapes, want_reference_points, device)


def pyramid_inputs_from_masks(mlvl_masks, positional_encoding, level_embed=None, dtype=None, want_reference_points=False):
    """The same from given level masks: a list of ``(N, h, w)`` bool or uint8 tensors, non-zero = masked; rectangles are not
    assumed.  The returned ``mlvl_masks`` are views of the new ``mask_flatten``."""
    what = "pyramid_inputs_from_masks"
    mlvl_masks = list(mlvl_masks)
    if not mlvl_masks:
        raise NotImplementedError(f"{what}: 0 levels (1 .. {MAX_LEVELS})")
    m0 = mlvl_masks[0]
    for l, m in enumerate(mlvl_masks):
        if m.dim() != 3 or m.dtype not in (torch.bool, torch.uint8) or m.shape[0] != m0.shape[0] or m.device != m0.device:
            raise ValueError(f"{what}: level {l} is {tuple(m.shape)} {m.dtype} on {m.device}; the levels are (N, h, w) bool or uint8 "
                             "tensors of one batch on one device")
    shapes = [(int(m.shape[1]), int(m.shape[2])) for m in mlvl_masks]
    cfg = _settings(positional_encoding)
    _check(m0.shape[0], shapes, level_embed, dtype or _F32, m0.device, what)
    masks = [m if m.is_contiguous() else m.contiguous() for m in mlvl_masks]
    out = PyramidInputsFunction.apply(level_embed, None, masks, shapes, cfg, dtype or _F32, want_reference_points, m0.device)
    return _result(out, shapes, want_reference_points, m0.device)


class SinePositionalEncodingHW(nn.Module):
    """The reference's ``SinePositionalEncodingHW`` (positional_encoding.py:10-110): same constructor arguments, attributes and
    ``__repr__``; no parameters.  ``forward(mask)`` is a one-level call of the op without a level row; the head calls
    ``head_inputs`` instead, which builds every level at once."""

    def __init__(self, num_feats, temperatureH=10000, temperatureW=10000, normalize=False, scale=2 * math.pi, eps=1e-6,
                 offset=0., init_cfg=None):
        super().__init__()
        if normalize and not isinstance(scale, (float, int)):
            raise AssertionError(f"normalize=True needs a float or int scale, found {type(scale)}")
        self.num_feats, self.normalize, self.scale, self.eps, self.offset = num_feats, normalize, scale, eps, offset
        self.temperatureH, self.temperatureW = temperatureH, temperatureW
        self.init_cfg = init_cfg

    def forward(self, mask):
        """``mask`` ``(bs, h, w)``, non-zero = ignored -> ``(bs, 2 * num_feats, h, w)`` fp32, the permuted view of the token rows."""
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask != 0
        pos = pyramid_inputs_from_masks([mask], self).pos
        return pos.unflatten(1, (mask.shape[1], mask.shape[2])).permute(0, 3, 1, 2)

    def __repr__(self):
        return (f"{self.__class__.__name__}(num_feats={self.num_feats}, temperatureH={self.temperatureH}, "
                f"temperatureW={self.temperatureW}, normalize={self.normalize}, scale={self.scale}, eps={self.eps})")


def head_inputs(head, mlvl_feats_shapes, img_metas, dtype=None, want_reference_points=True):
    """What dino_detr_ssod_head.py:351-377 and transformer.py:1271-1292 build from ``img_metas``: ``batch_input_shape`` of the
    first image, ``img_shape`` of each, ``head.positional_encoding`` and ``head.transformer.level_embed`` -- the latter only
    where the transformer adds it (``num_feature_levels > 1 and level_embed is not None``).  ``mlvl_feats_shapes``: the ``(h, w)``
    of all ``num_feature_levels`` levels, the extra ones included (``project_pyramid`` returns them as ``spatial_shapes``'
    host list; ``[src.shape[-2:] for src in srcs]`` is the same)."""
    input_img_h, input_img_w = img_metas[0]['batch_input_shape']
    img_shapes = [meta['img_shape'][:2] for meta in img_metas]
    transformer = head.transformer
    level_embed = getattr(transformer, "level_embed", None)
    if not (getattr(transformer, "num_feature_levels", len(mlvl_feats_shapes)) > 1 and level_embed is not None):
        level_embed = None
    device = level_embed.device if level_embed is not None else next(head.parameters()).device
    return pyramid_inputs(img_shapes, (input_img_h, input_img_w), mlvl_feats_shapes, head.positional_encoding, level_embed,
                          dtype=dtype, want_reference_points=want_reference_points, device=device)

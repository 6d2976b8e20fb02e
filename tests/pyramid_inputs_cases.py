"""The cases of the pyramid-inputs tests (semi_detr_amd.pyramid_inputs, csrc/pyramid_inputs.hip): the smallest shapes at which
the kernels can go wrong.  Shared by tests/test_pyramid_inputs_ref.py (CPU), tests/test_gpu_pyramid_inputs.py and
tools/gen_pyramid_inputs_golden.py.

Test helper (not a conftest; imported by name).  Numpy only.  A case is a dict:

  ``img_shapes`` / ``input`` / ``shapes``   from image sizes: ``[(img_h, img_w)]``, ``batch_input_shape``, the levels' ``(h, w)``
  ``masks``                                 given masks instead: one ``(N, h, w)`` bool array per level (``img_shapes`` is None)
  ``enc``                                   the keyword arguments of the positional encoding (``num_feats`` = 128)
  ``level_embed`` / ``le_dtype``            ``(L, 256)`` fp32 array holding values of ``le_dtype``, or None
  ``dtype``                                 of ``pos``;  ``g`` / ``g_dtype``: the upstream gradient ``(N, S, 256)`` of ``pos``

The kernels' tiles: 64 columns / rows per scan wave, 32 token rows per emit workgroup, 256 rows per backward slot, 4 parts in
the final sum.

  padded_batch   batch_input_shape (67, 93), levels (9,12) (5,6) (3,3) (2,2), images full size, (41, 93), (5, 7): a valid extent
                 of one pixel on the coarse levels, levels smaller than a tile, a first level (108 rows) that is no multiple of 32.
  exact_product  the same pyramid with image widths on both sides of 31 and 62: at 93 -> 12 the fp32 product 4 * 7.75 is the
                 exact integer 31 (8 * 7.75 = 62).  At 1333 -> 167 / 84 / 42 / 21 and 37 -> 5 / 3 / 2 no destination index gives an
                 exact integer (tests/test_pyramid_inputs_ref.py checks that), so the exact product is taken here.
  real_divisor   batch_input_shape (1333, 37), levels (167,5) (84,3) (42,2) (21,1), 1192 rows: floorf(50 * fp32(1333 / 167)) = 399
                 and floorf(25 * fp32(1333 / 84)) = 396, image heights 399 | 400 and 396 | 397 lie on both sides of those steps.
  wide_tall      levels (3, 130) and (130, 3): scans of three waves' width, from sizes and (``wide_tall_masks``) from random masks.
  five_levels, one_level (no level row), and the given masks: ``masks_random`` (about 30 % masked), ``masks_row_col`` (a fully
  masked row and column, holes in row 0 and column 0), ``masks_all_valid``, ``masks_one_full`` (image 1 fully masked: valid
  ratios 0, reference points non-finite).
  Settings: ``no_normalize`` (N = 1), ``offset_temps`` (offset -0.5, temperatureH != temperatureW), ``no_level_embed``,
  ``pos_fp16`` / ``pos_bf16`` (16-bit pos and g; bf16 level_embed), ``g_fp16`` / ``g_bf16`` (fp32 pos, 16-bit g).
"""
import numpy as np

NUM_FEATS, C = 128, 256
DEFAULT = dict(num_feats=NUM_FEATS, temperatureH=20, temperatureW=20, normalize=True)     # the DINO configs' settings
PADDED = dict(input=(67, 93), shapes=[(9, 12), (5, 6), (3, 3), (2, 2)])
# sizes at which the host-side nearest rule is compared with F.interpolate for every image height: (input, outputs)
NEAREST_SIZES = ((800, (100, 50, 25, 13)), (1333, (167, 84, 42, 21)), (1199, (150,)), (37, (5, 3)), (7, (7,)), (9, (2,)))


def round_to(a, dtype):
    """fp32 array holding the values of ``dtype`` ("fp32", "fp16", "bf16") nearest to ``a`` (round to nearest even)"""
    a = np.asarray(a, np.float32)
    if dtype == "fp32":
        return a
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32)


def rows_of(shapes):
    return int(sum(h * w for h, w in shapes))


def _case(name, rng, shapes, img_shapes=None, input=None, masks=None, enc=None, level_embed=True, le_dtype="fp32", dtype="fp32",
          g_dtype=None):
    n = len(img_shapes) if img_shapes is not None else masks[0].shape[0]
    le = round_to(rng.standard_normal((len(shapes), C)), le_dtype) if level_embed and len(shapes) > 1 else None
    g_dtype = g_dtype or dtype
    return dict(name=name, shapes=[tuple(s) for s in shapes], img_shapes=img_shapes, input=input, masks=masks,
                enc=dict(DEFAULT, **(enc or {})), level_embed=le, le_dtype=le_dtype, dtype=dtype, g_dtype=g_dtype,
                g=round_to(rng.standard_normal((n, rows_of(shapes), C)), g_dtype))


def _random_masks(rng, n, shapes, share=0.3):
    return [rng.random((n, h, w)) < share for h, w in shapes]


_cache = None


def cases():
    """{name: case}; built once, the arrays must be left unchanged"""
    global _cache
    if _cache is not None:
        return _cache
    rng = np.random.default_rng(20240911)
    out = {}

    def add(name, *a, **kw):
        out[name] = _case(name, rng, *a, **kw)

    add("padded_batch", PADDED["shapes"], [(67, 93), (41, 93), (5, 7)], PADDED["input"])
    add("exact_product", PADDED["shapes"], [(67, 31), (67, 32), (30, 62), (30, 63)], PADDED["input"])
    add("real_divisor", [(167, 5), (84, 3), (42, 2), (21, 1)], [(399, 37), (400, 37), (396, 20), (397, 1)], (1333, 37))
    add("wide_tall", [(3, 130), (130, 3)], [(200, 131), (260, 260), (1, 1)], (260, 260))
    add("wide_tall_masks", [(3, 130), (130, 3)], masks=_random_masks(rng, 2, [(3, 130), (130, 3)]))
    add("five_levels", [(16, 12), (8, 6), (4, 3), (2, 2), (1, 1)], [(128, 96), (100, 50)], (128, 96))
    add("one_level", [(6, 7)], [(48, 56), (30, 29)], (48, 56))
    sh = [(9, 12), (5, 6), (3, 3)]
    add("masks_random", sh, masks=_random_masks(rng, 2, sh))
    m = [np.zeros((2, h, w), bool) for h, w in sh]
    m[0][0, 2, :] = True                                   # a fully masked row and a fully masked column
    m[0][0, :, 3] = True
    m[0][1, 0, [1, 5, 6]] = True                           # holes in row 0 and column 0: the counts differ from the extents
    m[0][1, [2, 3], 0] = True
    m[1][1, 0, 2] = True
    add("masks_row_col", sh, masks=m)
    add("masks_all_valid", sh, masks=[np.zeros((2, h, w), bool) for h, w in sh])
    m = _random_masks(rng, 2, sh, 0.2)
    for lvl in m:
        lvl[1] = True                                      # image 1 fully masked
    add("masks_one_full", sh, masks=m)
    add("no_normalize", PADDED["shapes"], [(50, 70)], PADDED["input"], enc=dict(normalize=False))
    add("offset_temps", sh, masks=_random_masks(rng, 2, sh), enc=dict(offset=-0.5, temperatureH=20, temperatureW=10000))
    add("no_level_embed", PADDED["shapes"], [(67, 93), (33, 47)], PADDED["input"], level_embed=False)
    add("pos_fp16", PADDED["shapes"], [(67, 93), (41, 60)], PADDED["input"], dtype="fp16")
    add("pos_bf16", PADDED["shapes"], [(67, 93), (41, 60)], PADDED["input"], dtype="bf16", le_dtype="bf16")
    add("g_fp16", sh, masks=_random_masks(rng, 2, sh), g_dtype="fp16")
    add("g_bf16", sh, masks=_random_masks(rng, 1, sh), g_dtype="bf16")
    _cache = out
    return out


def names():
    return list(cases())

"""The cases of the reference-point kernels (csrc/ref_points.hip), shared by tests/test_ref_points_ref.py (CPU) and
tests/test_gpu_ref_points.py: the smallest shapes at which the kernels can still go wrong.  A wave takes 8 rows, so ``nq * bs``
of 1, 3, 6, 130, 195 and 390 covers a lone partial wave, full waves and a ragged last wave; widths 2 and 4; 1, 4 and 5 levels;
coordinates exactly at 0, 1, 0.5 (argument about pi), 0.25, eps and 1 - eps; deltas of +-inf, NaN, +-88 and 0; valid ratios of
exactly 1 and inside (0.5, 1); fp32, fp16 and bf16 operands (alone and mixed); contiguous rows, the head's transposed rows and a
slice of a NaN-filled wider buffer; 1, 6 and 8 segments of unequal row counts.

Every array is float32 numpy holding numbers its dtype represents exactly; ``layout`` and the dtypes say how the GPU test lays
them out.  The random coordinates are sigmoids of unit normals, the upstream gradients fp32-exact pseudo-random numbers in
[-2, 2).
"""
import functools

import numpy as np
import torch

NONE, SIGMOID, REFINE = 0, 1, 2
EPS = 1e-5
EPS32 = float(np.float32(EPS))
TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def as_dtype(a, dtype):
    """float32 numpy rounded to the numbers of ``dtype``"""
    a = np.asarray(a, np.float32)
    return a if dtype == "fp32" else torch.from_numpy(a).to(TORCH[dtype]).float().numpy()


def promoted(mode, delta_dtype, ref_dtype):
    """the dtype torch's promotion gives the refined points outside autocast"""
    if mode != REFINE:
        return ref_dtype
    return ref_dtype if delta_dtype == ref_dtype else "fp32"


def grad_pattern(shape, salt, dtype="fp32"):
    n = int(np.prod(shape))
    i = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) % np.uint64(2 ** 32)
    g = (((i >> np.uint64(16)).astype(np.float64) - 32768.0) / 16384.0).astype(np.float32).reshape(shape)
    return as_dtype(g, dtype)


def table():
    """the 128 divisors with the reference's own expression (transformer.py:471-472), on the CPU"""
    t = torch.arange(128, dtype=torch.float32)
    return (10000 ** (2 * (t // 2) / 128)).numpy()


SPECIAL_COORDS = (0.0, 1.0, 0.5, 0.25, EPS32, float(np.float32(1.0) - np.float32(EPS32)))
SPECIAL_DELTAS = (np.inf, -np.inf, np.nan, 88.0, -88.0, 0.0)


def _coords(rng, shape, special):
    c = (1.0 / (1.0 + np.exp(-rng.standard_normal(shape)))).astype(np.float32)
    if special:
        flat = c.reshape(-1)
        for k, v in enumerate(SPECIAL_COORDS * 2):          # every special value at an even and an odd coordinate
            flat[(k * 5 + k // len(SPECIAL_COORDS)) % flat.size] = v
    return c


def _deltas(rng, shape, special):
    d = rng.standard_normal(shape).astype(np.float32)
    if special:
        flat = d.reshape(-1)
        for k, v in enumerate(SPECIAL_DELTAS):
            flat[(k * 7 + 3) % flat.size] = v
    return d


def _case(mode, width, rows, levels=0, dtypes=("fp32", "fp32"), layout="contiguous", seed=0, special=False, ratio_one=False,
          random_only=False):
    """``rows``: one (nq, bs) per segment; ``levels`` > 0 adds valid ratios (bs, levels, 2), scale and embed"""
    rng = np.random.default_rng(seed)
    delta_dtype, ref_dtype = dtypes
    out_dtype = promoted(mode, delta_dtype, ref_dtype)
    segments = []
    for s, (nq, bs) in enumerate(rows):
        shape = (nq, bs, width)
        if mode == SIGMOID:                                   # ref holds the unsigmoided points
            ref = _deltas(rng, shape, special)
        else:
            ref = _coords(rng, shape, special)
        seg = {"ref": as_dtype(ref, ref_dtype), "g_new": grad_pattern(shape, 17 + s, out_dtype)}
        if mode == REFINE:
            seg["delta"] = as_dtype(_deltas(rng, shape, special), delta_dtype)
        segments.append(seg)
    case = {"mode": mode, "width": width, "eps": EPS, "segments": segments, "delta_dtype": delta_dtype, "ref_dtype": ref_dtype,
            "out_dtype": out_dtype, "layout": layout, "random_only": random_only and not special, "dim_t": table(), "vr": None}
    if levels:
        nq, bs = rows[0]
        vr = np.ones((bs, levels, 2), np.float32) if ratio_one else (0.5 + 0.5 * rng.random((bs, levels, 2))).astype(np.float32)
        if not ratio_one and bs > 1:
            vr[0] = 1.0                                       # an image without padding next to padded ones
        case.update(vr=vr, g_ref_input=grad_pattern((nq, bs, levels, width), 5), g_embed=grad_pattern((nq, bs, 128 * width), 9))
    return case


@functools.lru_cache(maxsize=None)
def cases():
    c = {
        # the launch in front of layer 0: sigmoid + scale + embed
        "sigmoid_q1_b1_l1_w4": _case(SIGMOID, 4, [(1, 1)], 1, seed=1, ratio_one=True),
        "sigmoid_q3_b2_l4_w4_special": _case(SIGMOID, 4, [(3, 2)], 4, seed=2, special=True),
        "sigmoid_q65_b3_l5_w2": _case(SIGMOID, 2, [(65, 3)], 5, seed=3, random_only=True),
        "sigmoid_q130_b3_l4_w4": _case(SIGMOID, 4, [(130, 3)], 4, seed=4, random_only=True),
        "sigmoid_q65_b2_l4_w4_bf16": _case(SIGMOID, 4, [(65, 2)], 4, ("fp32", "bf16"), seed=5),
        # the launch between two layers: refine + scale + embed
        "refine_q65_b2_l4_w4": _case(REFINE, 4, [(65, 2)], 4, seed=6, random_only=True),
        "refine_q3_b3_l5_w4_special": _case(REFINE, 4, [(3, 3)], 5, seed=7, special=True),
        "refine_q130_b1_l1_w2_special": _case(REFINE, 2, [(130, 1)], 1, seed=8, special=True, ratio_one=True),
        "refine_q65_b3_l4_w4_slice": _case(REFINE, 4, [(65, 3)], 4, seed=9, layout="slice", special=True),
        "refine_q65_b2_l4_w4_fp16": _case(REFINE, 4, [(65, 2)], 4, ("fp16", "fp16"), seed=10, special=True),
        "refine_q65_b2_l4_w4_bf16": _case(REFINE, 4, [(65, 2)], 4, ("bf16", "bf16"), seed=11, special=True),
        "refine_q65_b2_l4_w4_fp16_fp32": _case(REFINE, 4, [(65, 2)], 4, ("fp16", "fp32"), seed=12),
        "refine_q3_b2_l4_w2_fp32_bf16": _case(REFINE, 2, [(3, 2)], 4, ("fp32", "bf16"), seed=13, special=True),
        # the launch after the last layer and the head's loop: refine alone, segments
        "refine_q130_b3_w4_transposed": _case(REFINE, 4, [(130, 3)], seed=14, layout="transposed", special=True),
        "refine_6_segments_w4_transposed": _case(REFINE, 4, [(65, 2), (3, 1), (130, 3), (1, 1), (8, 2), (9, 3)], seed=15,
                                                 layout="transposed", special=True),
        "refine_8_segments_w2_slice": _case(REFINE, 2, [(1, 1), (65, 2), (3, 3), (16, 1), (130, 2), (7, 1), (5, 3), (64, 1)], seed=16,
                                            layout="slice", special=True),
        "refine_6_segments_w4_bf16": _case(REFINE, 4, [(65, 2)] * 3 + [(3, 3), (1, 2), (130, 1)], dtypes=("bf16", "fp32"), seed=17),
        "refine_q130_b2_w4_random": _case(REFINE, 4, [(130, 2)], seed=18, random_only=True),
        # reference_inputs / gen_sineembed_for_position: scale + embed of given points
        "none_q65_b2_l4_w4_special": _case(NONE, 4, [(65, 2)], 4, seed=19, special=True),
        "none_q130_b3_l1_w2_one": _case(NONE, 2, [(130, 3)], 1, seed=20, special=True, ratio_one=True),
        "none_q3_b1_l5_w4_fp16": _case(NONE, 4, [(3, 1)], 5, ("fp32", "fp16"), seed=21, special=True),
    }
    return c


def names():
    return list(cases())


def random_names():
    return [k for k, v in cases().items() if v["random_only"]]


def fp32_names():
    return [k for k, v in cases().items() if v["delta_dtype"] == v["ref_dtype"] == "fp32"]

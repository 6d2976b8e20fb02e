"""Inputs of the exact MSDA backward's tests (tests/test_gpu_msda_exact.py on the GPU, tests/test_msda_exact_ref.py for the
model), D = 32 throughout, built from seeds with numpy.  Test helper, not a conftest.  A case is a dict of numpy arrays:
shapes (L, 2) int64, value (N, S, M, 32), loc (N, Lq, M, L, P, 2), attn (N, Lq, M, L, P), gout (N, Lq, M * 32), and `pixels`
(the queries are the pyramid's pixels in order: SEMIDETR_MSDA_QUERIES_ARE_PIXELS may be set).  Sizes are the smallest at which the
pipeline takes every path: several (image, head) slices, rows without entries, off-map samples and edge corners, both gathers'
instantiations (L * P = 16 and 20 with the pixel flag, the strips gather otherwise), and one row longer than the reduce kernel's
split length."""
import os
import re

import numpy as np

D = 32
PYR = [(6, 8), (3, 4), (2, 2), (1, 1)]                 # S = 65
PYR5 = [(6, 8), (3, 4), (2, 2), (1, 2), (1, 1)]        # S = 67


def split_len():
    """kSplitLen of the reduce kernel, as the implementation names it (semi-detr_amd/csrc/msda_exact.h)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "semi-detr_amd", "csrc", "msda_exact.h")).read()
    return int(re.search(r"constexpr int kSplitLen = (\d+);", src).group(1))


def _softmaxed(rng, N, Lq, M, L, P):
    lg = rng.normal(0, 2, (N, Lq, M, L * P))
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P).astype(np.float32)


def _pixel_centres(levels):
    return np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                           for h, w in levels])


def _case(levels, N, M, Lq, P, seed, loc=None, pixels=False):
    rng = np.random.default_rng(seed)
    shapes = np.asarray(levels, np.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    L = len(levels)
    value = (rng.standard_normal((N, S, M, D)) * 10.0 ** rng.integers(-2, 2, (1, 1, M, 1))).astype(np.float32)
    if loc is None:
        loc = rng.uniform(-0.1, 1.1, (N, Lq, M, L, P, 2))
    attn = _softmaxed(rng, N, Lq, M, L, P)
    gout = rng.standard_normal((N, Lq, M * D)).astype(np.float32)
    return dict(shapes=shapes, value=value, loc=np.ascontiguousarray(loc, np.float32), attn=attn, gout=gout, pixels=pixels)


def case_a():
    """off-map samples, edge corners, empty rows; two images, two heads.  Locations are uniform on [-0.1, 1.1]^2, except that head 1
    of image 1 keeps x below 0.45: the right half of every level gets no sample there (rows without entries)"""
    rng = np.random.default_rng(100)
    loc = rng.uniform(-0.1, 1.1, (2, 120, 2, 4, 4, 2))
    loc[1, :, 1, :, :, 0] = rng.uniform(-0.1, 0.45, (120, 4, 4))
    return _case(PYR, 2, 2, 120, 4, seed=101, loc=loc)


def _pixel_case(levels, seed):
    rng = np.random.default_rng(seed)
    L, P, N, M = len(levels), 4, 2, 2
    c = _pixel_centres(levels)                                            # (S, 2)
    sigma = 1.5 / np.asarray(levels, np.float64)[:, ::-1]                   # 1.5 px of each level, (L, 2) as (x, y)
    loc = c[None, :, None, None, None, :] + rng.standard_normal((N, len(c), M, L, P, 2)) * sigma[None, None, None, :, None, :]
    return _case(levels, N, M, len(c), P, seed + 1, loc=loc, pixels=True)


def case_b():
    """the queries are the pixels of PYR in order (Lq = S = 65, L * P = 16: the patch gather's instantiation with the flag)"""
    return _pixel_case(PYR, 102)


def case_c5():
    """five levels, P 4 (L * P = 20), queries = pixels"""
    return _pixel_case(PYR5, 103)


def case_c1():
    """one level, one point"""
    return _case([(5, 7)], 2, 3, 40, 1, seed=104)


def case_d():
    """one 1 x 1 level, P 8, Lq 1024: every sample has exactly one valid corner, the level's only pixel -- 8192 entries in one row"""
    rng = np.random.default_rng(105)
    loc = rng.uniform(0.01, 0.99, (1, 1024, 1, 1, 8, 2))
    return _case([(1, 1)], 1, 1, 1024, 8, seed=106, loc=loc)


def case_e():
    """a 4 x 4 level, every sample on a pixel centre ((j + 0.5) / 4, exact in fp32), attention weights 1, grad_out drawn from
    {+-2^100, +-2^-100, +-1.5}: a sample's contribution to its pixel is grad_out exactly (w = 1 * (1 * 1)) and exactly zero to the
    other corners, so grad_value is the exact sum of the grad_out rows that sample the pixel"""
    rng = np.random.default_rng(107)
    N, M, Lq, P = 1, 2, 96, 2
    pix = rng.integers(0, 4, (N, Lq, M, 1, P, 2))
    loc = ((pix + 0.5) / 4.0).astype(np.float32)
    case = _case([(4, 4)], N, M, Lq, P, seed=108, loc=loc)
    case["attn"] = np.ones((N, Lq, M, 1, P), np.float32)
    vals = np.array([2.0 ** 100, -2.0 ** 100, 2.0 ** -100, -2.0 ** -100, 1.5, -1.5], np.float32)
    case["gout"] = vals[rng.integers(0, 6, (N, Lq, M * D))]
    case["pix"] = pix
    return case


def case_f():
    """case (a) with NaN, +inf and -inf planted in grad_out: queries 3 / 4 / 5 of image 0, head 0.  All three reach the 1 x 1
    level's pixel (a shared destination row: NaN wins there, and without the NaN the two infinities would meet); on the finest level
    their rows mostly differ."""
    case = case_a()
    g = case["gout"].copy()
    g[0, 3, 0:8] = np.nan
    g[0, 4, 0:16] = np.inf
    g[0, 5, 8:24] = -np.inf
    case["gout"] = g
    return case

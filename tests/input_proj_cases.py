"""Cases of the input-projection tests (tests/test_input_proj_ref.py on the CPU, tests/test_gpu_input_proj.py on the GPU): the
smallest at which csrc/group_norm_tokens.hip can go wrong.  Test helper, numpy only; the float64 statement of a case is computed
once (``reference``) and shared.

shapes: ``pyr4_odd`` -- four levels of odd sizes down to 1 x 1 (every plane start only element-aligned, tiles smaller than 64
pixels, one pixel); ``one_9x33`` -- 297 pixels: five tiles with a ragged tail of 41, three backward units, hw odd;
``aligned_vec`` -- 16 x 16 and 8 x 8: hw % 4 == 0, the 16-byte path, four tiles and one; ``ragged_chunks`` -- one level whose
groups span three statistics chunks (the last ragged) and whose pixels span 34 tiles with a tail of 3, from the kernel's
constants; ``levels8`` -- the most levels the table holds.
special groups (fp32 cases with a 5 x 7 or 16 x 16 level 0): group 0 of image 0, level 0 holds equal values (var = 0: the
tokens are the bias bit for bit); group 1 sits at mean 4096 with spread 1e-2 (cancellation).
``pos``: ``contiguous`` (N, S, 256) or ``strided`` -- the slice ``buf[:, 1:-1, :256]`` of an (N, S + 2, 512) buffer: both leading
strides differ from the contiguous ones whatever N is, and the N = 2 pyramid and its 16-bit variants (8-byte rows) have it; the upstream
gradients ``gy`` only, ``gq`` only, or both.  Every level has its own random weight (with zeros and negatives) and bias.
The 16-bit variants hold 16-bit numbers in fp32 arrays: ``x`` of that type, and -- ``out16`` -- tokens, q, gy, gq, pos and dx
of that type too, or -- ``out32``, what autocast gives -- everything else fp32.
"""
import functools

import numpy as np

import input_proj_ref64 as R

F = np.float32
D = 256
RAGGED_HW = 2 * R.CHUNK // R.CG + R.TILE + 3        # 2115 pixels: 8 * hw = 2 chunks + 536 elements; 33 tiles + 3 pixels

#        name             N  shapes                                                          pos           grads   eps    x16    out16
TABLE = [("pyr4_odd",      2, [(5, 7), (3, 4), (2, 2), (1, 1)],                                "strided",    "both", 1e-5, None,   False),
         ("one_9x33",      1, [(9, 33)],                                                       "strided",    "gq",   1e-5, None,   False),
         ("aligned_vec",   2, [(16, 16), (8, 8)],                                              "contiguous", "both", 1e-5, None,   False),
         ("ragged_chunks", 2, [(1, RAGGED_HW)],                                                None,         "gy",   1e-5, None,   False),
         ("levels8",       1, [(3, 5), (2, 4), (4, 4), (1, 3), (2, 2), (1, 2), (1, 1), (3, 3)], "strided",    "both", 1e-6, None,   False)]
for _dt in ("fp16", "bf16"):
    for _o16 in (False, True):
        _tag = f"{_dt}_{'out16' if _o16 else 'out32'}"
        TABLE += [(f"pyr4_odd_{_tag}", 2, [(5, 7), (3, 4), (2, 2), (1, 1)], "strided", "both", 1e-5, _dt, _o16),
                  (f"one_9x33_{_tag}", 1, [(9, 33)], "strided", "gq", 1e-5, _dt, _o16)]


def names():
    return [t[0] for t in TABLE]


def round16(a, dtype):
    """fp32 array -> the nearest (ties to even) numbers of the 16-bit type, held in fp32; ``None``: unchanged"""
    a = np.ascontiguousarray(a, F)
    if dtype is None:
        return a
    if dtype == "fp16":
        return a.astype(np.float16).astype(F)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
    return bits.astype(np.uint32).view(F)


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    for i, (name, n, shapes, pos, grads, eps, x16, out16) in enumerate(TABLE):
        rng = np.random.default_rng(300 + i)
        o16 = x16 if out16 else None
        xs = [(rng.standard_normal((n, D) + s) * (0.5 + 0.5 * l) + 0.25 * l).astype(F) for l, s in enumerate(shapes)]
        if x16 is None and shapes[0] in ((5, 7), (16, 16)):
            xs[0][0, 0:8] = F(1.375)
            xs[0][0, 8:16] = (4096.0 + 1e-2 * rng.standard_normal((8,) + shapes[0])).astype(F)
        xs = [round16(x, x16) for x in xs]
        weights, biases = [], []
        for _ in shapes:
            w = (rng.standard_normal(D) * 0.5 + 1.0).astype(F)
            w[::17] = 0.0
            w[5::29] = -np.abs(w[5::29]) - F(0.25)
            b = (rng.standard_normal(D) * 0.3 + 0.1).astype(F)
            b[b == 0] = F(0.5)
            weights.append(w)
            biases.append(b)
        rows = sum(h * w for h, w in shapes)
        full = (n, rows, D)
        case = dict(name=name, shapes=shapes, xs=xs, weights=weights, biases=biases, eps=eps, pos_layout=pos, x16=x16, out16=o16,
                    pos=round16(rng.standard_normal(full), o16) if pos else None,
                    gy=round16(rng.standard_normal(full), o16) if grads in ("gy", "both") else None,
                    gq=round16(rng.standard_normal(full), o16) if grads in ("gq", "both") else None)
        assert case["gq"] is None or pos
        for v in list(case.values()) + xs + weights + biases:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[name] = case
    return out


def cases():
    return _cases()


def out_dtypes(case):
    """{output: 'fp16' | 'bf16'} of the outputs a case rounds into a 16-bit type (``check_gn_tokens``' ``dtypes``)"""
    d = {}
    if case["out16"]:
        d.update(tokens=case["out16"], q=case["out16"])
    if case["x16"]:
        d.update({f"dx{l}": case["x16"] for l in range(len(case["shapes"]))})
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 statement of a case, computed once; callers leave it unchanged"""
    return R.ref64(_cases()[name])

"""Cases of the add + LayerNorm tests (tests/test_add_norm_ref.py on the CPU, tests/test_gpu_add_norm.py on the GPU): the
smallest at which csrc/add_norm.hip can go wrong.  Test helper, numpy only; the float64 statement of a case is computed once
(``reference``) and shared.

rows: 1 (a single wave-row), 3 (fewer rows than waves in a workgroup), 65 (a ragged tail: 4 forward workgroups and a 17th row
in the fifth, one full backward slot and one with a single row), 2 051 (several workgroups, the last parameter slot ragged:
2 051 = 32 * 64 + 3).
layouts: ``contiguous`` (B, S, 256); ``transposed`` -- the (L, B, 256) view of a (B, L, 256) buffer; ``offset`` -- a slice
``buf[:, 1:-1]`` of a (B, S + 2, 256) buffer with a storage offset of 256 elements.
Rows of every case with at least 3 rows: row 0 holds equal values (var = 0: y == bias exactly), row 1 sits at mean 4096 with
spread 1e-2 (cancellation); ``weight`` has zeros and negatives.
"""
import functools

import numpy as np

import add_norm_ref64 as R

F = np.float32
D = 256

#        name                    shape        layout        residual pos    grads   eps
TABLE = [("r1_plain",            (1, 1),      "contiguous", True,    True,  "both", 1e-5),
         ("r1_bare",             (1, 1),      "contiguous", False,   False, "gy",   1e-5),
         ("r3_special_rows",     (1, 3),      "contiguous", True,    True,  "both", 1e-5),
         ("r3_tiny_eps",         (3, 1),      "transposed", False,   True,  "gq",   1e-12),
         ("r65_transposed",      (13, 5),     "transposed", True,    True,  "gq",   1e-5),
         ("r65_offset",          (5, 13),     "offset",     False,   False, "gy",   1e-12),
         ("r65_contiguous",      (1, 65),     "contiguous", True,    False, "gy",   1e-5),
         ("r2051_contiguous",    (7, 293),    "contiguous", True,    True,  "both", 1e-5),
         ("r2051_transposed",    (293, 7),    "transposed", True,    False, "gy",   1e-5),
         ("r2051_offset_nores",  (7, 293),    "offset",     False,   True,  "gy",   1e-5)]


def names():
    return [t[0] for t in TABLE]


@functools.lru_cache(maxsize=None)
def _cases():
    out = {}
    for i, (name, shape, layout, has_res, has_pos, grads, eps) in enumerate(TABLE):
        rng = np.random.default_rng(100 + i)
        full = shape + (D,)
        x = rng.standard_normal(full).astype(F)
        res = (rng.standard_normal(full) * 0.5 + 0.25).astype(F) if has_res else None
        rows = shape[0] * shape[1]
        if rows >= 3:
            xf = x.reshape(rows, D)
            xf[0] = F(1.375)
            xf[1] = (4096.0 + 1e-2 * rng.standard_normal(D)).astype(F)
            if res is not None:
                rf = res.reshape(rows, D)
                rf[0] = F(-0.625)
                rf[1] = F(0.0)
        w = (rng.standard_normal(D) * 0.5 + 1.0).astype(F)
        w[::17] = 0.0
        w[5::29] = -np.abs(w[5::29]) - F(0.25)
        b = (rng.standard_normal(D) * 0.3 + 0.1).astype(F)
        b[b == 0] = F(0.5)
        case = dict(name=name, shape=shape, layout=layout, x=x, residual=res,
                    pos=rng.standard_normal(full).astype(F) if has_pos else None, weight=w, bias=b, eps=eps,
                    gy=rng.standard_normal(full).astype(F) if grads in ("gy", "both") else None,
                    gq=rng.standard_normal(full).astype(F) if grads in ("gq", "both") else None)
        assert case["gq"] is None or has_pos
        for v in case.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[name] = case
    return out


def cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 statement of a case, computed once; callers leave it unchanged"""
    return R.ref64(_cases()[name])

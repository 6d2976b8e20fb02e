"""Small problems at which the self-attention kernels can still go wrong (tests/test_self_attn_ref.py on the CPU,
tests/test_gpu_self_attn.py on the GPU).  A problem is what ``self_attn_ref64.ref64`` takes: ``q (Lq, B, E)``, ``k, v (Lk, B, E)``
float32, ``heads``, ``mask`` (bool, True = blocked) or None, ``scale`` (None = D ** -0.5), ``gout`` from ``grad_pattern``;
``layout`` says how the GPU test hands the operands over (``separate`` contiguous tensors or ``packed`` slices of one
``(L, B, 3E)`` buffer) and ``forward_only`` marks the case whose backward is outside the contract.

The kernels work on 32 x 32 tiles, two query (or key) tiles per workgroup: the sizes straddle 32, 64 and 128, and 257 takes
more than one workgroup per head with a ragged last tile."""
import functools

import numpy as np

from self_attn_ref64 import grad_pattern, ref64

D = 32
SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 129, 257)


def dn_mask(single_pad, groups, matching):
    """The attention mask of prepare_for_cdn (detr_od/models/dense_heads/dn_components.py:101-112): ``groups`` de-noising groups
    of ``2 * single_pad`` queries, then ``matching`` queries.  True = blocked."""
    pad = single_pad * 2 * groups
    size = pad + matching
    m = np.zeros((size, size), bool)
    m[pad:, :pad] = True
    for i in range(groups):
        lo, hi = single_pad * 2 * i, single_pad * 2 * (i + 1)
        m[lo:hi, hi:pad] = True
        m[lo:hi, :lo] = True
    return m


def random_mask(rng, Lq, Lk, density):
    """Blocked with probability ``density``; every row keeps one open key."""
    m = rng.random((Lq, Lk)) < density
    m[np.arange(Lq), rng.integers(0, Lk, Lq)] = False
    return m


def _problem(seed, Lq, Lk, B, H, mask=None, scale=None, amp=1.0, layout="separate", forward_only=False):
    rng = np.random.default_rng(seed)
    E = H * D
    p = dict(q=(rng.standard_normal((Lq, B, E)) * amp).astype(np.float32), k=(rng.standard_normal((Lk, B, E)) * amp).astype(np.float32),
             v=rng.standard_normal((Lk, B, E)).astype(np.float32), heads=H, mask=mask, scale=scale,
             gout=grad_pattern((Lq, B, E), seed), layout=layout, forward_only=forward_only)
    return p


@functools.lru_cache(maxsize=None)
def cases():
    """name -> problem (built once; nothing in a problem is to be modified)"""
    out = {}
    for i, L in enumerate(SIZES):
        rng = np.random.default_rng(100 + L)
        out[f"L{L}_B1"] = _problem(L, L, L, 1, 8, layout="packed" if i % 2 else "separate")
        out[f"L{L}_B3_masked"] = _problem(1000 + L, L, L, 3, 8, mask=random_mask(rng, L, L, 0.5) if L > 1 else None,
                                          layout="separate" if i % 2 else "packed")
    out["one_head"] = _problem(1, 70, 70, 2, 1, mask=dn_mask(3, 4, 46))
    out["lq_ne_lk"] = _problem(2, 45, 100, 2, 8, mask=random_mask(np.random.default_rng(2), 45, 100, 0.5))
    out["lq_ne_lk_wide"] = _problem(3, 130, 37, 1, 8)
    out["dn_edges_in_tiles"] = _problem(4, 70, 70, 2, 8, mask=dn_mask(3, 4, 46), layout="packed")
    out["dn_skipped_tiles"] = _problem(5, 390, 390, 1, 8, mask=dn_mask(40, 4, 70))
    out["random_050"] = _problem(6, 97, 97, 2, 8, mask=random_mask(np.random.default_rng(6), 97, 97, 0.5))
    out["random_095"] = _problem(7, 150, 150, 1, 8, mask=random_mask(np.random.default_rng(7), 150, 150, 0.95))
    one = np.ones((80, 80), bool)
    one[np.arange(80), np.random.default_rng(8).integers(0, 80, 80)] = False
    out["one_open_key"] = _problem(8, 80, 80, 2, 8, mask=one)
    # the score scale * q.k has the standard deviation amp^2 = 40, so its extremes reach about +-200: exp() overflows in fp32
    # without the subtraction of the maximum
    out["large_scores"] = _problem(9, 96, 96, 1, 8, amp=6.3, mask=random_mask(np.random.default_rng(9), 96, 96, 0.3))
    out["scale_given"] = _problem(10, 65, 65, 1, 8, scale=0.3, layout="packed")
    dead = random_mask(np.random.default_rng(11), 66, 66, 0.5)
    dead[40, :] = True
    out["blocked_row"] = _problem(11, 66, 66, 2, 8, mask=dead, forward_only=True)
    return out


def names():
    return list(cases())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 statement of a case with its bounds, computed once and shared."""
    p = cases()[name]
    return ref64(p, grads=not p["forward_only"])


def full_size():
    """The decoder's own size: 900 matching queries + a pad of 200 (100 groups of 2), B = 2."""
    return _problem(12, 1100, 1100, 2, 8, mask=dn_mask(1, 100, 900))

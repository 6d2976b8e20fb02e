"""A plain float64 statement of DINO's two-stage query selection (detr_od/models/utils/transformer.py:525-575, 1315-1346,
1398) with per-element bounds on what an fp32 implementation may differ by.  numpy only.

Decisions.  The valid flag compares the quotient (x + 0.5) / valid_W with 0.01 and 0.99 in fp32.  Both operands of the
quotient are exact in fp32 (half-integers and counts below 2^24), so "the fp32 run" means one thing: the IEEE correctly
rounded fp32 quotient against float32(0.01) / float32(0.99).  A float64 quotient of two fp32 numbers rounded to fp32 IS that
quotient (53 >= 2 * 24 + 2 bits: no double rounding), so the statement decides on ``float32(float64 quotient)`` and the
flags of any correctly rounding fp32 implementation equal it bit for bit.  The boundary is hit by DINO's own shapes: level
(50, 84) gives 0.5 / 50 against 0.01, which is not ``>`` in either precision.

Values, with u = 2^-24 (one rounding).  p32 = p (1 + d), |d| <= u (for the w/h anchors: float32(0.05) against 0.05).
logit(p) = log(p) - log(1 - p) has slope 1 / (p (1 - p)), so the input error moves it by u / (1 - p) (< 101 u on (0.01,
0.99)); 1 - p32 rounds once (u), the division once (u), and ``logf`` is within one ulp = 2 u |result|:
    bound_logit = u (1 / (1 - p) + 2) + 2 u |logit|,  times 1.01 for the second-order terms.
sigmoid(x) = 1 / (1 + exp(-x)) from an exact fp32 x: exp one ulp (2 u), the sum u, the quotient u, all relative and damped
by e / (1 + e) <= 1 or 1:  bound_sigmoid = 4 u s + 2^-126.  An input error E adds s (1 - s) E + E^2 (|s''| < 1).
Copies (rows of tensors, masked rows, gradients routed through the inverse map) are exact.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
F32 = np.float32

MUTANTS = ("ge", "no_half", "swap_wh", "extents", "linear_scale", "fill_zero", "ascending", "ties_high", "max_axis",
           "no_sigmoid")


def grad_pattern(shape, salt):
    """A deterministic gradient of fp32-representable values in [-1, 1]."""
    n = int(np.prod(shape))
    return (((np.arange(n, dtype=np.int64) * (2 * salt + 7) + salt) % 17 - 8) / 8.0).astype(F32).reshape(shape)


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def proposals(mask, shapes, mutant=None):
    """mask (N, S) bool, shapes [(H, W)] -> dict(valid (N, S) bool, prop (N, S, 4) float64 (+inf where invalid), bound)."""
    mask = np.asarray(mask, bool)
    N, S = mask.shape
    prop = np.zeros((N, S, 4))
    valid = np.zeros((N, S), bool)
    at = 0
    lo, hi = F32(0.01), F32(0.99)
    for l, (H, W) in enumerate(shapes):
        H, W = int(H), int(W)
        m = mask[:, at:at + H * W].reshape(N, H, W)
        if mutant == "extents":          # the last unmasked row / column + 1, what a mask summary would return
            vH = np.asarray([(np.nonzero(~m[n].all(1))[0].max(initial=-1) + 1) for n in range(N)], np.float64)
            vW = np.asarray([(np.nonzero(~m[n].all(0))[0].max(initial=-1) + 1) for n in range(N)], np.float64)
        else:
            vH, vW = (~m[:, :, 0]).sum(1).astype(np.float64), (~m[:, 0, :]).sum(1).astype(np.float64)
        if mutant == "swap_wh":
            vH, vW = vW, vH
        half = 0.0 if mutant == "no_half" else 0.5
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        with np.errstate(divide="ignore", invalid="ignore"):
            px = (x[None] + half) / vW[:, None, None]
            py = (y[None] + half) / vH[:, None, None]
        wh = 0.05 * l if mutant == "linear_scale" else 0.05 * 2.0 ** l
        p = np.stack([px, py, np.full_like(px, wh), np.full_like(px, wh)], -1).reshape(N, H * W, 4)
        p32 = p.astype(F32)              # the fp32 run's operands of the comparison (module docstring)
        p32[..., 2:] = F32(0.05) * F32(2.0 ** l) if mutant != "linear_scale" else F32(0.05) * F32(l)
        ok = ((p32 >= lo) & (p32 <= hi)) if mutant == "ge" else ((p32 > lo) & (p32 < hi))
        valid[:, at:at + H * W] = ok.all(-1) & ~mask[:, at:at + H * W]
        prop[:, at:at + H * W] = p
        at += H * W
    assert at == S, (at, S)
    v = valid[..., None] & np.ones(4, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        logit = np.log(prop / (1.0 - prop))
        bound = 1.01 * (U * (1.0 / (1.0 - prop) + 2.0) + 2.0 * U * np.abs(logit))
    fill = 0.0 if mutant == "fill_zero" else np.inf
    return dict(valid=valid, prop=np.where(v, logit, fill), bound=np.where(v, bound, 0.0))


def masked_memory(memory, valid):
    return np.where(valid[..., None], memory, 0).astype(memory.dtype)


def keys_of(logits, mutant=None):
    """(N, S, C) -> (N, S) float64 keys, NaN propagating.  Mutant: the buffer read as (N, C, S), max over the wrong axis."""
    lg = np.asarray(logits, np.float64)
    if mutant == "max_axis":
        return lg.reshape(lg.shape[0], lg.shape[2], lg.shape[1]).max(1)
    return lg.max(-1)


def topk(keys, k, mutant=None):
    """keys (N, S) -> indices (N, k) sorted by (key descending, token ascending); NaN above +inf; -0 == +0."""
    keys = np.asarray(keys, np.float64)
    N, S = keys.shape
    out = np.zeros((N, k), np.int64)
    idx = np.arange(S)
    for n in range(N):
        nan = np.isnan(keys[n])
        kv = np.where(nan, 0.0, keys[n]) + 0.0
        tie = -idx if mutant == "ties_high" else idx
        order = np.lexsort((tie, kv, nan)) if mutant == "ascending" else np.lexsort((tie, -kv, ~nan))
        out[n] = order[:k]
    return out


def inverse_map(indices, S):
    N, k = indices.shape
    inv = np.full((N, S), -1, np.int32)
    for n in range(N):
        inv[n, indices[n]] = np.arange(k, dtype=np.int32)
    return inv


def gather(indices, coord, prop, prop_bound, memory, mutant=None):
    """-> dict(refpoint, tgt (exact copies), init_box, init_bound, ref_enc, ref_bound) in float64."""
    n = np.arange(indices.shape[0])[:, None]
    ref = np.asarray(coord, np.float64)[n, indices]
    pr, E = np.asarray(prop, np.float64)[n, indices], np.asarray(prop_bound, np.float64)[n, indices]
    s = pr if mutant == "no_sigmoid" else sigmoid(pr)
    r = sigmoid(ref)
    return dict(refpoint=ref, tgt=np.asarray(memory)[n, indices], init_box=s,
                init_bound=s * (1 - s) * E + E * E + 4 * U * s + TINY, ref_enc=r, ref_bound=4 * U * r + TINY)


def gather_backward(indices, S, ref_enc, g_ref, g_tgt, g_enc):
    """float64 gradients w.r.t. coord (N, S, 4) (+ its fp32 bound) and output_memory (N, S, D) (copies); any g may be None."""
    N, k = indices.shape
    n = np.arange(N)[:, None]
    r = np.asarray(ref_enc, np.float64)
    t = r * (1 - r)
    gc, bound = np.zeros((N, S, 4)), np.zeros((N, S, 4))
    a = np.zeros((N, k, 4)) if g_ref is None else np.asarray(g_ref, np.float64)
    b = np.zeros((N, k, 4)) if g_enc is None else np.asarray(g_enc, np.float64)
    rows = a + b * t
    # r carries 4 u r; 1 - r, r (1 - r), the product with g and the sum round once each
    gc[n, indices] = rows
    bound[n, indices] = 1.01 * (np.abs(b) * (4 * U * r + 3 * U * t) + U * (np.abs(a) + np.abs(b) * t)) + TINY
    gm = None
    if g_tgt is not None:
        gm = np.zeros((N, S, g_tgt.shape[2]), g_tgt.dtype)
        gm[n, indices] = g_tgt
    return gc, bound, gm


def widen16(bound, value, dtype):
    """``bound`` of a result with the float64 value ``value`` that leaves in a 16-bit type (``'fp16'`` / ``'bf16'``), widened by
    that one rounding: B + u16 (|ref| + B) + s16 (tests/msda_h16_ref.py).  ``None``: unchanged."""
    if dtype is None:
        return bound
    from msda_h16_ref import widen16 as widen
    return widen(np.asarray(bound, np.float64), np.asarray(value, np.float64), dtype)


def unique_key_slots(keys, indices):
    """(N, k) bool: the slot's key occurs once in its image (its token is then decided by the keys alone)."""
    out = np.zeros(indices.shape, bool)
    for n in range(indices.shape[0]):
        kv = np.asarray(keys[n], np.float64) + 0.0
        for r, i in enumerate(indices[n]):
            out[n, r] = (np.isnan(kv).sum() if np.isnan(kv[i]) else (kv == kv[i]).sum()) == 1
    return out

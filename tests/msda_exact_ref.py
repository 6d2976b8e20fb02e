"""Model of the exact MSDA backward (semidetr_msda_backward_exact_f32): grad_value as the exact sum of its fp32 contributions,
rounded once.  Test helper (not a conftest), numpy + Python integers only.

Contribution (the definition of csrc/msda_exact.h, restated in numpy float32 whose every operation rounds once): a sample at
normalised (lx, ly) of level l has x = fl(fl(lx * W) - 0.5), y = fl(fl(ly * H) - 0.5) and is skipped unless -1 < x < W and
-1 < y < H; x0 = floor(x), fx = fl(x - x0), gx = fl(1 - fx) (likewise y); its corners (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
(y0 + 1, x0 + 1) have c = fl(gy * gx), fl(gy * fx), fl(fy * gx), fl(fy * fx) and count only inside the map.  For a valid corner k:
w = fl(a * c_k) and contribution[d] = fl(w * grad_out[n, q, m, d]), added to grad_value[n, row_k, m, d].

Sum.  A finite fp32 number is an integer multiple of 2^-149, so the exact sum is Fraction(T, 2^149) with T the sum of the
contributions' integer multiples: the model adds Python integers (exact, unbounded) and rounds T / 2^149 once to nearest even
(`round_fraction_bits`, written from the Fraction, not from the accumulator's word layout).  `exact_sum_bits` does the same on a
plain list through `fractions.Fraction` itself: it is what the accumulator (csrc/msda_exactsum.h) is compared with bit for bit.
Non-finite contributions follow IEEE addition's answer in every order: NaN if a NaN or both infinities occur, else the infinity.

Bound against tests/msda_ref64.py (its error model: |got - ref| <= 2u * n * A + 2 * C + tiny, one ulp = 2u allowed per
operation, n = the roundings on a term's path).  Here a term's path has the roundings INSIDE the term -- 1 - fy, 1 - fx, their
product, times a, times grad_out: 5, within the model's DEPTH = 8 -- and the sum adds exactly ONE more rounding in total (the
final round to nearest) instead of the (number of contributions - 1) a floating-point sum pays.  So n = DEPTH + 1 for every
element, whatever the number of contributions; A and C (the sensitivity to the pixel coordinates' own rounding, which the exact
sum shares with every other kernel) are msda_ref64's, unscaled.  `bounded_exact(gv)` re-labels msda_ref64's grad_value so.
"""
from fractions import Fraction

import numpy as np

from msda_ref64 import DEPTH, Bounded

_SCALE = 2.0 ** 149


def round_fraction_bits(fr):
    """fp32 bit pattern of a Fraction rounded to nearest even; overflow -> +-inf, subnormals as fp32 has them, 0 -> +0."""
    fr = Fraction(fr)
    sign = 0x80000000 if fr < 0 else 0
    t = abs(fr) * (1 << 149)                 # in units of the smallest subnormal
    if t < (1 << 24):                        # subnormals and the first normal binade: spacing 1 unit
        q, rem = divmod(t.numerator, t.denominator)
        if 2 * rem > t.denominator or (2 * rem == t.denominator and q & 1):
            q += 1
        return sign | q                      # (q == 2^24 lands on the next binade's first pattern by itself)
    mag_floor = t.numerator // t.denominator
    shift = mag_floor.bit_length() - 24      # spacing of the binade, in units: 2^shift
    unit = Fraction(1 << shift)
    q = int(t / unit)                        # 24-bit mantissa, floor
    rem = t - q * unit
    if 2 * rem > unit or (2 * rem == unit and q & 1):
        q += 1
    if q == 1 << 24:
        q >>= 1
        shift += 1
    e = shift + 1
    if e >= 255:
        return sign | 0x7f800000
    return sign | (e << 23) | (q & 0x7fffff)


def bits_of(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def exact_sum_bits(values):
    """The contract on a list of fp32 numbers -> bit pattern (int)."""
    v = np.asarray(values, np.float32).reshape(-1)
    if np.isnan(v).any() or (np.isposinf(v).any() and np.isneginf(v).any()):
        return 0x7fc00000
    if np.isposinf(v).any():
        return 0x7f800000
    if np.isneginf(v).any():
        return 0xff800000
    return round_fraction_bits(sum((Fraction(float(x)) for x in v), Fraction(0)))


def sequential_sum_bits(values):
    """fp32 addition in the order given (what an atomic or a loop does)."""
    acc = np.float32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for x in np.asarray(values, np.float32).reshape(-1):
            acc = np.float32(acc + x)
    return int(bits_of(acc)[0])


def contributions(shapes, loc, attn, gout):
    """-> dest (K,) int64 = (n * S + row) * M + m, contrib (K, D) float32, in the order (n, q, m, l, p, corner)."""
    shapes = np.asarray(shapes, np.int64)
    loc = np.asarray(loc, np.float32)
    attn = np.asarray(attn, np.float32)
    N, Lq, M, L, P, _ = loc.shape
    start = np.concatenate([[0], np.cumsum(shapes[:, 0] * shapes[:, 1])[:-1]]).astype(np.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    g = np.asarray(gout, np.float32).reshape(N, Lq, M, -1)
    Hf = shapes[:, 0].astype(np.float32).reshape(L, 1)
    Wf = shapes[:, 1].astype(np.float32).reshape(L, 1)
    one, half = np.float32(1), np.float32(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (loc[..., 0] * Wf).astype(np.float32) - half
        y = (loc[..., 1] * Hf).astype(np.float32) - half
        inside = (y > -1) & (x > -1) & (y < Hf) & (x < Wf)
        xs, ys = np.where(inside, x, np.float32(0)), np.where(inside, y, np.float32(0))
        x0, y0 = np.floor(xs), np.floor(ys)
        fx, fy = (xs - x0).astype(np.float32), (ys - y0).astype(np.float32)
        gx, gy = (one - fx).astype(np.float32), (one - fy).astype(np.float32)
        c = np.stack([gy * gx, gy * fx, fy * gx, fy * fx], -1).astype(np.float32)
        w = (attn[..., None] * c).astype(np.float32)                                   # (N, Lq, M, L, P, 4)
        cy = y0[..., None].astype(np.int64) + np.array([0, 0, 1, 1])
        cx = x0[..., None].astype(np.int64) + np.array([0, 1, 0, 1])
        Hi, Wi = shapes[:, 0].reshape(L, 1, 1), shapes[:, 1].reshape(L, 1, 1)
        ok = inside[..., None] & (cy >= 0) & (cx >= 0) & (cy <= Hi - 1) & (cx <= Wi - 1)
        row = start.reshape(L, 1, 1) + cy * Wi + cx
        n_i = np.arange(N).reshape(N, 1, 1, 1, 1, 1)
        m_i = np.arange(M).reshape(1, 1, M, 1, 1, 1)
        dest = np.broadcast_to((n_i * S + row) * M + m_i, ok.shape)[ok]
        gq = np.broadcast_to(g[:, :, :, None, None, None, :], ok.shape + (g.shape[-1],))[ok]
        contrib = (w[ok][:, None] * gq).astype(np.float32)
    return dest.astype(np.int64), contrib


def exact_grad_value(N, S, M, dest, contrib):
    """grad_value (N, S, M, D) float32: per element the exact sum of its contributions, rounded once; counts (N, S, M)."""
    D = contrib.shape[1]
    rows = N * S * M
    c64 = contrib.astype(np.float64)
    fin = np.isfinite(c64)
    nan = np.zeros((rows, D), np.int64)
    pinf = np.zeros((rows, D), np.int64)
    ninf = np.zeros((rows, D), np.int64)
    np.add.at(nan, dest, np.isnan(c64))
    np.add.at(pinf, dest, np.isposinf(c64))
    np.add.at(ninf, dest, np.isneginf(c64))
    counts = np.bincount(dest, minlength=rows)
    # integer multiples of 2^-149 (exact in float64: a product of an fp32 number and a power of two), as Python integers
    units = np.where(fin, c64, 0.0) * _SCALE
    order = np.argsort(dest, kind="stable")
    out_bits = np.zeros((rows, D), np.uint32)
    if len(order):
        ints = np.array([[int(v) for v in r] for r in units[order]], dtype=object).reshape(len(order), D)
        sd = dest[order]
        first = np.flatnonzero(np.concatenate([[True], sd[1:] != sd[:-1]]))
        sums = np.add.reduceat(ints, first, axis=0)
        for r, tot in zip(sd[first], sums):
            out_bits[r] = [round_fraction_bits(Fraction(int(t), 1 << 149)) for t in tot]
    out_bits = np.where(pinf > 0, np.uint32(0x7f800000), out_bits)
    out_bits = np.where(ninf > 0, np.uint32(0xff800000), out_bits)
    out_bits = np.where((nan > 0) | ((pinf > 0) & (ninf > 0)), np.uint32(0x7fc00000), out_bits)
    return out_bits.view(np.float32).reshape(N, S, M, D), counts.reshape(N, S, M)


def sequential_grad_value(N, S, M, dest, contrib):
    """The same contributions added in fp32 in the order listed (what row atomics do in SOME order)."""
    out = np.zeros((N * S * M, contrib.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r, c in zip(dest, contrib):
            out[r] += c
    return out.reshape(N, S, M, -1)


def model(shapes, loc, attn, gout):
    """grad_value of the exact route for a whole call -> (N, S, M, D) float32."""
    shapes = np.asarray(shapes, np.int64)
    N, _, M = np.asarray(loc).shape[:3]
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    dest, contrib = contributions(shapes, loc, attn, gout)
    return exact_grad_value(N, S, M, dest, contrib)[0]


def bounded_exact(gv):
    """msda_ref64's grad_value with the exact sum's rounding count (module docstring): n = DEPTH + 1."""
    return Bounded(gv.val, gv.A, DEPTH + 1, gv.C, gv.skip)

"""Plain float64 statement of csrc/group_norm_tokens.hip -- GroupNorm(32, 256) of every pyramid level written as token rows, the
positional add, and the backward -- each quantity carried as a (value, err) pair through the expression tree (the helpers are
those of add_norm_ref64.py), and the checker ``check_gn_tokens`` that decides whether a result (from the GPU, from torch's fp32
CPU ops, or from the numpy evaluation ``eval_f32`` below) is ADMISSIBLE against it.

Test helper (not a conftest; imported by name like add_norm_ref64.py).  Numpy only.

Conventions: those of add_norm_ref64.py (u = 2^-24, inputs exact, one rounding per fp32 operation, contraction off in the kernels
so there is no fused operation to allow for), and
  * a sum over a group (8 channels x H W elements) is bounded by  depth * u * sum |terms|  plus the terms' own errors.  The
    kernel adds a group in chunks of ``CHUNK`` = 8192 consecutive elements, one workgroup each, and merges the chunks in
    float64.  Within a chunk a term passes through at most
        log2(4)                     the four elements of a lane's float4                                   2
      + CHUNK / (256 threads * 4)   the chain over the thread's eight float4 (the first lands on nothing:   8
                                    7 for the sum, 8 for the squares, which start from 0)
      + log2(64)                    the xor butterfly over the wave                                        6
      + 4 - 1                       the four waves in wave order                                           3
    additions, hence ``GROUP_DEPTH`` = 19; the float64 merge adds  chunks * 2^-53  and the one rounding to fp32 of the result.
    It is derived from the kernel's constants, not tuned.
  * the variance follows the kernel's tree: per chunk c the mean m_c = fp32(s_c / n_c) and M2_c = sum (x - m_c)^2, then
    M2 = sum_c (M2_c + n_c (m_c - mean)^2) in float64 with m_c - mean rounded to fp32, var = fp32(M2 / n).  The error of m_c
    enters M2_c in second order only (``_sq_dev_sum``), which is what keeps a statement on the cancellation group.  A group of one
    chunk has m_c == mean bit for bit (the same correctly rounded quotient), so its second term is exactly zero.  The plain
    E[x^2] - mean^2 is far outside on the group at mean 4096 with spread 1e-2 (its error is u 4096^2 = 1 against a variance of 1e-4).
  * the affine step is stated as the kernel has it, y = ((x - mean) * rstd) * w + b, and the bound also admits the other
    factorisation stock implementations use, y = x * (rstd * w) + (b - mean * rstd * w): its two products and its sum round
    numbers of the size |x rstd w|, |mean rstd w| and |b|, so  2 u (|x| + |mean|) |rstd w| + u |b|  is added.  Where the mean is small
    against the spread this is a few u |y|; on the group at mean 4096 it is dwarfed by what the mean's own error already allows.
  * backward group sums (sum g w, sum g w xhat): a lane adds its 4 channels' terms over the 2 * 16 pixels its wave owns in a unit
    of ``UNIT`` = 128 pixels (32), the 4 channels (2), the lane pair (1), the 4 waves (3): ``BWD_GROUP_DEPTH`` = 38 within a unit;
    the units merge in float64, one rounding.
  * dweight / dbias: "fp32 within a slot, fp64 across slots".  A slot is a unit of one image: a term passes through the 32 pixels
    of its wave and the 3 additions of the 4 waves, ``SLOT_DEPTH`` = 35; then  slots * 2^-53 sum |terms|  and one rounding.
"""
import numpy as np

import add_norm_ref64 as A
from add_norm_ref64 import Inadmissible, U, add, inp, mul, ratio, rsqrt, rsum, scale, sub, table, widen16, within  # noqa: F401

F = np.float32
CHANNELS, GROUPS, CG = 256, 32, 8
CHUNK, TILE, UNIT = 8192, 64, 128              # kChunk, kTile, kUnit of csrc/group_norm_tokens.hip (the mirror exposes them)
GROUP_DEPTH = 2 + CHUNK // (256 * 4) + 6 + 3   # 19
BWD_GROUP_DEPTH = 2 * (TILE // 4) + 2 + 1 + 3  # 38
SLOT_DEPTH = 2 * (TILE // 4) + 3               # 35
MUTANTS = ("unbiased_variance", "eps_outside_sqrt", "one_pass_variance", "level_params_swapped", "group_of_4_channels",
           "rows_in_nchw_order", "gq_dropped", "dweight_without_xhat", "mean_over_hw_only")


_FLOAT64 = False        # ``float64_rounding``: the same tree with u = 2^-53 and every sum as deep as it has terms


def _u():
    return A.U


def _depth(fp32_depth, terms):
    """additions a term of a sum passes through: the kernel's depth, or -- for a float64 evaluation of unknown order -- at most
    the number of terms"""
    return terms if _FLOAT64 else fp32_depth


def _round(a):
    return A._r(*a)


def _exact_mul(a, b):
    """the product of two pairs carried in float64: no fp32 rounding"""
    return a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]


def _sq_dev_sum(part, mc):
    """sum over the last axis of (x - m)^2 for exact x and the exact mean of these x known as the pair ``mc``.  The kernel's m
    is off by some |delta| <= mc[1], and because the deviations from the exact mean add up to zero,
    sum (x - m)^2 = sum (x - mean)^2 + n delta^2  exactly: the mean's error enters in second order only.  The roundings: one for
    the difference, two for its square (relative 2 u from the rounded difference, u from the product), GROUP_DEPTH for the sum,
    each on a term no larger than (|x - mean| + |delta|)^2."""
    if _FLOAT64:          # an implementation of unknown order (Welford updates, say) feels the mean's rounding in first order
        d = sub(part, mc)
        return rsum(mul(d, d), part[0].shape[-1])
    d = part[0] - mc[0]
    n = part[0].shape[-1]
    mag = ((np.abs(d) + mc[1]) ** 2).sum(-1, keepdims=True)
    return (d * d).sum(-1, keepdims=True), n * mc[1] ** 2 + (GROUP_DEPTH + 3) * _u() * mag * (1 + 4 * _u()) + n * A.TINY


def group_stats(xg, eps):
    """xg: pair of (..., n) arrays, one group per row -> pairs mean, rstd of shape (..., 1)"""
    n = xg[0].shape[-1]
    chunks = -(-n // CHUNK)
    total = rsum(xg, _depth(GROUP_DEPTH, n))
    total = total[0], total[1] + chunks * 2.0 ** -53 * np.abs(xg[0]).sum(-1, keepdims=True)
    mean = _round(scale(total, 1.0 / n))
    m2 = (np.zeros_like(mean[0]), np.zeros_like(mean[1]))
    for c in range(chunks):
        part = xg[0][..., c * CHUNK:(c + 1) * CHUNK], xg[1][..., c * CHUNK:(c + 1) * CHUNK]
        cnt = part[0].shape[-1]
        mc = mean if chunks == 1 else _round(scale(rsum(part, _depth(GROUP_DEPTH, cnt)), 1.0 / cnt))
        inside = _sq_dev_sum(part, mc)
        m2 = m2[0] + inside[0], m2[1] + inside[1]
        if chunks > 1:
            dm = sub(mc, mean)
            between = scale(_exact_mul(dm, dm), float(cnt))
            m2 = m2[0] + between[0], m2[1] + between[1]
    m2 = m2[0], m2[1] + chunks * 2.0 ** -52 * np.abs(m2[0])
    var = _round(scale(m2, 1.0 / n))
    return mean, rsqrt(add(var, inp(F(eps))))


def _bsum(a, n):
    """a backward group sum over the last axis divided by n: fp32 within a unit, float64 across units, one rounding"""
    s = rsum(a, _depth(BWD_GROUP_DEPTH, n))
    return _round(scale(s, 1.0 / n))


def _colsum(a, slots):
    """sum over axis 0 of a (rows, 256) pair: fp32 within a slot, float64 across the slots, one rounding"""
    mag = (np.abs(a[0]) + a[1]).sum(0)
    return _round((a[0].sum(0), a[1].sum(0) + _depth(SLOT_DEPTH, a[0].shape[0]) * _u() * mag + slots * 2.0 ** -53 * mag))


def level_rows(case):
    hw = [h * w for h, w in case["shapes"]]
    starts = np.concatenate([[0], np.cumsum(hw)]).astype(int)
    return hw, starts


def ref64(case):
    """case: dict(shapes [(H, W)], xs [(N, 256, H, W)], weights, biases [(256,)], eps, pos | None (N, S, 256), gy | None, gq | None)
    -> dict of pairs: tokens, q (if pos), mean, rstd (N, levels, 32) and, where an upstream gradient is given, dx<l> per level,
    dweight, dbias (levels, 256)."""
    with np.errstate(all="ignore"):
        hw, starts = level_rows(case)
        n_img, levels = case["xs"][0].shape[0], len(hw)
        toks, means, rstds, saved = [], [], [], []
        for l in range(levels):
            x = inp(np.asarray(case["xs"][l], F).reshape(n_img, GROUPS, CG * hw[l]))
            mean, rstd = group_stats(x, case["eps"])
            xh = mul(sub(x, mean), rstd)
            w = inp(np.repeat(np.asarray(case["weights"][l], F).reshape(GROUPS, CG), hw[l], axis=1)[None])
            b = inp(np.repeat(np.asarray(case["biases"][l], F).reshape(GROUPS, CG), hw[l], axis=1)[None])
            y = add(mul(xh, w), b)
            y = y[0], y[1] + 2 * _u() * (np.abs(x[0]) + np.abs(mean[0])) * np.abs(rstd[0] * w[0]) + _u() * np.abs(b[0])   # the other factorisation
            toks.append(tuple(a.reshape(n_img, CHANNELS, hw[l]).transpose(0, 2, 1) for a in y))
            means.append(tuple(a[..., 0] for a in mean))
            rstds.append(tuple(a[..., 0] for a in rstd))
            saved.append((x, mean, rstd, xh, w))
        tokens = tuple(np.concatenate([t[k] for t in toks], 1) for k in (0, 1))
        out = dict(tokens=tokens, mean=tuple(np.stack([m[k] for m in means], 1) for k in (0, 1)),
                   rstd=tuple(np.stack([m[k] for m in rstds], 1) for k in (0, 1)))
        if case["pos"] is not None:
            out["q"] = add(tokens, inp(case["pos"]))
        gy, gq = case["gy"], case["gq"]
        if gy is None and gq is None:
            return out
        g_all = inp(gy) if gq is None else inp(gq) if gy is None else add(inp(gy), inp(gq))
        dws, dbs = [], []
        for l in range(levels):
            x, mean, rstd, xh, w = saved[l]
            rows = tuple(a[:, starts[l]:starts[l + 1]] for a in g_all)                       # (N, hw, 256)
            g = tuple(a.transpose(0, 2, 1).reshape(n_img, GROUPS, CG * hw[l]) for a in rows)
            gw = mul(g, w)
            c1 = _bsum(gw, CG * hw[l])
            c2 = _bsum(mul(gw, xh), CG * hw[l])
            dx = mul(rstd, sub(sub(gw, c1), mul(xh, c2)))
            out[f"dx{l}"] = tuple(a.reshape((n_img, CHANNELS) + tuple(case["shapes"][l])) for a in dx)
            slots = n_img * -(-hw[l] // UNIT)
            per_row = lambda a: tuple(v.reshape(n_img, CHANNELS, hw[l]).transpose(0, 2, 1).reshape(-1, CHANNELS) for v in a)  # noqa: E731
            dws.append(_colsum(per_row(mul(g, xh)), slots))
            dbs.append(_colsum(per_row(g), slots))
        out["dweight"] = tuple(np.stack([d[k] for d in dws]) for k in (0, 1))
        out["dbias"] = tuple(np.stack([d[k] for d in dbs]) for k in (0, 1))
        return out


def float64_rounding(case):
    """The statement's tree evaluated for FLOAT64 arithmetic: the same pairs with u = 2^-53 and, because nothing is known
    about the order in which a float64 implementation adds, every sum bounded by  count * 2^-53 * sum |terms|  with count the
    number of its terms (8 H W for a group, N H W for a parameter gradient).  ``err`` of an element is then what one float64
    evaluation of the formulas -- this module's own values, or torch's float64 ops -- can be off by from the real-number
    result, through that element's own group: its own sum |terms|, its own rstd."""
    global _FLOAT64
    saved = A.U, A.TINY
    try:
        _FLOAT64, A.U, A.TINY = True, 2.0 ** -53, 2.0 ** -1000
        return ref64(case)
    finally:
        _FLOAT64 = False
        A.U, A.TINY = saved


def check_gn_tokens(case, got, name, ref=None, dtypes=None):
    """got: dict with any of tokens, q, mean, rstd, dx<l>, dweight, dbias -> {output: worst |err| / bound}; raises Inadmissible
    naming the case, the output and the index.  An output the statement has and ``got`` lacks is not judged.  ``dtypes``: {output:
    'fp16' | 'bf16'} for the outputs that were rounded once into that type (``widen16``)."""
    ref = ref64(case) if ref is None else ref
    rep = {}
    for k, v in got.items():
        if k not in ref:
            raise Inadmissible(f"{name}: {k} given but the case has no statement for it")
        a = widen16(ref[k], (dtypes or {}).get(k))
        within(f"{name}: {k}", v, a)
        rep[k] = ratio(v, a)
    return rep


# ------------------------------------------------------------------------------------------------------------------
# an fp32 evaluation of the same formulas (sums in float64, rounded once: well inside), and its mutants
# ------------------------------------------------------------------------------------------------------------------
def eval_f32(case, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    with np.errstate(all="ignore"):
        hw, starts = level_rows(case)
        n_img, levels = case["xs"][0].shape[0], len(hw)
        eps = F(case["eps"])
        groups = 2 * GROUPS if mutant == "group_of_4_channels" else CHANNELS if mutant == "mean_over_hw_only" else GROUPS
        cg = CHANNELS // groups
        toks, means, rstds, saved = [], [], [], []
        for l in range(levels):
            x = np.asarray(case["xs"][l], F).reshape(n_img, groups, cg * hw[l])
            n = x.shape[-1]
            mean = (x.astype(np.float64).sum(-1, keepdims=True) / n).astype(F)
            d = x - mean
            if mutant == "one_pass_variance":
                var = ((x.astype(np.float64) ** 2).sum(-1, keepdims=True) / n).astype(F) - mean * mean
            else:
                var = ((d.astype(np.float64) ** 2).sum(-1, keepdims=True) / (n - 1 if mutant == "unbiased_variance" else n)).astype(F)
            rstd = (F(1) / (np.sqrt(var) + eps) if mutant == "eps_outside_sqrt" else F(1) / np.sqrt(var + eps)).astype(F)
            lp = (l + 1) % levels if mutant == "level_params_swapped" else l
            w = np.repeat(np.asarray(case["weights"][lp], F).reshape(groups, cg), hw[l], axis=1)[None]
            b = np.repeat(np.asarray(case["biases"][lp], F).reshape(groups, cg), hw[l], axis=1)[None]
            xh = d * rstd
            y = (xh * w + b).reshape(n_img, CHANNELS, hw[l])
            toks.append(y.reshape(n_img, hw[l], CHANNELS) if mutant == "rows_in_nchw_order" else y.transpose(0, 2, 1))
            means.append(mean.reshape(n_img, groups)[:, :GROUPS])
            rstds.append(rstd.reshape(n_img, groups)[:, :GROUPS])
            saved.append((rstd, xh, w))
        out = dict(tokens=np.concatenate(toks, 1), mean=np.stack(means, 1), rstd=np.stack(rstds, 1))
        if case["pos"] is not None:
            out["q"] = out["tokens"] + np.asarray(case["pos"], F)
        gy, gq = case["gy"], case["gq"]
        if gy is None and gq is None:
            return out
        g_all = np.asarray(gy if gq is None else gq if gy is None else np.asarray(gy, F) + np.asarray(gq, F), F)
        g_dx = np.asarray(gy, F) if mutant == "gq_dropped" and gy is not None and gq is not None else g_all
        dws, dbs = [], []
        for l in range(levels):
            rstd, xh, w = saved[l]
            n = xh.shape[-1]

            def grouped(a):
                return a[:, starts[l]:starts[l + 1]].transpose(0, 2, 1).reshape(n_img, groups, n)
            g, gd = grouped(g_all), grouped(g_dx)
            gw = gd * w
            c1 = (gw.astype(np.float64).sum(-1, keepdims=True) / n).astype(F)
            c2 = ((gw * xh).astype(np.float64).sum(-1, keepdims=True) / n).astype(F)
            out[f"dx{l}"] = (rstd * ((gw - c1) - xh * c2)).reshape((n_img, CHANNELS) + tuple(case["shapes"][l]))
            term = g if mutant == "dweight_without_xhat" else g * xh
            dws.append(term.reshape(n_img, CHANNELS, hw[l]).astype(np.float64).sum((0, 2)).astype(F))
            dbs.append(g.reshape(n_img, CHANNELS, hw[l]).astype(np.float64).sum((0, 2)).astype(F))
        out["dweight"], out["dbias"] = np.stack(dws), np.stack(dbs)
        return out

"""Plain float64 statement of csrc/ref_points.hip -- box refinement through ``inverse_sigmoid``, valid-ratio scaling, the sine
embedding of the query boxes and the backward of all three -- each result carried as a (value, err) pair in the arithmetic of
tests/assign_ref64.py, and the checker that decides whether a result (from the GPU, or from torch's fp32 evaluation of
tests/ref_points_torch_restated.py) is ADMISSIBLE against it.

Test helper (not a conftest; imported by name like dn_ref64.py / loss_ref64.py).  Numpy only.

Conventions: those of assign_ref64.py (u = 2^-24; + - * / , expf and logf are allowed one ulp = 2u |result| each plus 2^-126 for a
flushed subnormal; a bound that is not finite means "no statement"; nothing scaled per test), plus:

  * exact operations.  Where both operands are exact and the float64 result is itself an fp32 number, the fp32 result IS that
    number and no rounding is charged (``1 - x`` for x in [0.5, 1], ``y * 1``).
  * what a stage reads is exact.  The kernel's stages hand fp32 (or 16-bit) numbers on: the scale reads the ROUNDED refined
    points, the embedding reads level 0 of ``ref_input``, the backward reads the stored ``new_ref``.  Each stage is therefore
    judged from the numbers the stage before it actually produced, which the check before it has bounded: the bounds are those
    of one stage and do not compound.
  * the embedding's argument ``coord * 2 pi / dim_t[j]``: relative error 2u (the product and the quotient, half an ulp each)
    plus the relative error of fp32(2 pi), ``REL_2PI``; propagated with |d sin| , |d cos| <= 1.  ``sinf`` / ``cosf``: 2 ulp of
    the result, the ulp being the fp32 spacing at the float64 value (not below 2^-149).  dim_t is the table the kernel is
    handed: exact.
  * 16-bit results: half an ulp of the 16-bit format at the far end of the fp32 interval, on top of the fp32 bound.
  * the embedding's backward: term_j = (g_j * cosf(arg_j)) / dim_t[j] (odd j: -sinf): |g_j| (argument error + 2 ulp) / dim_t[j]
    plus the two roundings; the 128 terms are added four per lane in index order and then by five butterfly steps: no partial
    sum passes more than ``SUM_DEPTH`` = 8 additions, each 2u sum |term|.
  * gradient kinks (x against 0, 1 and eps; 1 - x against eps).  The operands are exact here, so every gate is decided by the
    fp32 comparison itself and torch's rule holds with no allowance: the gradient passes at equality.  A gate whose operand
    carries an error that straddles the kink admits the hull of its two branches and counts as OPEN (``grad`` returns the
    count): with exact inputs that can only be ``1 - x`` where the difference is not an fp32 number, which puts it far above eps,
    so no element of any case is open.
"""
import itertools

import numpy as np

from assign_ref64 import TINY, U, Inadmissible, add, bound, div, exp_, fmax, log_, mul, neg, sub

F = np.float32
TWO_PI = 2.0 * np.pi
TWO_PI32 = float(F(TWO_PI))
REL_2PI = abs(TWO_PI32 - TWO_PI) / TWO_PI
SUM_DEPTH = 8
SINCOS_ULPS = 2.0
BLOCK = 128
BLOCK_COORD = (1, 0, 2, 3)                      # the blocks (y, x, w, h) as coordinate indices
NONE, SIGMOID, REFINE = 0, 1, 2
DTYPES = {"fp32": (24, -126), "fp16": (11, -14), "bf16": (8, -126)}      # significand bits, smallest normal exponent


def exact(x):
    """Numbers the kernel reads: exact.  float64 in, so that a float64 chain passes through unchanged."""
    x = np.asarray(x, np.float64)
    return x, np.zeros_like(x)


def ulp(v, dtype="fp32"):
    """The spacing of ``dtype`` at |v| (at the smallest normal for anything below it)."""
    bits, emin = DTYPES[dtype]
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** emin)))
    return np.where(np.isfinite(e), 2.0 ** (np.maximum(e, emin) - (bits - 1)), np.inf)


def stored(a, dtype):
    """A pair rounded once to ``dtype`` for storing: half an ulp at the far end of its interval (fp32: already counted)."""
    if dtype == "fp32":
        return a
    return a[0], a[1] + 0.5 * ulp(np.abs(a[0]) + np.where(np.isfinite(a[1]), a[1], 0.0), dtype)


def _x(op):
    def f(a, b):
        with np.errstate(all="ignore"):
            v, e = op(a, b)
            v = np.asarray(v, np.float64)
            same = v.astype(F).astype(np.float64) == v
            ok = (np.asarray(a[1]) == 0) & (np.asarray(b[1]) == 0) & same & ((np.abs(v) >= TINY) | (v == 0))
        return v, np.where(ok, 0.0, e)
    return f


xadd, xsub, xmul, xdiv = _x(add), _x(sub), _x(mul), _x(div)
ONE = exact(1.0)


def sigmoid(x):
    """1 / (1 + expf(-x)); an expf that overflows in every precision gives an exact 0 (1 / inf)"""
    with np.errstate(all="ignore"):
        ex = exp_(neg(x))
        p = xdiv(ONE, xadd(ONE, ex))
        over = np.isposinf(ex[0]) | (x[0] < -88.8)
        one = np.isposinf(x[0])
        v = np.where(over, 0.0, np.where(one, 1.0, p[0]))
        e = np.where(over, TINY, np.where(one, 0.0, p[1]))
        return np.where(np.isnan(x[0]), np.nan, v), e


def inverse_sigmoid(x, eps, mutant=None):
    """transformer.py:435-451 on a pair; eps is the fp32 number the C ABI carries"""
    with np.errstate(all="ignore"):
        eps = exact(float(F(eps)))
        xc = (np.clip(x[0], 0.0, 1.0), x[1])
        om = xsub(ONE, xc)
        x1, x2 = fmax(xc, eps), fmax(om, eps)
        return log_(xdiv(x1, x2))


def refine(mode, delta, ref, eps, dtype="fp32"):
    """the refined points as stored: (value, err)"""
    with np.errstate(all="ignore"):
        if mode == NONE:
            return ref
        y = sigmoid(ref) if mode == SIGMOID else sigmoid(xadd(delta, inverse_sigmoid(ref, eps)))
        return stored(y, dtype)


def _ratio4(vr, width):
    """valid_ratios (bs, L, 2) -> (1, bs, L, width): (vx, vy, vx, vy)"""
    vr = np.asarray(vr, np.float64)
    return np.concatenate([vr, vr], -1)[None, :, :, :width]


def scale(y, vr):
    """ref_input (nq, bs, L, width) of the stored points y (nq, bs, width)"""
    width = y[0].shape[-1]
    return xmul((y[0][:, :, None, :], y[1][:, :, None, :]), exact(_ratio4(vr, width)))


def _argument(coord, dim_t):
    """coord (.., ) pair -> argument pair (.., 128)"""
    d = np.asarray(dim_t, np.float64)
    arg = coord[0][..., None] * TWO_PI / d
    return arg, np.abs(arg) * (2 * U + REL_2PI) + coord[1][..., None] * TWO_PI / d + TINY


def embed(coords, dim_t):
    """gen_sineembed_for_position of coords (nq, bs, width) -> (nq, bs, 128 * width) pair"""
    vals, errs = [], []
    even = (np.arange(BLOCK) % 2 == 0)
    for k in BLOCK_COORD[:coords[0].shape[-1]]:
        arg, ea = _argument((coords[0][..., k], coords[1][..., k]), dim_t)
        v = np.where(even, np.sin(arg), np.cos(arg))
        vals.append(v)
        errs.append(ea + SINCOS_ULPS * ulp(v))
    return np.concatenate(vals, -1), np.concatenate(errs, -1)


def embed_grad(coords, dim_t, g_embed):
    """d sum(embed * g_embed) / d coords (nq, bs, width) as a pair: the sum over each block's 128 terms and the factor 2 pi"""
    d = np.asarray(dim_t, np.float64)
    g = np.asarray(g_embed, np.float64)
    even = (np.arange(BLOCK) % 2 == 0)
    vals, errs = [], []
    width = coords[0].shape[-1]
    for b, k in enumerate(BLOCK_COORD[:width]):
        arg, ea = _argument((coords[0][..., k], coords[1][..., k]), dim_t)
        gb = g[..., b * BLOCK:(b + 1) * BLOCK]
        trig = np.where(even, np.cos(arg), -np.sin(arg))
        term = gb * trig / d
        eterm = np.abs(gb) * (ea + SINCOS_ULPS * ulp(trig)) / d + 2 * 2 * U * np.abs(term) + 2 * TINY
        s = term.sum(-1)
        es = eterm.sum(-1) + SUM_DEPTH * 2 * U * np.abs(term).sum(-1)
        v = s * TWO_PI
        vals.append((k, v, es * TWO_PI + np.abs(v) * (REL_2PI + 2 * U) + TINY))
    vals.sort(key=lambda t: t[0])
    return np.stack([t[1] for t in vals], -1), np.stack([t[2] for t in vals], -1)


def _gate(d, exclusive=False):
    """(selector of d >= 0, open): open where the operand's error straddles the kink"""
    val = (d[0] > 0) if exclusive else (d[0] >= 0)
    return val.astype(np.float64), (np.abs(d[0]) <= d[1]) & (d[1] > 0)


def slope(ref, eps, mutant=None):
    """d inverse_sigmoid / d x as a pair, and the mask of open elements"""
    with np.errstate(all="ignore"):
        excl = mutant == "clamp_grad_exclusive"
        eps = exact(float(F(eps)))
        om = xsub(ONE, ref)
        gates = [_gate(ref, excl), _gate(om, excl), _gate(xsub(ref, eps), excl), _gate(xsub(om, eps), excl)]
        t1, t2 = xdiv(ONE, fmax(ref, eps)), xdiv(ONE, fmax(om, eps))
        lo, hi = None, None
        for corner in itertools.product((0, 1), repeat=4):
            sel = [np.where(op, float(c), val) for c, (val, op) in zip(corner, gates)]
            inside = sel[0] * sel[1]
            both = add((t1[0] * sel[2], t1[1] * sel[2]), (t2[0] * sel[3], t2[1] * sel[3]))
            single = (t1[0] * sel[2] + t2[0] * sel[3], t1[1] * sel[2] + t2[1] * sel[3])
            v = np.where(sel[2] * sel[3] > 0, both[0], single[0]) * inside
            e = np.where(sel[2] * sel[3] > 0, both[1], single[1]) * inside
            v, e = np.where(inside > 0, v, 0.0), np.where(inside > 0, e, 0.0)
            lo = v - e if lo is None else np.minimum(lo, v - e)
            hi = v + e if hi is None else np.maximum(hi, v + e)
        opened = gates[0][1] | gates[1][1] | gates[2][1] | gates[3][1]
        return ((lo + hi) / 2, (hi - lo) / 2), opened


def grad(mode, y, ref, eps, g_new=None, vr=None, g_ref_input=None, g_emb=None, dim_t=None, coords=None, dtypes=("fp32", "fp32"),
         mutant=None):
    """The backward from what it reads -- y = new_ref as stored, ref, the upstream gradients (all exact) -- as pairs:
    ``{"g_delta", "g_ref"}`` (``g_delta`` only for REFINE) and the number of open elements.  ``coords``: level 0 of
    ``ref_input`` as the forward stored it (``fp32(y * vr[:, 0])``), needed with ``g_emb``.  ``dtypes``: of delta and of ref."""
    with np.errstate(all="ignore"):
        G = None if g_new is None else exact(g_new)
        width = ref[0].shape[-1]
        if g_ref_input is not None:
            r4 = _ratio4(vr, width)
            for l in range(r4.shape[2]):
                t = xmul(exact(np.asarray(g_ref_input, np.float64)[:, :, l, :]), exact(r4[:, :, l, :]))
                G = t if G is None else xadd(G, t)
        if g_emb is not None:
            t = mul(embed_grad(coords, dim_t, g_emb), exact(_ratio4(vr, width)[:, :, 0, :]))
            G = t if G is None else add(G, t)
        if mode == NONE:
            return {"g_ref": stored(G, dtypes[1])}, 0
        gd = mul(mul(G, xsub(ONE, y)), y)
        if mode == SIGMOID:
            return {"g_ref": stored(gd, dtypes[1])}, 0
        sl, opened = slope(ref, eps, mutant)
        return {"g_delta": stored(gd, dtypes[0]), "g_ref": stored(mul(gd, sl), dtypes[1])}, int(opened.sum())


def within(name, got, a):
    """Raise unless |got - value| <= err elementwise; a NaN statement asks for a NaN; a bound that is not finite asks for nothing"""
    got = np.asarray(got, np.float64)
    e = bound(a)
    with np.errstate(all="ignore"):
        nan = np.isnan(a[0])
        bad = np.where(nan, ~np.isnan(got), ~(np.abs(got - a[0]) <= e) & np.isfinite(e))
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise Inadmissible(f"{name}{list(i)}: got {got[i]!r}, fp64 {a[0][i]!r}, |diff| {abs(got[i] - a[0][i]):.3e} > "
                           f"allowance {e[i]:.3e}")


def ratio(got, a):
    """max |got - value| / err over the elements with a finite, positive bound and a finite value"""
    got = np.asarray(got, np.float64)
    e = bound(a)
    with np.errstate(all="ignore"):
        ok = np.isfinite(e) & (e > 0) & np.isfinite(a[0]) & np.isfinite(got)
        return float(np.max(np.abs(got - a[0])[ok] / e[ok])) if ok.any() else 0.0


def check(case, got, name="", mutant=None):
    """Every output and gradient of a case (tests/ref_points_cases.py) in ``got`` against the statement; ``got`` holds float
    arrays in the case's logical shapes: ``new_ref`` / ``g_delta`` / ``g_ref``: lists, one per segment; ``ref_input`` (nq, bs,
    L, width); ``embed``; keys that are absent are not judged, but a key needs the stage before it.  Returns ``{key: worst
    |diff| / bound}`` and, under "open" / "elements", the open gradient elements and their total."""
    mode, eps, out = case["mode"], case["eps"], {}
    opened = elements = 0
    for s, seg in enumerate(case["segments"]):
        ref = exact(seg["ref"])
        delta = exact(seg["delta"]) if mode == REFINE else None
        if mode != NONE and "new_ref" in got:
            a = refine(mode, delta, ref, eps, case["out_dtype"])
            within(f"{name} new_ref[{s}]", got["new_ref"][s], a)
            out["new_ref"] = max(out.get("new_ref", 0.0), ratio(got["new_ref"][s], a))
        y = ref if mode == NONE else exact(got["new_ref"][s])
        coords = None
        if s == 0 and case.get("vr") is not None and "ref_input" in got:
            a = scale(y, case["vr"])
            within(f"{name} ref_input", got["ref_input"], a)
            out["ref_input"] = ratio(got["ref_input"], a)
            coords = exact(np.asarray(got["ref_input"], np.float64)[:, :, 0, :])
            if "embed" in got:
                a = embed(coords, case["dim_t"])
                within(f"{name} embed", got["embed"], a)
                out["embed"] = ratio(got["embed"], a)
        if "g_ref" in got or "g_delta" in got:
            if coords is None and case.get("vr") is not None:
                coords = exact((np.asarray(y[0], F) * np.asarray(_ratio4(case["vr"], y[0].shape[-1])[:, :, 0, :], F)).astype(np.float64))
            first = s == 0 and case.get("vr") is not None
            stmt, n = grad(mode, y, ref, eps, seg.get("g_new"), case.get("vr"), case.get("g_ref_input") if first else None,
                           case.get("g_embed") if first else None, case.get("dim_t"), coords,
                           (case.get("delta_dtype", "fp32"), case["ref_dtype"]), mutant)
            opened += n
            for key in ("g_delta", "g_ref"):
                if key in got and key in stmt and got[key][s] is not None:
                    within(f"{name} {key}[{s}]", got[key][s], stmt[key])
                    out[key] = max(out.get(key, 0.0), ratio(got[key][s], stmt[key]))
                    elements += int(np.asarray(got[key][s]).size)
    out["open"], out["elements"] = opened, elements
    return out


def table(name, ratios):
    return f"  {name:34s} " + "  ".join(f"{k} {v:.2f}" if isinstance(v, float) else f"{k} {v}" for k, v in ratios.items())

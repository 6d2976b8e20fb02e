"""Plain float64 statement of csrc/add_norm.hip -- residual add, LayerNorm, positional add, and the backward -- each quantity
carried as a (value, err) pair through the expression tree, and the checkers that decide whether a result (from the GPU, from
torch's fp32 CPU ops, or from the fp32 numpy evaluation ``eval_f32`` below) is ADMISSIBLE against it.

Test helper (not a conftest; imported by name like msda_ref64.py / loss_ref64.py).  Numpy only.

Conventions
  * u = 2^-24.  Inputs are fp32 numbers: exact (err 0).  Every fp32 operation (+ - * / sqrt) is correctly rounded and adds
    u (|value| + err) to the propagated error -- one rounding per operation; a fused multiply-add has one rounding fewer and
    stays inside.  Multiplying by 1 / 256 is exact.
  * sums over the 256 columns of a row.  The bound is  depth * u * sum |terms|  plus the terms' own errors, independent of the
    ORDER of the additions: it holds for every reduction in which no term passes through more than ``ROW_DEPTH`` = 16
    additions -- any tree or butterfly over 256 terms (depth 8; the kernel's is 2 in the lane + 6 across lanes), 16 chains of
    16, vectors of Welford updates.  It is deliberately NOT the (n - 1) u of one chain over all 256 columns: on the row at mean
    4096 with spread 1e-2 that bound is 255 u 4096 = 0.06, six times the spread, i.e. no statement about y at all, and the
    ``E[s^2] - mu^2`` variance could not be told from the right one.
  * 1 / sqrt(var + eps) is evaluated at both ends of the interval of var + eps (not linearised); an interval that reaches zero
    gives a bound that is not finite = "no statement": such an element must still be finite.
  * the backward's xhat is (x + residual - mean) * rstd with the forward's mean and rstd: their pairs cover the fp32 numbers
    the forward saved.
  * dweight / dbias: "fp32 within a slot, fp64 across slots".  A term passes through at most ``SLOT_DEPTH`` = 19 fp32 additions
    (the 16 rows of its wave, the 3 additions of the 4 waves), hence 19 u sum |terms| over ALL rows (the slots' bounds add up),
    then  slots * 2^-53 sum |terms|  for the fp64 additions and one rounding to fp32.  A whole-column fp32 chain over thousands
    of rows is outside (and torch's CPU backward, which adds per thread, is inside on every case of add_norm_cases.py).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
ROW_DEPTH = 16
SLOT_ROWS, SLOT_DEPTH = 64, 19
DIM = 256
F = np.float32
MUTANTS = ("unbiased_variance", "eps_outside_sqrt", "residual_dropped", "pos_before_norm", "one_pass_variance", "gq_dropped",
           "dweight_without_xhat", "mean_g_not_gw")


class Inadmissible(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------
# (value, err) arithmetic
# ------------------------------------------------------------------------------------------------------------------
def inp(a):
    v = np.asarray(a, F).astype(np.float64)
    return v, np.zeros_like(v)


def _r(v, e):
    return v, e + U * (np.abs(v) + e) + TINY


def add(a, b):
    return _r(a[0] + b[0], a[1] + b[1])


def sub(a, b):
    return _r(a[0] - b[0], a[1] + b[1])


def mul(a, b):
    return _r(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def rsum(a, depth, axis=-1, keepdims=True):
    return a[0].sum(axis, keepdims=keepdims), (a[1] + depth * U * (np.abs(a[0]) + a[1])).sum(axis, keepdims=keepdims)


def scale(a, m):
    return a[0] * m, a[1] * abs(m)


def rsqrt(a):
    """1 / sqrt(a) of a >= 0, at both ends of a's interval, then the two roundings of sqrt and /"""
    with np.errstate(all="ignore"):
        v, e = a
        val = 1.0 / np.sqrt(v)
        lo, hi = v - e, v + e
        err = np.where(lo > 0, np.maximum(1.0 / np.sqrt(np.where(lo > 0, lo, 1.0)) - val, val - 1.0 / np.sqrt(hi)), np.inf)
        return _r(*_r(val, err))


def colsum(a, rows):
    """sum over the rows (axis 0) of a (rows, 256) pair: fp32 within a slot, fp64 across slots, one rounding"""
    slots = -(-rows // SLOT_ROWS)
    mag = (np.abs(a[0]) + a[1]).sum(0)
    return _r(a[0].sum(0), a[1].sum(0) + SLOT_DEPTH * U * mag + slots * 2.0 ** -53 * mag)


# ------------------------------------------------------------------------------------------------------------------
# the statement
# ------------------------------------------------------------------------------------------------------------------
def _flat(a):
    return None if a is None else np.asarray(a, F).reshape(-1, DIM)


def ref64(case):
    """case: dict(x, residual | None, pos | None, weight, bias, eps, gy | None, gq | None), arrays (..., 256) ->
    dict of pairs: y, q (if pos), mean, rstd, and, where an upstream gradient is given, dx, dweight, dbias."""
    with np.errstate(all="ignore"):
        x, res, pos, gy, gq = (_flat(case[k]) for k in ("x", "residual", "pos", "gy", "gq"))
        rows = x.shape[0]
        w, b = inp(case["weight"]), inp(case["bias"])
        s = inp(x) if res is None else add(inp(x), inp(res))
        mu = scale(rsum(s, ROW_DEPTH), 1.0 / DIM)
        d = sub(s, mu)
        var = scale(rsum(mul(d, d), ROW_DEPTH), 1.0 / DIM)
        rstd = rsqrt(add(var, inp(F(case["eps"]))))
        xh = mul(d, rstd)
        y = add(mul(xh, w), b)
        out = dict(y=y, mean=(mu[0][:, 0], mu[1][:, 0]), rstd=(rstd[0][:, 0], rstd[1][:, 0]))
        if pos is not None:
            out["q"] = add(y, inp(pos))
        if gy is None and gq is None:
            return out
        g = inp(gy) if gq is None else inp(gq) if gy is None else add(inp(gy), inp(gq))
        gw = mul(g, w)
        c1 = scale(rsum(gw, ROW_DEPTH), 1.0 / DIM)
        c2 = scale(rsum(mul(gw, xh), ROW_DEPTH), 1.0 / DIM)
        out["dx"] = mul(rstd, sub(sub(gw, c1), mul(xh, c2)))
        out["dweight"] = colsum(mul(g, xh), rows)
        out["dbias"] = colsum(g, rows)
        return out


# ------------------------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------------------------
def ratio(got, a):
    """largest |got - value| / err over the elements that have a statement (0 / 0 counts as 0)"""
    got = np.asarray(got, np.float64).reshape(np.shape(a[0]))
    with np.errstate(all="ignore"):
        diff = np.abs(got - a[0])
        ok = np.isfinite(a[1])
        r = np.where(diff == 0, 0.0, diff / a[1])
        return float(np.max(r[ok])) if ok.any() else 0.0


def within(name, got, a):
    got = np.asarray(got, np.float64)
    if got.size != np.size(a[0]):
        raise Inadmissible(f"{name}: {got.size} elements, expected {np.size(a[0])}")
    got = got.reshape(np.shape(a[0]))
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(got) | (np.isfinite(a[1]) & ~(np.abs(got - a[0]) <= a[1]))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise Inadmissible(f"{name}{list(i)}: got {got[i]!r}, float64 {a[0][i]!r}, bound {a[1][i]:.3e} "
                           f"(off by {abs(got[i] - a[0][i]):.3e}; {int(bad.sum())} of {bad.size} elements outside)")


def widen16(a, dtype):
    """The pair of a result that leaves in a 16-bit type (``'fp16'`` / ``'bf16'``): the fp32 bound widened by the one output
    rounding, B + u16 (|ref| + B) + s16 (tests/msda_h16_ref.py).  ``None``: the pair as it is.  The inputs of such a case are
    16-bit numbers held in fp32 (exact), so the statement itself is unchanged."""
    if dtype is None:
        return a
    from msda_h16_ref import widen16 as widen
    with np.errstate(invalid="ignore"):
        return a[0], widen(a[1], a[0], dtype)


def check_add_norm(case, got, name, ref=None, dtypes=None):
    """got: dict with any of y, q, mean, rstd, dx, dweight, dbias -> {output: worst |err| / bound}; raises Inadmissible naming
    the case, the output and the index.  An output the statement has and ``got`` lacks is not judged.  ``dtypes``: {output:
    'fp16' | 'bf16'} for the outputs that were rounded once into that type (``widen16``); every other output keeps the fp32
    bound."""
    ref = ref64(case) if ref is None else ref
    rep = {}
    for k, v in got.items():
        if k not in ref:
            raise Inadmissible(f"{name}: {k} given but the case has no statement for it")
        a = widen16(ref[k], (dtypes or {}).get(k))
        within(f"{name}: {k}", v, a)
        rep[k] = ratio(v, a)
    return rep


def table(name, rep):
    return f"  {name:34s} " + " ".join(f"{k}={v:.3g}" for k, v in rep.items())


# ------------------------------------------------------------------------------------------------------------------
# an honest fp32 evaluation of the same formulas (a cast after every operation; row sums as a pairwise tree), and its mutants
# ------------------------------------------------------------------------------------------------------------------
def _tree(a):
    a = np.asarray(a, F)
    while a.shape[-1] > 1:
        a = (a[..., 0::2] + a[..., 1::2]).astype(F)
    return a


def eval_f32(case, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    with np.errstate(all="ignore"):
        x, res, pos, gy, gq = (_flat(case[k]) for k in ("x", "residual", "pos", "gy", "gq"))
        w, b, eps = np.asarray(case["weight"], F), np.asarray(case["bias"], F), F(case["eps"])
        inv = F(1.0 / DIM)
        s = x if res is None or mutant == "residual_dropped" else x + res
        if mutant == "pos_before_norm" and pos is not None:
            s = s + pos
        mu = _tree(s) * inv
        d = s - mu
        if mutant == "one_pass_variance":
            var = _tree(s * s) * inv - mu * mu
        elif mutant == "unbiased_variance":
            var = _tree(d * d) * F(1.0 / (DIM - 1))
        else:
            var = _tree(d * d) * inv
        rstd = (F(1) / (np.sqrt(var) + eps) if mutant == "eps_outside_sqrt" else F(1) / np.sqrt(var + eps)).astype(F)
        xh = d * rstd
        y = xh * w + b
        out = dict(y=y, mean=mu[:, 0], rstd=rstd[:, 0])
        if pos is not None:
            out["q"] = y if mutant == "pos_before_norm" else y + pos
        if gy is None and gq is None:
            return out
        g = gy if gq is None else gq if gy is None else gy + gq
        gdx = gy if mutant == "gq_dropped" and gy is not None and gq is not None else g
        gw = gdx * w
        c1 = _tree(gdx if mutant == "mean_g_not_gw" else gw) * inv
        c2 = _tree(gw * xh) * inv
        out["dx"] = rstd * ((gw - c1) - xh * c2)
        out["dweight"] = (g if mutant == "dweight_without_xhat" else g * xh).astype(np.float64).sum(0).astype(F)
        out["dbias"] = g.astype(np.float64).sum(0).astype(F)
        return out

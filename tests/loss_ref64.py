"""Plain float64 statement of the loss kernels -- csrc/set_loss.hip (sigmoid focal, task-aligned focal, weighted L1, GIoU, the
dn targets, the fixed-order reduce, finalize and the backward) and csrc/tal_loss.hip -- value AND derivative, each carried as a
(value, err) pair in the arithmetic of tests/assign_ref64.py, and the checkers that decide whether a result (from the GPU, from
the C oracle, or from the fp32 numpy evaluation ``eval_f32`` below) is ADMISSIBLE against it.

Test helper (not a conftest; imported by name like msda_ref64.py / assign_ref64.py).  Numpy only: no call into oracle/ or the
library.  tests/set_loss_ref64.py stays the bare fp64 restatement; this module calls it for nothing but its constants and agrees
with its values to 1e-12 (tests/test_loss_ref64.py).

Conventions: those of assign_ref64.py (u = 2^-24, one ulp = 2u per operation, transcendentals included, 2^-126 per operation
for a flushed subnormal, a bound that is not finite means "no statement", nothing scaled per test), plus:

  * exact operations.  + - * / are correctly rounded in IEEE fp32, so where both operands are exact (err 0) and the fp64 result
    is itself an fp32 number, the fp32 result IS that number: no rounding is charged (``xadd`` ...).  This is what makes the
    corners of dyadic boxes on 512 / 1024 / 768-pixel images exact, and with them the ties of max / min.
  * sums.  set_loss adds fp32 elements in fp64: the bound of a statistic is the sum of its elements' bounds, n 2^-53 sum|x| for
    the fp64 additions, and -- where C % 4 == 0, so that the float4 path may run -- two fp32 roundings of each group of four
    classification elements, which that path adds in fp32 before widening.  A loss is (float)(sum * (double)scale): the product of
    the pairs and one rounding.  The count statistics (5, 6, 7) are decided from the fp32 inputs with fp32 arithmetic and carry no
    allowance.  tal_loss adds in fp32, per thread, then a 64-lane tree, four waves, and the partials in fp64: ``tal_depth``
    roundings of the running sum, each 2u sum|x|.
  * gradients.  Every product of the kernel's backward is stated in its order: co = scale x upstream, the element's derivative,
    their product; so the bound of an element is its derivative's error times |scale x coef| plus the roundings of the products.
  * kinks of the gradient (max / min operands, uraw / eraw against eps, the >= 0 gates, sign(b - t), sign(s - p), |s - p| > 0).
    Both operands the same expression of bitwise-identical fp32 inputs, or both exact and equal: the tie is exact and torch's
    rule holds with no allowance (0.5 to each side of a tied max / min, sign(0) = 0, 0 >= 0 true).  Intervals merely meet: the
    gradient is multi-affine in the selectors, so its range over them is spanned by the 0 / 1 corners; the statement is the hull of
    the corners' value +- err.  Surely apart: decided.
  * the task-aligned element in saturation follows the reference: log of the fp32 sigmoid, clamped at -100.  Where the interval of
    p or 1 - p reaches zero the clamped log lies in [-100, max(-100, log(upper end))]; the statement keeps the fp64 value and takes
    the farther end of that interval as its error, so the LOSS keeps a (wide) statement.  The gradient divides by
    max((1 - p) p, 1e-12), whose interval then reaches 1e-12 from both sides: no statement.  Whatever has no statement must still
    be finite, and no task-aligned loss may be negative.
"""
import itertools

import numpy as np

import set_loss_ref64 as R
from assign_ref64 import (TINY, U, Inadmissible, _f, _r, _within, add, bound, const, div, exp_, fabs, fmax, fmin, inp, log1p_,
                          log_, mul, neg, pow_, ratio, sub)

F = np.float32
MATCHED, DN, WARMUP = R.MATCHED, R.DN, R.WARMUP
TERMS = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
MUTANTS = ("tie_full", "gate_gt", "no_union_clamp_grad", "no_log_clamp", "no_bce_clamp", "pow_sign_dropped", "alpha_swapped",
           "any_w_as_sum_w", "l1_sign0_as_1", "half_precision_sigmoid")
MAX_OPEN = 8                      # more open selectors than this in one launch: their rows get no statement


# ------------------------------------------------------------------------------------------------------------------
# arithmetic on top of assign_ref64
# ------------------------------------------------------------------------------------------------------------------
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


def scal(a, m):
    """times an exact selector / sign in {-1, 0, 0.5, 1}: no rounding"""
    return a[0] * m, a[1] * np.abs(m)


def _sel(c, a, b):
    return np.where(c, a[0], b[0]), np.where(c, a[1], b[1])


def _bc(a, shape):
    return np.broadcast_to(a[0], shape).copy(), np.broadcast_to(a[1], shape).copy()


def _pow(a, g):
    g = float(g)
    v, e = a
    if g == 0.0:                                    # powf(x, 0) is exactly 1
        return np.ones_like(v), np.zeros_like(e)
    if 0.0 < g < 1.0:                               # concave: the lower end moves farther than the first order says
        pv = np.power(v, g)
        d = np.maximum(pv - np.power(np.maximum(v - e, 0.0), g), np.power(v + e, g) - pv)
        return _r(pv, np.where(e == 0, 0.0, d))
    return pow_(a, g)


def _clog(a):
    """max(logf(t), -100) of t >= 0; see the module docstring for the interval that reaches zero"""
    v, e = a
    lv, le = log_(a)
    res = fmax((lv, le), const(-100.0))
    hi = np.log(v + e)
    top = np.where(np.isfinite(hi), np.maximum(hi + 2 * U * np.abs(hi) + TINY, -100.0), np.where(hi < 0, -100.0, np.inf))
    none = ~np.isfinite(le)
    val = np.maximum(lv, -100.0)
    return np.where(none, val, res[0]), np.where(none, np.maximum(top - val, val + 100.0), res[1])


def _cmp(a, b, same=None):
    """selector d max(a, b) / d a in {0, 0.5, 1} and where it is OPEN (intervals meet, tie not exact)"""
    av, ae, bv, be = np.broadcast_arrays(a[0], a[1], b[0], b[1])
    m = np.where(av > bv, 1.0, np.where(av == bv, 0.5, 0.0))
    exact = (ae == 0) & (be == 0)
    if same is not None:
        m = np.where(same, 0.5, m)
        exact = exact | same
    return m, ~(np.abs(av - bv) > ae + be) & ~exact


def _gate(d):
    return (d[0] >= 0).astype(np.float64), (np.abs(d[0]) <= d[1]) & (d[1] > 0)


def _sign(d):
    """sign as a pair: exact where decided or where the difference is an exact zero, else anywhere in [-1, 1]"""
    op = (np.abs(d[0]) <= d[1]) & (d[1] > 0)
    return np.where(op, 0.0, np.sign(d[0])), op.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# elements: value and derivative, in the kernels' expression order
# ------------------------------------------------------------------------------------------------------------------
def focal_elem(x, t, alpha, gamma):
    """set_loss.hip focal_elem -> (loss, d loss / d x) pairs; x a pair, t bool"""
    with np.errstate(all="ignore"):
        one, zero = const(1.0), const(0.0)
        z = (np.where(t, -x[0], x[0]), x[1])
        al = const(alpha)
        a = _sel(t, al, xsub(one, al))
        ez = exp_((-np.abs(z[0]), z[1]))
        den = xadd(one, ez)
        big, small = xdiv(one, den), xdiv(ez, den)
        s, oms = _sel(z[0] >= 0, big, small), _sel(z[0] >= 0, small, big)
        sp = xadd(fmax(z, zero), log1p_(ez))
        sg = xmul(s, s) if gamma == 2.0 else _pow(s, gamma)
        asg = xmul(a, sg)
        dz = xmul(asg, xadd(xmul(xmul(const(gamma), oms), sp), s))
        return xmul(asg, sp), scal(dz, np.where(t, -1.0, 1.0))


def tal_elem(x, st, gamma, input_is_prob=False):
    """tal_elem of set_loss.hip and the body of tal_loss_kernel (one statement for both copies) -> (loss, d loss / d x)"""
    with np.errstate(all="ignore"):
        one = const(1.0)
        if input_is_prob:
            p = x
        else:
            ex = exp_(neg(x))
            p = xdiv(one, xadd(one, ex))
            over = ~np.isfinite(ex[0])                        # expf overflows in every precision: 1 / inf is an exact 0
            p = np.where(over, 0.0, p[0]), np.where(over, TINY, p[1])
        q = xsub(one, p)
        lp, l1p = _clog(p), _clog(q)
        ce = neg(xadd(xmul(st, lp), xmul(xsub(one, st), l1p)))
        d = xsub(st, p)
        ad = fabs(d)
        mod = xmul(ad, ad) if gamma == 2.0 else _pow(ad, gamma)
        if gamma == 2.0:
            dmod = xmul(const(-2.0), d)
        else:                                                 # ad > 0 ? -gamma powf(ad, gamma - 1) sign(d) : 0
            t = xmul(const(-gamma), _pow(ad, gamma - 1.0))
            op = (np.abs(d[0]) <= d[1]) & (d[1] > 0)
            far = float(gamma) * np.power(ad[0] + ad[1], gamma - 1.0) * (1 + 6 * U) + TINY
            zero = (d[0] == 0) & (d[1] == 0)
            dmod = (np.where(op | zero, 0.0, t[0] * np.sign(d[0])), np.where(zero, 0.0, np.where(op, far, t[1])))
        dce = xdiv(xsub(p, st), fmax(xmul(q, p), const(1e-12)))
        dp = xadd(xmul(dmod, ce), xmul(mod, dce))
        return xmul(mod, ce), (dp if input_is_prob else xmul(dp, xmul(p, q)))


def giou_elem(b, tg, fw, fh, eps):
    """giou_loss of set_loss.hip.  b, tg: four pairs each (cxcywh).  -> (loss pair, grad_fn, selectors) where selectors is a
    list of (m, open) and grad_fn(ms, c) gives d (c * loss) / d b as four pairs for the selector values ms."""
    half, zero, one = const(0.5), const(0.0), const(1.0)
    f = (fw, fh, fw, fh)
    e_ = const(eps)

    def corners(q):
        hw, hh = xmul(half, q[2]), xmul(half, q[3])
        return [xmul(xsub(q[0], hw), f[0]), xmul(xsub(q[1], hh), f[1]), xmul(xadd(q[0], hw), f[2]), xmul(xadd(q[1], hh), f[3])]

    p, g = corners(b), corners(tg)
    pw, ph = xsub(p[2], p[0]), xsub(p[3], p[1])
    a1, a2 = xmul(pw, ph), xmul(xsub(g[2], g[0]), xsub(g[3], g[1]))
    lt = [fmax(p[k], g[k]) for k in range(2)]
    rb = [fmin(p[k + 2], g[k + 2]) for k in range(2)]
    dw = [xsub(rb[k], lt[k]) for k in range(2)]
    wh = [fmax(dw[k], zero) for k in range(2)]
    elt = [fmin(p[k], g[k]) for k in range(2)]
    erb = [fmax(p[k + 2], g[k + 2]) for k in range(2)]
    dew = [xsub(erb[k], elt[k]) for k in range(2)]
    ewh = [fmax(dew[k], zero) for k in range(2)]
    ov = xmul(wh[0], wh[1])
    uraw = xsub(xadd(a1, a2), ov)
    u = fmax(uraw, e_)
    eraw = xmul(ewh[0], ewh[1])
    e = fmax(eraw, e_)
    loss = xsub(one, xsub(xdiv(ov, u), xdiv(xsub(e, u), e)))
    # the same expression of bitwise-identical inputs: corner k of the prediction IS corner k of the target
    same = [(b[k][0] == tg[k][0]) & (b[k + 2][0] == tg[k + 2][0]) & (b[k][1] == 0) & (tg[k][1] == 0) & (b[k + 2][1] == 0) &
            (tg[k + 2][1] == 0) for k in range(2)]
    sels = [_cmp(p[0], g[0], same[0]), _cmp(p[1], g[1], same[1]), _cmp(p[2], g[2], same[0]), _cmp(p[3], g[3], same[1]),
            _gate(dw[0]), _gate(dw[1]), _gate(dew[0]), _gate(dew[1]), _cmp(uraw, e_), _cmp(eraw, e_)]

    def grad_fn(ms, c):
        mlo, mhi, gi, ge, mu, me = ms[0:2], ms[2:4], ms[4:6], ms[6:8], ms[8], ms[9]
        dU = scal(xsub(xdiv(ov, xmul(u, u)), xdiv(one, e)), mu)
        dE = scal(xdiv(u, xmul(e, e)), me)
        dO = xsub(xdiv(const(-1.0), u), dU)
        dp = [neg(xmul(dU, ph)), neg(xmul(dU, pw)), xmul(dU, ph), xmul(dU, pw)]
        for k in range(2):
            dwh = scal(xmul(dO, wh[1 - k]), gi[k])
            dp[k + 2] = xadd(dp[k + 2], scal(dwh, 1.0 - mhi[k]))
            dp[k] = xsub(dp[k], scal(dwh, mlo[k]))
            dewh = scal(xmul(dE, ewh[1 - k]), ge[k])
            dp[k + 2] = xadd(dp[k + 2], scal(dewh, mhi[k]))
            dp[k] = xsub(dp[k], scal(dewh, 1.0 - mlo[k]))
        dp = [xmul(dp[k], xmul(f[k], c)) for k in range(4)]
        return [xadd(dp[0], dp[2]), xadd(dp[1], dp[3]), xmul(half, xsub(dp[2], dp[0])), xmul(half, xsub(dp[3], dp[1]))]

    return loss, grad_fn, sels


def _hull(fn, sels):
    """fn(ms) -> list of pairs.  The hull over the 0 / 1 corners of every open selector -> (list of pairs, rows that used it)."""
    ms = [m for m, _ in sels]
    base = fn(ms)
    open_ids = [i for i, (_, o) in enumerate(sels) if o.any()]
    if not open_ids:
        return base, np.zeros(np.shape(base[0][0]), bool)
    used = np.zeros(np.shape(base[0][0]), bool)
    n_open = np.zeros(used.shape, np.int64)
    for i in open_ids:
        used |= sels[i][1]
        n_open += sels[i][1]
    ids = open_ids[:MAX_OPEN]
    lo = [v - e for v, e in base]
    hi = [v + e for v, e in base]
    for corner in itertools.product((0.0, 1.0), repeat=len(ids)):
        trial = list(ms)
        for i, c in zip(ids, corner):
            trial[i] = np.where(sels[i][1], c, ms[i])
        for k, (v, e) in enumerate(fn(trial)):
            lo[k], hi[k] = np.minimum(lo[k], v - e), np.maximum(hi[k], v + e)
    out = []
    too_many = len(open_ids) > MAX_OPEN
    for k, (v, e) in enumerate(base):
        w = 0.5 * (hi[k] - lo[k])
        ok = np.isfinite(w) & ~(too_many & used)
        out.append((np.where(used & ok, 0.5 * (hi[k] + lo[k]), v), np.where(used, np.where(ok, w, np.inf), e)))
    return out, used


# ------------------------------------------------------------------------------------------------------------------
# one segment: rows, statistics, finalize, gradients
# ------------------------------------------------------------------------------------------------------------------
def _rows(seg):
    """-> labels (nl,B,Q) int, pos, lw pair, tg: four pairs, w: four pairs (all (nl,B,Q))"""
    x = np.asarray(seg["cls"], F)
    nl, B, Q, C = x.shape
    if seg["kind"] == DN:
        sp = seg["single_pad"]
        labels = np.full((B, Q), C, np.int64)
        gt = np.zeros((B, Q, 4), F)
        pos = np.zeros((B, Q), bool)
        lw = np.zeros((B, Q), F)
        for b in range(B):
            g = np.asarray(seg["gts"][b], F).reshape(-1, 4)
            G = len(g)
            lw[b] = 1.0 if G > 0 else 0.0
            j = np.arange(Q) % sp
            pos[b] = j < G
            labels[b, pos[b]] = np.asarray(seg["labs"][b], np.int64)[j[pos[b]]]
            gt[b, pos[b]] = g[j[pos[b]]]
        wh = np.asarray(seg["wh"], F)
        fw, fh = inp(wh[:, 0:1]), inp(wh[:, 1:2])
        gp = inp(gt)
        two = const(2.0)
        x1, y1 = xdiv((gp[0][..., 0], gp[1][..., 0]), fw), xdiv((gp[0][..., 1], gp[1][..., 1]), fh)
        x2, y2 = xdiv((gp[0][..., 2], gp[1][..., 2]), fw), xdiv((gp[0][..., 3], gp[1][..., 3]), fh)
        tg = [xdiv(xadd(x1, x2), two), xdiv(xadd(y1, y2), two), xsub(x2, x1), xsub(y2, y1)]
        tg = [_bc((np.where(pos, t[0], 0.0), np.where(pos, t[1], 0.0)), (nl, B, Q)) for t in tg]
        w = [_bc(inp(pos.astype(F)), (nl, B, Q)) for _ in range(4)]
        rep = lambda a: np.broadcast_to(a, (nl, B, Q)).copy()  # noqa: E731
        return rep(labels), rep(pos), inp(rep(lw)), tg, w
    labels = np.asarray(seg["labels"], np.int64).reshape(nl, B, Q)
    pos = (labels >= 0) & (labels < C)
    if seg["kind"] == WARMUP:
        lw = np.asarray(seg["metrics"], F).reshape(nl, B, Q)
    else:
        lw = np.ones((nl, B, Q), F) if seg.get("label_weights") is None else np.asarray(seg["label_weights"], F).reshape(nl, B, Q)
    bt = np.asarray(seg["bbox_targets"], F).reshape(nl, B, Q, 4)
    bw = np.asarray(seg["bbox_weights"], F).reshape(nl, B, Q, 4)
    if seg["kind"] == WARMUP:
        bw = bw * pos[..., None]
    return labels, pos, inp(lw), [inp(bt[..., k]) for k in range(4)], [inp(bw[..., k]) for k in range(4)]


def _sum(v, e, axes, extra=0.0):
    n = np.prod([v.shape[a] for a in axes])
    a = np.abs(v).sum(axes)
    return v.sum(axes), bound((v, e)).sum(axes) + n * 2.0 ** -53 * a + extra * a


def _cast(a):
    return _r(a[0], a[1])


def _fp32_counts(w):
    """statistics 6 and 7 and the gate wm != 0, with the kernel's own fp32 arithmetic on the fp32 weights"""
    w = [np.asarray(x[0], F) for x in w]
    wsum = (w[0] + w[1]) + (w[2] + w[3])
    return wsum, wsum / F(4.0), (w[0] > 0) | (w[1] > 0) | (w[2] > 0) | (w[3] > 0)


def segment_statement(seg, coef):
    """coef (nl, 5) fp32 upstream gradients -> dict of pairs: stats (nl,10), terms (nl,5), scales (nl,5), gcls, gbox, and
    hull_rows (box rows whose gradient is a hull)."""
    with np.errstate(all="ignore"):
        P = seg["params"]
        kind = seg["kind"]
        x = np.asarray(seg["cls"], F)
        bx = np.asarray(seg["boxes"], F)
        nl, B, Q, C = x.shape
        labels, pos, lw, tg, w = _rows(seg)
        onehot = labels[..., None] == np.arange(C)
        gamma = float(F(P["gamma"]))
        if kind == WARMUP:
            st = inp(np.where(onehot, lw[0][..., None], 0.0))
            cv, cd = tal_elem(inp(x), st, gamma)
        else:
            cv, dz = focal_elem(inp(x), onehot, P["alpha"], gamma)
            lw4 = (lw[0][..., None], lw[1][..., None])
            cv, cd = xmul(cv, lw4), xmul(dz, lw4)
        sv, se = np.zeros((nl, 10)), np.zeros((nl, 10))
        sv[:, 0], se[:, 0] = _sum(cv[0], cv[1], (1, 2, 3), extra=4 * U if C % 4 == 0 else 0.0)
        b = [inp(bx[..., k]) for k in range(4)]
        d = [xsub(b[k], tg[k]) for k in range(4)]
        l1 = [xmul(fabs(d[k]), w[k]) for k in range(4)]
        for col, ks in ((1, (0, 1, 2, 3)), (2, (0, 1)), (3, (2, 3))):
            v = np.stack([l1[k][0] for k in ks], -1)
            e = np.stack([l1[k][1] for k in ks], -1)
            sv[:, col], se[:, col] = _sum(v, e, (1, 2, 3))
        wsum32, wm32, anyw = _fp32_counts(w)
        wm = xdiv(xadd(xadd(w[0], w[1]), xadd(w[2], w[3])), const(4.0))
        wh = np.asarray(seg["wh"], F)
        fw, fh = _bc(inp(wh[None, :, None, 0]), (nl, B, Q)), _bc(inp(wh[None, :, None, 1]), (nl, B, Q))
        gl, grad_fn, sels = giou_elem(b, tg, fw, fh, F(P["iou_eps"]))
        on = wm32 != 0
        ge = xmul(gl, wm)
        ge = np.where(on, ge[0], 0.0), np.where(on, ge[1], 0.0)
        sv[:, 4], se[:, 4] = _sum(ge[0], ge[1], (1, 2))
        sv[:, 5] = pos.sum((1, 2))
        sv[:, 6] = (wsum32 > 0).sum((1, 2))
        sv[:, 7] = anyw.sum((1, 2))
        sv[:, 8], se[:, 8] = _sum(np.where(pos, w[0][0], 0.0), np.zeros((nl, B, Q)), (1, 2))
        if kind == WARMUP:
            sv[:, 9], se[:, 9] = _sum(lw[0], lw[1], (1, 2))
        # norm_inputs + finalize_one
        bg = float(F(P["bg_cls_weight"]))
        if kind == WARMUP:
            nin = [_cast((sv[:, 9], se[:, 9])), _cast((sv[:, 8], se[:, 8]))]
        elif kind == DN:
            nin = [_cast((sv[:, 5] + sv[:, 5] * bg, np.zeros(nl))), _cast((sv[:, 5], np.zeros(nl)))]
        else:
            nin = [_cast((sv[:, 5] + (B * Q - sv[:, 5]) * bg, np.zeros(nl))), _cast((sv[:, 6], np.zeros(nl)))]
        one = const(1.0)
        ncls, nreg = fmax(nin[0], one), fmax(nin[1], one)
        s_cls, s_l1 = xdiv(const(P["cls_weight"]), ncls), xdiv(const(P["l1_weight"]), nreg)
        s_iou = xdiv(const(P["iou_weight"]), nreg)
        s_iou = np.where(sv[:, 7] > 0, s_iou[0], 0.0), np.where(sv[:, 7] > 0, s_iou[1], 0.0)
        sc = [s_cls, s_l1, s_iou, s_l1, s_l1]
        sums = [(sv[:, k], se[:, k]) for k in (0, 1, 4, 2, 3)]
        terms = []
        for k in range(5):
            zero = (sc[k][0] == 0) & (sc[k][1] == 0)
            t = _cast(mul(sums[k], sc[k]))                        # a double product, then one cast
            terms.append((np.where(zero, 0.0, t[0]), np.where(zero, 0.0, t[1])))
        # backward
        co = [xmul(sc[k], inp(np.asarray(coef, F)[:, k])) for k in range(5)]
        c4 = lambda a: (a[0][:, None, None, None], a[1][:, None, None, None])  # noqa: E731
        c3 = lambda a: (a[0][:, None, None], a[1][:, None, None])  # noqa: E731
        gcls = xmul(cd, c4(co[0]))
        cxy, chw = xadd(c3(co[1]), c3(co[3])), xadd(c3(co[1]), c3(co[4]))
        sg = [_sign(d[k]) for k in range(4)]
        l1g = [xmul(xmul(w[k], sg[k]), cxy if k < 2 else chw) for k in range(4)]
        gon = on & (co[2][0] != 0)[:, None, None]
        cg = xmul(wm, c3(co[2]))

        def full(ms):
            gg = grad_fn(ms, cg)
            return [_sel(gon, xadd(l1g[k], gg[k]), l1g[k]) for k in range(4)]

        sels = [(m, o & gon) for m, o in sels]
        gb, used = _hull(full, sels)
        gbox = np.stack([g[0] for g in gb], -1), np.stack([g[1] for g in gb], -1)
        st = lambda ps: (np.stack([p[0] for p in ps], -1), np.stack([p[1] for p in ps], -1))  # noqa: E731
        return dict(stats=(sv, se), terms=st(terms), scales=st(sc), gcls=gcls, gbox=gbox,
                    hull_rows=int((used | np.any([s[1] > 0 for s in sg], 0)).sum()))


# ------------------------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------------------------
def _check(case, name, got, a, report, nonneg=False):
    got = _f(got)
    if got.shape != np.shape(a[0]):
        raise Inadmissible(f"{case}: {name}: shape {got.shape}, expected {np.shape(a[0])}")
    e = bound(a)
    none = ~np.isfinite(e)
    bad = none & ~np.isfinite(got)
    if nonneg:
        bad |= got < 0
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise Inadmissible(f"{case}: {name}{list(i)}: got {got[i]!r} where the statement (fp64 {a[0][i]!r}) has no bound: it must "
                           f"still be finite{' and not negative' if nonneg else ''}")
    try:
        _within(f"{case}: {name}", got, a)
    except Inadmissible:
        raise
    report[name] = dict(ratio=ratio(got, a), none=float(none.mean()) if none.size else 0.0)


def check_set_loss(problem, terms, stats, grads):
    """problem: dict(name, segs, coef (T,5) fp32).  terms (T,5), stats (T,10), grads: per segment (d cls, d boxes).
    -> {output: dict(ratio, none[, hull])}; raises Inadmissible naming the case, the output and the index."""
    rep = {}
    t0 = 0
    terms, stats = _f(terms), _f(stats)
    for i, seg in enumerate(problem["segs"]):
        nl = np.shape(seg["cls"])[0]
        ref = segment_statement(seg, np.asarray(problem["coef"], F)[t0:t0 + nl])
        tag = f"seg{i}({('matched', 'dn', 'warmup')[seg['kind']]})"
        _check(problem["name"], f"{tag}.stats", stats[t0:t0 + nl], ref["stats"], rep, nonneg=False)
        _check(problem["name"], f"{tag}.terms", terms[t0:t0 + nl], ref["terms"], rep, nonneg=seg["kind"] == WARMUP)
        _check(problem["name"], f"{tag}.gcls", grads[i][0], ref["gcls"], rep)
        _check(problem["name"], f"{tag}.gbox", grads[i][1], ref["gbox"], rep)
        rep[f"{tag}.gbox"]["hull"] = ref["hull_rows"]
        t0 += nl
    return rep


def tal_depth(total):
    """fp32 additions on the path of one element into tal_loss.hip's sum: the thread's grid-stride trips, six shuffle steps, two
    for the four waves, and the final cast (256 threads, four elements per thread and launch, at most 1024 workgroups)."""
    blocks = min((total + 1023) // 1024, 1024)
    return -(-total // (blocks * 256)) + 6 + 2 + 1


def tal_statement(logits, labels, metrics, gamma=2.0, input_is_prob=False):
    with np.errstate(all="ignore"):
        x = np.asarray(logits, F)
        N, C = x.shape
        onehot = np.asarray(labels, np.int64)[:, None] == np.arange(C)
        st = inp(np.where(onehot, np.asarray(metrics, F)[:, None], F(0)))
        v, g = tal_elem(inp(x), st, float(F(gamma)), input_is_prob)
        s = v[0].sum()
        se = bound(v).sum() + tal_depth(x.size) * 2 * U * np.abs(v[0]).sum() + TINY
        return (np.asarray(s), np.asarray(se)), g, v


def check_tal(logits, labels, metrics, gamma, input_is_prob, loss_sum, grad, name="tal"):
    rep = {}
    s, g, _ = tal_statement(logits, labels, metrics, gamma, input_is_prob)
    _check(name, "loss_sum", np.asarray(loss_sum, np.float64).reshape(()), s, rep, nonneg=True)
    if grad is not None:
        _check(name, "grad", grad, g, rep)
    return rep


def focal_statement(logits, labels, weights, alpha, gamma):
    with np.errstate(all="ignore"):
        x = np.asarray(logits, F)
        N, C = x.shape
        onehot = np.asarray(labels, np.int64)[:, None] == np.arange(C)
        v, dz = focal_elem(inp(x), onehot, alpha, float(F(gamma)))
        lw = inp(np.ones(N, F) if weights is None else np.asarray(weights, F))
        lw = (lw[0][:, None], lw[1][:, None])
        v, dz = xmul(v, lw), xmul(dz, lw)
        s = _sum(v[0], v[1], (0, 1), extra=4 * U if C % 4 == 0 else 0.0)
        return _cast((np.asarray(s[0]), np.asarray(s[1]))), dz


def check_focal(logits, labels, weights, alpha, gamma, loss_sum, grad, name="focal"):
    """FocalLoss(reduction='sum', loss_weight=1): the fp32 cast of statistic 0 and d / d logits under an upstream gradient of 1"""
    rep = {}
    s, g = focal_statement(logits, labels, weights, alpha, gamma)
    _check(name, "loss_sum", np.asarray(loss_sum, np.float64).reshape(()), s, rep)
    if grad is not None:
        _check(name, "grad", grad, g, rep)
    return rep


# ------------------------------------------------------------------------------------------------------------------
# an honest fp32 evaluation of the same formulas (a cast after every operation), and its mutants
# ------------------------------------------------------------------------------------------------------------------
def _half(p, mutant):
    return p.astype(np.float16).astype(F) if mutant == "half_precision_sigmoid" else p


def _focal32(x, t, alpha, gamma, mutant):
    one = F(1.0)
    al = F(alpha)
    a = np.where(t, one - al, al) if mutant == "alpha_swapped" else np.where(t, al, one - al)
    z = np.where(t, -x, x)
    ez = np.exp(-np.abs(z))
    big, small = one / (one + ez), ez / (one + ez)
    s, oms = _half(np.where(z >= 0, big, small), mutant), _half(np.where(z >= 0, small, big), mutant)
    sp = np.maximum(z, F(0.0)) + np.log1p(ez)
    sg = s * s if gamma == 2.0 else np.power(s, F(gamma))
    dz = a * sg * (F(gamma) * oms * sp + s)
    return a * sg * sp, np.where(t, -dz, dz)


def _tal32(x, st, gamma, input_is_prob, mutant):
    one = F(1.0)
    p = x if input_is_prob else _half(one / (one + np.exp(-x)), mutant)
    lp, l1p = np.log(p), np.log(one - p)
    if mutant != "no_log_clamp":
        lp, l1p = np.maximum(lp, F(-100.0)), np.maximum(l1p, F(-100.0))
    ce = -(st * lp + (one - st) * l1p)
    d = st - p
    ad = np.abs(d)
    mod = ad * ad if gamma == 2.0 else np.power(ad, F(gamma))
    if gamma == 2.0:
        dmod = F(-2.0) * d
    else:
        sgn = one if mutant == "pow_sign_dropped" else np.where(d > 0, one, -one)
        dmod = np.where(ad > 0, -F(gamma) * np.power(ad, F(gamma - 1.0)) * sgn, F(0.0))
    den = (one - p) * p
    if mutant != "no_bce_clamp":
        den = np.maximum(den, F(1e-12))
    dp = dmod * ce + mod * ((p - st) / den)
    return mod * ce, (dp if input_is_prob else dp * (p * (one - p)))


def _giou32(b, tg, fw, fh, eps, c, mutant):
    half, zero, one = F(0.5), F(0.0), F(1.0)
    f = (fw, fh, fw, fh)
    tie = one if mutant == "tie_full" else half
    dmax = lambda a, b_: np.where(a > b_, one, np.where(a == b_, tie, zero))  # noqa: E731
    dmin = lambda a, b_: np.where(a < b_, one, np.where(a == b_, tie, zero))  # noqa: E731
    gate = (lambda v: (v > 0).astype(F)) if mutant == "gate_gt" else (lambda v: (v >= 0).astype(F))

    def corners(q):
        return [(q[0] - half * q[2]) * f[0], (q[1] - half * q[3]) * f[1], (q[0] + half * q[2]) * f[2], (q[1] + half * q[3]) * f[3]]

    p, g = corners(b), corners(tg)
    a1, a2 = (p[2] - p[0]) * (p[3] - p[1]), (g[2] - g[0]) * (g[3] - g[1])
    lt = [np.maximum(p[k], g[k]) for k in range(2)]
    rb = [np.minimum(p[k + 2], g[k + 2]) for k in range(2)]
    wh = [np.maximum(rb[k] - lt[k], zero) for k in range(2)]
    elt = [np.minimum(p[k], g[k]) for k in range(2)]
    erb = [np.maximum(p[k + 2], g[k + 2]) for k in range(2)]
    ewh = [np.maximum(erb[k] - elt[k], zero) for k in range(2)]
    ov = wh[0] * wh[1]
    uraw = a1 + a2 - ov
    u = np.maximum(uraw, eps)
    eraw = ewh[0] * ewh[1]
    e = np.maximum(eraw, eps)
    loss = one - (ov / u - (e - u) / e)
    dU = ov / (u * u) - one / e
    if mutant != "no_union_clamp_grad":
        dU = dU * dmax(uraw, eps)
    dE = (u / (e * e)) * dmax(eraw, eps)
    dO = -one / u - dU
    hh, ww = p[3] - p[1], p[2] - p[0]
    dp = [zero - dU * hh, zero - dU * ww, zero + dU * hh, zero + dU * ww]
    for k in range(2):
        dwh = dO * wh[1 - k] * gate(rb[k] - lt[k])
        dp[k + 2] = dp[k + 2] + dwh * dmin(p[k + 2], g[k + 2])
        dp[k] = dp[k] - dwh * dmax(p[k], g[k])
        dewh = dE * ewh[1 - k] * gate(erb[k] - elt[k])
        dp[k + 2] = dp[k + 2] + dewh * dmax(p[k + 2], g[k + 2])
        dp[k] = dp[k] - dewh * dmin(p[k], g[k])
    dp = [dp[k] * (f[k] * c) for k in range(4)]
    return loss, [dp[0] + dp[2], dp[1] + dp[3], half * (dp[2] - dp[0]), half * (dp[3] - dp[1])]


def _segment32(seg, coef, mutant):
    P = seg["params"]
    kind = seg["kind"]
    x = np.asarray(seg["cls"], F)
    bx = np.asarray(seg["boxes"], F)
    nl, B, Q, C = x.shape
    labels, pos, lw, tg, w = _rows(seg)
    lw = lw[0].astype(F)
    w = [a[0].astype(F) for a in w]
    wh = np.asarray(seg["wh"], F)
    fw, fh = np.broadcast_to(wh[None, :, None, 0], (nl, B, Q)), np.broadcast_to(wh[None, :, None, 1], (nl, B, Q))
    if kind == DN:                                    # the targets with fp32 divisions, as load_row forms them
        gt = np.zeros((B, Q, 4), F)
        for b in range(B):
            g = np.asarray(seg["gts"][b], F).reshape(-1, 4)
            j = np.arange(Q) % seg["single_pad"]
            gt[b, pos[0, b]] = g[j[pos[0, b]]]
        x1, y1, x2, y2 = gt[..., 0] / wh[:, 0:1], gt[..., 1] / wh[:, 1:2], gt[..., 2] / wh[:, 0:1], gt[..., 3] / wh[:, 1:2]
        t = [(x1 + x2) / F(2), (y1 + y2) / F(2), x2 - x1, y2 - y1]
        tg = [np.broadcast_to(np.where(pos[0], a, F(0)), (nl, B, Q)) for a in t]
    else:
        tg = [a[0].astype(F) for a in tg]
    onehot = labels[..., None] == np.arange(C)
    gamma = float(F(P["gamma"]))
    if kind == WARMUP:
        cv, cd = _tal32(x, np.where(onehot, lw[..., None], F(0)), gamma, False, mutant)
    else:
        cv, dz = _focal32(x, onehot, P["alpha"], gamma, mutant)
        cv, cd = cv * lw[..., None], dz * lw[..., None]
    st = np.zeros((nl, 10))
    st[:, 0] = cv.astype(np.float64).sum((1, 2, 3))
    b = [bx[..., k] for k in range(4)]
    d = [b[k] - tg[k] for k in range(4)]
    l1 = np.stack([np.abs(d[k]) * w[k] for k in range(4)], -1).astype(np.float64)
    st[:, 1], st[:, 2], st[:, 3] = l1.sum((1, 2, 3)), l1[..., :2].sum((1, 2, 3)), l1[..., 2:].sum((1, 2, 3))
    wsum = (w[0] + w[1]) + (w[2] + w[3])
    wm = wsum / F(4.0)
    eps = F(P["iou_eps"])
    gl, _ = _giou32(b, tg, fw, fh, eps, F(0.0), mutant)
    st[:, 4] = np.where(wm != 0, gl * wm, F(0)).astype(np.float64).sum((1, 2))
    st[:, 5] = pos.sum((1, 2))
    st[:, 6] = (wsum > 0).sum((1, 2))
    st[:, 7] = st[:, 6] if mutant == "any_w_as_sum_w" else ((w[0] > 0) | (w[1] > 0) | (w[2] > 0) | (w[3] > 0)).sum((1, 2))
    st[:, 8] = np.where(pos, w[0], F(0)).astype(np.float64).sum((1, 2))
    st[:, 9] = lw.astype(np.float64).sum((1, 2)) if kind == WARMUP else 0.0
    bg = float(F(P["bg_cls_weight"]))
    if kind == WARMUP:
        nin = (st[:, 9].astype(F), st[:, 8].astype(F))
    elif kind == DN:
        nin = ((st[:, 5] + st[:, 5] * bg).astype(F), st[:, 5].astype(F))
    else:
        nin = ((st[:, 5] + (B * Q - st[:, 5]) * bg).astype(F), st[:, 6].astype(F))
    ncls, nreg = np.maximum(nin[0], F(1)), np.maximum(nin[1], F(1))
    s_l1 = F(P["l1_weight"]) / nreg
    sc = np.stack([F(P["cls_weight"]) / ncls, s_l1, np.where(st[:, 7] > 0, F(P["iou_weight"]) / nreg, F(0)), s_l1, s_l1], -1).astype(F)
    sums = np.stack([st[:, 0], st[:, 1], st[:, 4], st[:, 2], st[:, 3]], -1)
    terms = np.where(sc == 0, F(0), (sums * sc.astype(np.float64)).astype(F)).astype(F)
    co = sc * np.asarray(coef, F)
    gcls = cd * co[:, 0, None, None, None]
    sgn = [np.where((d[k] == 0) & (mutant == "l1_sign0_as_1"), F(1), np.sign(d[k])).astype(F) for k in range(4)]
    g = [w[k] * sgn[k] * (co[:, 1, None, None] + co[:, 3 if k < 2 else 4, None, None]) for k in range(4)]
    _, gg = _giou32(b, tg, fw, fh, eps, wm * co[:, 2, None, None], mutant)
    gon = (wm != 0) & (co[:, 2, None, None] != 0)
    gbox = np.stack([np.where(gon, g[k] + gg[k], g[k]) for k in range(4)], -1).astype(F)
    return terms, st, gcls.astype(F), gbox


def eval_f32(what, *args, mutant=None):
    """what = 'set_loss': (problem) -> terms (T,5), stats (T,10), grads [(d cls, d boxes) per segment];
    'tal': (logits, labels, metrics, gamma, input_is_prob) -> loss_sum, grad;  'focal': (logits, labels, weights, alpha, gamma)
    -> loss_sum, grad.  fp32 numpy, a cast after every operation; sums in fp64 then one cast."""
    assert mutant is None or mutant in MUTANTS, mutant
    with np.errstate(all="ignore"):
        if what == "set_loss":
            (problem,) = args
            terms, stats, grads, t0 = [], [], [], 0
            for seg in problem["segs"]:
                nl = np.shape(seg["cls"])[0]
                t, s, gc, gb = _segment32(seg, np.asarray(problem["coef"], F)[t0:t0 + nl], mutant)
                terms.append(t); stats.append(s); grads.append((gc, gb))
                t0 += nl
            return np.concatenate(terms), np.concatenate(stats), grads
        if what == "tal":
            logits, labels, metrics, gamma, input_is_prob = args
            x = np.asarray(logits, F)
            onehot = np.asarray(labels, np.int64)[:, None] == np.arange(x.shape[1])
            v, g = _tal32(x, np.where(onehot, np.asarray(metrics, F)[:, None], F(0)), float(F(gamma)), input_is_prob, mutant)
            return F(v.astype(np.float64).sum()), g.astype(F)
        if what == "focal":
            logits, labels, weights, alpha, gamma = args
            x = np.asarray(logits, F)
            onehot = np.asarray(labels, np.int64)[:, None] == np.arange(x.shape[1])
            v, dz = _focal32(x, onehot, alpha, float(F(gamma)), mutant)
            lw = np.ones(len(x), F) if weights is None else np.asarray(weights, F)
            return F((v * lw[:, None]).astype(np.float64).sum()), (dz * lw[:, None]).astype(F)
    raise ValueError(what)


def table(case, rep):
    """one printed line per case: worst err / bound, elements using a hull, share without statement, per output"""
    cells = []
    for k, v in rep.items():
        cells.append(f"{k}={v['ratio']:.3g}" + (f"/hull{v['hull']}" if "hull" in v else "") + (f"/none{v['none']:.2%}" if v["none"] else ""))
    return f"  {case:34s} " + " ".join(cells)

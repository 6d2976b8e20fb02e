"""Plain float64 statements of the kernels that end in a DECISION -- Hungarian match cost + assignment, the one-to-many
assigner and its targets, the teacher's score threshold / class-aware NMS / top max_per_img, the mean + std pseudo-label filter
and the weak->strong box warp -- each with a running fp32 error bound, and the checkers that decide whether a result (from the
GPU or from the C oracle) is ADMISSIBLE against them.

Test helper (not a conftest; imported by name like msda_ref64.py).  Numpy only: no call into oracle/ or the library.  Written
from the reference's Python:
  FocalLossCost / BBoxL1Cost / IoUCost   mmdet/core/bbox/match_costs/match_cost.py:33-50, :83-99, :169-185
  bbox_overlaps                          mmdet/core/bbox/iou_calculators/iou2d_calculator.py:200-261
  bbox_cxcywh_to_xyxy / xyxy_to_cxcywh   mmdet/core/bbox/transforms.py:222-247
  HungarianAssigner.assign               mmdet/core/bbox/assigners/hungarian_assigner.py:115-147
  O2MAssigner.assign                     detr_od/core/bbox/assigners/o2m_assigner.py:50-170
  warm-up targets                        detr_od/models/dense_heads/dino_detr_ssod_head.py:1108-1165
  _get_bboxes_single(for_pseudo_label)   detr_od/models/dense_heads/dino_detr_ssod_head.py:1364-1395
  multiclass_nms                         mmdet/core/post_processing/bbox_nms.py:8-95 (over mmcv batched_nms / nms)
  mean + std filter                      detr_ssod/models/dino_detr_ssod.py:918-939
  Transform2D.transform_bboxes           detr_ssod/models/utils/bbox_utils.py:167-192, :18-41

Error model (the convention of msda_ref64.py).  u = 2^-24.  Every fp32 operation is allowed ONE ulp, 2u|result|, rather than
half an ulp; expf / logf / powf / sqrtf likewise on top of their propagated input error.  The ROCm installation documents no ulp
table for OCML's expf / logf / powf, so the 1-ulp-as-2u convention stands for them as well.  A value is carried through the
expression tree as a pair (value, err) with running error

    err_out = sum_i |df/dx_i| err_i + 2u |f| + 2^-126

where the propagated part is first order for + - and carries the exact remainder for the operations whose input error need not
be small here: a b keeps err_a err_b, a / b is (err_a + |a / b| err_b) / (|b| - err_b), log t is -log(1 - err_t / t), exp and
x ** g use the interval's far end; a divisor or a log argument whose interval reaches zero gives no statement (inf).  The
first-order forms alone are too tight for honest fp32: at a logit of 17, 1 - p is 4e-8 in fp64 and 0 in fp32, and
-log(1 - p + eps) differs by 10.6 where err / t would allow 8.7.  (2^-126: one flushed subnormal; dropped where the result is
an exact zero of exact operands.)  fmax / fmin / clamp take the larger incoming error where the operands' intervals meet; where
one lies wholly beyond the other the result is that operand with its own error, so max(x, 0) of a surely negative x is an exact
0, and a product with an exact 0 is an exact 0.  The overlap of two surely disjoint boxes, their IoU and the O2M metric are
therefore (0, 0), and the static modes' `metric > 0` filter is a decision without allowance for every such pair; abs keeps the
error.  Inputs are the fp32 arrays themselves
(error 0) and the parameters are the fp32 values the C ABI carries (eps = fp32(1e-12), ...).  x ** n for integral n may be formed
by repeated multiplication (up to n - 1 roundings) or by powf (one): the bound allows n roundings.  sqrt near zero uses
min(e / (2 sqrt v), sqrt e).  A bound that is not finite (0 * inf, division by an exact zero) means "no statement": the element
is admissible whatever it holds and every decision that rests on it may go either way.  Nothing is scaled per test.

The expressions are short but ill-conditioned in places, which is why the error is carried and not a closed formula:
-log(1 - p + eps) near p = 1 has err(1 - p) / eps, about 2e5 for a logit above 17, and overlap / max(union, 1e-6) of a degenerate
box divides a pixel-rounding error by 1e-6.  On such inputs the continuous bound says nothing and the structural conditions,
which carry no allowance, are what is checked.

NMS compares boxes in the frame the reference builds, boxes + label * (boxes.max() + 1): the statement is the IoU of the plain
boxes, and each coordinate's error includes the rounding of that addition, 2u |x + offset| (the error of the offset itself is
common to the whole class and cancels in every difference).

Conventions where the reference leaves the result open; the checkers accept every order it could produce:
  * torch.topk among equal metrics (o2m_assigner.py:121): any of the tied queries may bid;
  * the gt of a query that bids for several gts of equal IoU (max over dim 0): any of them;
  * the (unstable) sorts by score in multiclass_nms / batched_nms: equal scores in any order, so any of a set of duplicated
    detections may be the one that survives;
  * O2M with fewer queries than candidate_topk raises torch.topk's error in the reference and here; it is not a case.
  * The gt of a positive query: the issue words the condition against the largest IoU among the gts the query is a POSSIBLE
    bidder of; a query that in fact lost a close top-k race for that gt is rightly given a smaller-IoU gt, so the lower bar is
    taken over the gts it is a CERTAIN bidder of (the two sets coincide wherever no race is within its allowance).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
O2M_INF = 100000000.0


class Inadmissible(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------
# (value, err) arithmetic
# ------------------------------------------------------------------------------------------------------------------
def _f(x):
    return np.asarray(x, np.float64)


def inp(x):
    """An fp32 input: exact."""
    x = _f(np.asarray(x, np.float32))
    return x, np.zeros_like(x)


def _r(v, e, n=1):
    exact0 = (v == 0) & (e == 0)
    return v, e + n * 2 * U * np.abs(v) + np.where(exact0, 0.0, TINY)


def add(a, b):
    return _r(a[0] + b[0], a[1] + b[1])


def sub(a, b):
    return _r(a[0] - b[0], a[1] + b[1])


def mul(a, b):
    zero = ((a[0] == 0) & (a[1] == 0)) | ((b[0] == 0) & (b[1] == 0))          # an exact zero times anything finite is an exact zero
    return _r(a[0] * b[0], np.where(zero, 0.0, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1]))


def div(a, b):
    v = a[0] / b[0]
    room = np.abs(b[0]) - b[1]                      # the divisor's interval must stay clear of zero
    return _r(v, np.where(room > 0, (a[1] + np.abs(v) * b[1]) / room, np.inf))


def neg(a):
    return -a[0], a[1]


def fabs(a):
    return np.abs(a[0]), a[1]


def _pick(a, b, sign):
    """max (sign = 1) or min (sign = -1): where one operand's interval lies wholly beyond the other's, the result IS that
    operand, value and error (so max(x, 0) of a surely negative x is an exact 0); where they meet, the larger error."""
    av, ae, bv, be = np.broadcast_arrays(a[0], a[1], b[0], b[1])
    a_wins = sign * (av - bv) > ae + be
    b_wins = sign * (bv - av) > ae + be
    v = np.maximum(av, bv) if sign > 0 else np.minimum(av, bv)
    return v, np.where(a_wins, ae, np.where(b_wins, be, np.maximum(ae, be)))


def fmax(a, b):
    return _pick(a, b, 1)


def fmin(a, b):
    return _pick(a, b, -1)


def exp_(a):
    v = np.exp(a[0])
    return _r(v, v * np.expm1(a[1]))


def log_(a):
    r = a[1] / np.abs(a[0])
    return _r(np.log(a[0]), np.where(r < 1, -np.log1p(-np.minimum(r, 0.5 + 0.5 * r)), np.inf))


def log1p_(a):
    """log1pf: log_ of 1 + t without the rounding of the sum (the loss kernels' softplus; tests/loss_ref64.py)."""
    r = a[1] / np.abs(1.0 + a[0])
    return _r(np.log1p(a[0]), np.where(r < 1, -np.log1p(-np.minimum(r, 0.5 + 0.5 * r)), np.inf))


def pow_(a, g):
    g = float(g)
    v = np.power(a[0], g)
    if g >= 1:
        d = np.where(a[1] == 0, 0.0, np.power(np.abs(a[0]) + a[1], g) - np.power(np.abs(a[0]), g))
    else:
        d = np.where(a[1] == 0, 0.0, g * np.power(a[0], g - 1.0) * a[1])
    n = max(int(g), 1) if g == int(g) and g >= 1 else 1
    return _r(v, np.abs(d), n)


def sqrt_(a):
    v = np.sqrt(a[0])
    return _r(v, np.minimum(a[1] / (2 * v), np.sqrt(a[1])))


def const(c):
    return inp(np.float32(c))


def bound(a):
    """The error of a pair as a usable allowance: not finite -> inf."""
    return np.where(np.isfinite(a[1]), a[1], np.inf)


def ratio(got, a):
    """max |got - value| / err over the elements with a finite, positive bound (the figure the GPU table prints)."""
    got = _f(got)
    e = bound(a)
    ok = np.isfinite(e) & (e > 0)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got - a[0])[ok] / e[ok]))


def _within(name, got, a, where=None):
    """Raise unless |got - value| <= err elementwise (NaN in got or value fails unless the bound is infinite)."""
    got = _f(got)
    e = bound(a)
    bad = (~(np.abs(got - a[0]) <= e) & np.isfinite(e)) | (~np.isfinite(a[0]) & np.isfinite(got))     # a statement that is not finite where the result is

    if where is not None:
        bad &= where
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise Inadmissible(f"{name}{list(i)}: got {got[i]!r}, fp64 {a[0][i]!r}, |diff| {abs(got[i] - a[0][i]):.3e} > "
                           f"allowance {e[i]:.3e}")


# ------------------------------------------------------------------------------------------------------------------
# shared geometry
# ------------------------------------------------------------------------------------------------------------------
def _col(p, k):
    return p[0][..., k], p[1][..., k]


def _iou(b1, b2, mode="iou", mutant=None):
    """b1, b2: four (value, err) coordinates each, already broadcast against each other.  bbox_overlaps, eps 1e-6."""
    area1 = mul(sub(b1[2], b1[0]), sub(b1[3], b1[1]))
    area2 = mul(sub(b2[2], b2[0]), sub(b2[3], b2[1]))
    zero = const(0.0)
    ow = fmax(sub(fmin(b1[2], b2[2]), fmax(b1[0], b2[0])), zero)
    oh = fmax(sub(fmin(b1[3], b2[3]), fmax(b1[1], b2[1])), zero)
    overlap = mul(ow, oh)
    uni = fmax(sub(add(area1, area2), overlap), const(1e-6))
    iou = div(overlap, uni)
    none = (overlap[0] == 0) & (overlap[1] == 0)      # surely disjoint: 0 / max(union, 1e-6) is an exact 0 in any precision
    iou = np.where(none, 0.0, iou[0]), np.where(none, 0.0, iou[1])
    if mode == "giou" and mutant != "iou_not_giou":
        ew = sub(fmax(b1[2], b2[2]), fmin(b1[0], b2[0]))
        eh = sub(fmax(b1[3], b2[3]), fmin(b1[1], b2[1]))
        earea = mul(fmax(ew, zero), fmax(eh, zero))
        if mutant != "earea_noclamp":
            earea = fmax(earea, const(1e-6))
        iou = sub(iou, div(sub(earea, uni), earea))
    return iou


def _decode(bp, img_w, img_h, clip=False):
    """normalised cxcywh (..., 4) fp32 -> four pixel coordinates (value, err)."""
    b = inp(bp)
    cx, cy, w, h = (_col(b, k) for k in range(4))
    half = const(0.5)
    W, H = inp(img_w), inp(img_h)
    out = [mul(sub(cx, mul(half, w)), W), mul(sub(cy, mul(half, h)), H), mul(add(cx, mul(half, w)), W),
           mul(add(cy, mul(half, h)), H)]
    if clip:
        zero = const(0.0)
        out = [fmin(fmax(c, zero), lim) for c, lim in zip(out, (W, H, W, H))]
    return out


# ------------------------------------------------------------------------------------------------------------------
# Hungarian: cost and assignment
# ------------------------------------------------------------------------------------------------------------------
def match_cost(bbox_pred, cls_pred, gt_bboxes, gt_labels, img_w, img_h, w_cls=2.0, alpha=0.25, gamma=2.0, eps=1e-12,
               w_reg=5.0, box_format="xywh", w_iou=2.0, iou_mode="giou", pred_xyxy=False, mutant=None):
    """-> dict(cost, cls, reg, iou) of (value, err) pairs, each (Q, G).  pred_xyxy: bbox_pred holds x1, y1, x2, y2 directly
    (the contract of the cost classes called on their own; img_w = img_h = 1 then)."""
    with np.errstate(all="ignore"):
        gt_bboxes = np.asarray(gt_bboxes, np.float32).reshape(-1, 4)
        gl = np.asarray(gt_labels, np.int64)
        one, zero = const(1.0), const(0.0)
        W, H = inp(img_w), inp(img_h)
        # FocalLossCost
        x = inp(np.asarray(cls_pred, np.float32)[:, gl])                       # (Q, G)
        p = div(one, add(one, exp_(neg(x))))
        e_ = const(0.0 if mutant == "no_eps" else eps)
        a_, na_ = const(alpha), sub(one, const(alpha))
        if mutant == "alpha_swapped":
            a_, na_ = na_, a_
        q1 = sub(one, p)
        negc = mul(mul(neg(log_(add(q1, e_))), na_), pow_(p, gamma))
        posc = mul(mul(neg(log_(add(p, e_))), a_), pow_(q1, gamma))
        c_cls = mul(sub(posc, negc), const(w_cls))
        # boxes
        b = inp(np.asarray(bbox_pred, np.float32)[:, None, :])                 # (Q, 1, 4)
        two, half = const(2.0), const(0.5)
        if pred_xyxy:
            n = [_col(b, k) for k in range(4)]
            cx, cy = div(add(n[0], n[2]), two), div(add(n[1], n[3]), two)
            bw, bh = sub(n[2], n[0]), sub(n[3], n[1])
        else:
            cx, cy, bw, bh = (_col(b, k) for k in range(4))
            n = [sub(cx, mul(half, bw)), sub(cy, mul(half, bh)), add(cx, mul(half, bw)), add(cy, mul(half, bh))]
        g = inp(gt_bboxes[None, :, :])                                          # (1, G, 4)
        gc = [_col(g, k) for k in range(4)]
        fac = (W, H, W, H)
        ng = gc if mutant == "l1_unnormalised" else [div(gc[k], fac[k]) for k in range(4)]
        # BBoxL1Cost
        if box_format == "xywh":
            t = [div(add(ng[0], ng[2]), two), div(add(ng[1], ng[3]), two), sub(ng[2], ng[0]), sub(ng[3], ng[1])]
            d = [fabs(sub(s, tt)) for s, tt in zip((cx, cy, bw, bh), t)]
        else:
            d = [fabs(sub(n[k], ng[k])) for k in range(4)]
        c_reg = mul(add(add(add(d[0], d[1]), d[2]), d[3]), const(w_reg))
        # IoUCost
        b1 = [mul(n[k], fac[k]) for k in range(4)]
        c_iou = mul(neg(_iou(b1, gc, iou_mode, mutant)), const(w_iou))
        full = np.broadcast_to
        shape = (np.shape(bbox_pred)[0], gt_bboxes.shape[0])
        parts = dict(cls=c_cls, reg=c_reg, iou=c_iou, cost=add(add(c_cls, c_reg), c_iou))
        return {k: (full(v[0], shape).copy(), full(v[1], shape).copy()) for k, v in parts.items()}


def _scipy_lsa(c):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(c)


def check_hungarian(inputs, gt_inds, labels, cost=None, num_pos=None, ref=None, **kw):
    """inputs: dict(bbox_pred, cls_pred, gt_bboxes, gt_labels, img_w, img_h).  gt_inds / labels (Q,) as AssignResult holds
    them (0 / -1 for unmatched, gt index + 1 / gt label for matched); cost (Q, G) or None.  Returns statistics."""
    Q, G = len(inputs["bbox_pred"]), len(inputs["gt_labels"])
    gi, lab = np.asarray(gt_inds), np.asarray(labels)
    gl = np.asarray(inputs["gt_labels"], np.int64)
    stats = dict(cost_ratio=0.0, regret=0.0, regret_allowance=0.0, used_allowance=0)
    if gi.shape != (Q,) or lab.shape != (Q,):
        raise Inadmissible(f"hungarian: gt_inds / labels shapes {gi.shape} / {lab.shape}, expected ({Q},)")
    # (b) structure, exact
    if G == 0 or Q == 0:
        if not (np.all(gi == 0) and np.all(lab == -1)):
            raise Inadmissible("hungarian: no gts, yet some query is not background")
        return stats
    pos = np.nonzero(gi > 0)[0]
    if np.any((gi < 0) | (gi > G)):
        raise Inadmissible(f"hungarian: gt_inds outside [0, {G}] at {int(np.nonzero((gi < 0) | (gi > G))[0][0])}")
    if len(pos) != min(Q, G) or (num_pos is not None and int(num_pos) != min(Q, G)):
        raise Inadmissible(f"hungarian: {len(pos)} positives (num_pos {num_pos}), expected min(Q, G) = {min(Q, G)}")
    cols = gi[pos] - 1
    if len(np.unique(cols)) != len(cols):
        c = int(np.nonzero(np.bincount(cols) > 1)[0][0])
        raise Inadmissible(f"hungarian: gt {c} is given to queries {pos[cols == c].tolist()}: not a matching")
    want = np.full(Q, -1, np.int64)
    want[pos] = gl[cols]
    if not np.array_equal(lab, want):
        q = int(np.nonzero(lab != want)[0][0])
        raise Inadmissible(f"hungarian query {q}: label {int(lab[q])}, expected {int(want[q])} (gt_inds {int(gi[q])}; -1 on background)")
    if ref is None:
        ref = match_cost(**inputs, **kw)
    c64, E = ref["cost"][0], bound(ref["cost"])
    # (a) cost within bound
    if cost is not None:
        _within("hungarian cost", cost, ref["cost"])
        stats["cost_ratio"] = ratio(cost, ref["cost"])
    # (c) regret against scipy on the fp64 matrix
    if np.all(np.isfinite(c64)):
        r, c = _scipy_lsa(c64)
        regret = c64[pos, cols].sum() - c64[r, c].sum()
        allow = E[pos, cols].sum() + E[r, c].sum()
        stats.update(regret=float(regret), regret_allowance=float(allow), used_allowance=int(regret > 0))
        if not regret <= allow:
            worst = int(np.argmax(c64[pos, cols] - c64[r, c][np.argsort(c)][np.argsort(np.argsort(cols))]
                                  if len(cols) == len(c) and np.array_equal(np.sort(cols), np.sort(c)) else 0))
            raise Inadmissible(f"hungarian regret: returned assignment costs {c64[pos, cols].sum()!r} in fp64, optimum "
                               f"{c64[r, c].sum()!r}; margin {regret:.3e} > allowance {allow:.3e} (e.g. query {int(pos[worst])} "
                               f"-> gt {int(cols[worst])}, fp64 cost {c64[pos[worst], cols[worst]]!r})")
    return stats


def hungarian_ambiguity(inputs, **kw):
    """From inputs alone: (sum of E over the fp64 optimum, gap to the best assignment that differs from it)."""
    ref = match_cost(**inputs, **kw)
    c64, E = ref["cost"][0], bound(ref["cost"])
    r, c = _scipy_lsa(c64)
    best = c64[r, c].sum()
    second = np.inf
    for i, j in zip(r, c):
        m = c64.copy()
        m[i, j] = 1e30
        r2, c2 = _scipy_lsa(m)
        second = min(second, m[r2, c2].sum())
    return float(E[r, c].sum()), float(second - best)


# ------------------------------------------------------------------------------------------------------------------
# one-to-many assigner
# ------------------------------------------------------------------------------------------------------------------
def o2m(bbox_pred, cls_prob, gt_bboxes, gt_labels, img_w, img_h, alpha=1.0, beta=6.0, mutant=None):
    """-> dict(iou, met) of (value, err) pairs (Q, G)."""
    with np.errstate(all="ignore"):
        gt_bboxes = np.asarray(gt_bboxes, np.float32).reshape(-1, 4)
        gl = np.asarray(gt_labels, np.int64)
        b1 = _decode(np.asarray(bbox_pred, np.float32)[:, None, :], img_w, img_h)
        g = inp(gt_bboxes[None, :, :])
        iou = _iou(b1, [_col(g, k) for k in range(4)], "iou")
        s = inp(np.asarray(cls_prob, np.float32)[:, gl])
        if mutant == "exponents_swapped":
            alpha, beta = beta, alpha
        met = mul(pow_(s, alpha), pow_(iou, beta))
        shape = (np.shape(bbox_pred)[0], gt_bboxes.shape[0])
        return {k: (np.broadcast_to(v[0], shape).copy(), np.broadcast_to(v[1], shape).copy())
                for k, v in dict(iou=iou, met=met).items()}


def _clamp_int(s, k):
    s = np.where(np.isnan(s), 0.0, s)
    return np.clip(np.trunc(np.clip(s, -1.0, k + 1.0)), 1, k).astype(np.int64)


def o2m_decisions(inputs, topk=13, dynamic_k=False, alpha=1.0, beta=6.0, mutant=None, ref=None):
    """Bidders from fp64 with margins: dict(iou, met, certain (Q,G) bool, possible (Q,G) bool, k_lo, k_hi (G,))."""
    ref = ref or o2m(**inputs, alpha=alpha, beta=beta, mutant=mutant)
    m, e = ref["met"][0], bound(ref["met"])
    iou, ei = ref["iou"][0], bound(ref["iou"])
    Q, G = m.shape
    k = min(int(topk), Q)
    if mutant == "topk_plus":
        k = min(k + 1, Q)
    if mutant == "topk_minus":
        k = max(k - 1, 0)
    k_lo = k_hi = np.full(G, k, np.int64)
    if dynamic_k:
        with np.errstate(all="ignore"):
            lo_s = -np.sort(-(iou - ei), 0)[:k].sum(0)
            hi_s = -np.sort(-(iou + ei), 0)[:k].sum(0)
            lo_s, hi_s = lo_s - 2 * U * k * np.abs(lo_s), hi_s + 2 * U * k * np.abs(hi_s)
        if mutant == "dynamic_k_rounded":
            lo_s, hi_s = lo_s + 0.5, hi_s + 0.5
        k_lo, k_hi = _clamp_int(lo_s, k), _clamp_int(np.where(np.isfinite(hi_s), hi_s, k + 1.0), k)
    lo, hi = m - e, m + e
    hs, ls = np.sort(hi, 0), np.sort(lo, 0)
    n_ge, n_gt = np.empty((Q, G), np.int64), np.empty((Q, G), np.int64)
    for g in range(G):
        n_ge[:, g] = Q - np.searchsorted(hs[:, g], lo[:, g], "left") - 1       # others that may be at or above me
        n_gt[:, g] = Q - np.searchsorted(ls[:, g], hi[:, g], "right")          # others surely above me
    certain, possible = n_ge < k_lo[None, :], n_gt < k_hi[None, :]
    if not dynamic_k and mutant != "metric_filter_dropped":
        certain &= lo > 0
        possible &= hi > 0
    return dict(iou=ref["iou"], met=ref["met"], certain=certain, possible=possible, k_lo=k_lo, k_hi=k_hi)


def o2m_targets(inputs, gt_inds, num_classes, ref):
    """Targets given a returned assignment -> labels_full (exact), bbox_targets and norm_metrics as (value, err)."""
    with np.errstate(all="ignore"):
        gi = np.asarray(gt_inds)
        Q = len(gi)
        gl = np.asarray(inputs["gt_labels"], np.int64)
        gt = np.asarray(inputs["gt_bboxes"], np.float32).reshape(-1, 4)
        pos = np.nonzero(gi > 0)[0]
        g = gi[pos] - 1
        lf = np.full(Q, num_classes, np.int64)
        lf[pos] = gl[g]
        bt = [np.zeros(Q), np.zeros(Q)]
        bt = (np.zeros((Q, 4)), np.zeros((Q, 4)))
        nm = (np.zeros(Q), np.zeros(Q))
        if len(pos):
            b = inp(gt[g])
            W, H, two = inp(inputs["img_w"]), inp(inputs["img_h"]), const(2.0)
            n = [div(_col(b, 0), W), div(_col(b, 1), H), div(_col(b, 2), W), div(_col(b, 3), H)]
            t = [div(add(n[0], n[2]), two), div(add(n[1], n[3]), two), sub(n[2], n[0]), sub(n[3], n[1])]
            for k in range(4):
                bt[0][pos, k], bt[1][pos, k] = t[k]
            m, e = ref["met"][0][pos, g], bound(ref["met"])[pos, g]
            i, ei = ref["iou"][0][pos, g], bound(ref["iou"])[pos, g]
            G = len(gl)
            mm, me, mi, mie = np.zeros(G), np.zeros(G), np.zeros(G), np.zeros(G)
            np.maximum.at(mm, g, m); np.maximum.at(me, g, e); np.maximum.at(mi, g, i); np.maximum.at(mie, g, ei)
            v = mul(div((m, e), add((mm[g], me[g]), const(10e-8))), (mi[g], mie[g]))
            nm[0][pos], nm[1][pos] = v
        return lf, bt, nm


def check_o2m(inputs, res, num_classes, topk=13, dynamic_k=False, alpha=1.0, beta=6.0, mutant=None, dec=None):
    """res: dict(gt_inds, labels, max_overlaps, assign_metrics[, labels_full, bbox_targets, norm_metrics]) of one problem."""
    gi, lab = np.asarray(res["gt_inds"]), np.asarray(res["labels"])
    mo, am = _f(res["max_overlaps"]), _f(res["assign_metrics"])
    Q, G = len(inputs["bbox_pred"]), len(inputs["gt_labels"])
    gl = np.asarray(inputs["gt_labels"], np.int64)
    stats = dict(iou_ratio=0.0, met_ratio=0.0, bt_ratio=0.0, nm_ratio=0.0, used_allowance=0)
    if any(np.shape(a) != (Q,) for a in (gi, lab, mo, am)):
        raise Inadmissible(f"o2m: output shapes {[np.shape(a) for a in (gi, lab, mo, am)]}, expected ({Q},) each")
    if G == 0 or Q == 0:
        if not (np.all(gi == 0) and np.all(lab == -1) and np.all(mo == 0) and np.all(am == 0)):
            raise Inadmissible("o2m: no gts, yet an output is not the background value")
        if "labels_full" in res and not (np.all(np.asarray(res["labels_full"]) == num_classes)
                                         and not np.any(_f(res["bbox_targets"])) and not np.any(_f(res["norm_metrics"]))):
            raise Inadmissible("o2m: no gts, yet a target is not the background value")
        return stats
    if np.any((gi < 0) | (gi > G)):
        raise Inadmissible(f"o2m: gt_inds outside [0, {G}]")
    dec = dec or o2m_decisions(inputs, topk, dynamic_k, alpha, beta, mutant)
    certain, possible = dec["certain"], dec["possible"]
    iou, ei = dec["iou"][0], bound(dec["iou"])
    pos = np.nonzero(gi > 0)[0]
    g = gi[pos] - 1
    bad = ~possible[pos, g]
    if bad.any():
        q, gg = int(pos[bad][0]), int(g[bad][0])
        m, e = dec["met"][0][:, gg], bound(dec["met"])[:, gg]
        above = int(((m - e) > m[q] + e[q]).sum())
        raise Inadmissible(f"o2m query {q}: positive for gt {gg}, where it cannot be among the top {int(dec['k_hi'][gg])}: metric "
                           f"{m[q]!r} +- {e[q]:.3e}, {above} queries surely above it")
    must = certain.any(1)
    bad = must & (gi == 0)
    if bad.any():
        q = int(np.nonzero(bad)[0][0])
        gg = int(np.nonzero(certain[q])[0][0])
        raise Inadmissible(f"o2m query {q}: background, yet certainly among the top {int(dec['k_lo'][gg])} of gt {gg} (metric "
                           f"{dec['met'][0][q, gg]!r} +- {bound(dec['met'])[q, gg]:.3e})")
    with np.errstate(invalid="ignore"):
        bar = np.where(certain[pos], (iou - ei)[pos], -np.inf).max(1)
    have = iou[pos, g] + ei[pos, g]
    bad = ~(have >= bar)
    if bad.any():
        q, gg = int(pos[bad][0]), int(g[bad][0])
        best = int(np.argmax(np.where(certain[q], iou[q] - ei[q], -np.inf)))
        raise Inadmissible(f"o2m query {q}: given gt {gg} (IoU {iou[q, gg]!r} +- {ei[q, gg]:.3e}) although it certainly bids for gt "
                           f"{best} with IoU {iou[q, best]!r} +- {ei[q, best]:.3e}; margin {bar[bad][0] - have[bad][0]:.3e}")
    stats["used_allowance"] = int((~certain[pos, g]).sum() + (iou[pos, g] < np.where(certain[pos], iou[pos], -np.inf).max(1)).sum())
    if not np.array_equal(lab[pos], gl[g]):
        i = int(np.nonzero(lab[pos] != gl[g])[0][0])
        raise Inadmissible(f"o2m query {int(pos[i])}: label {int(lab[pos][i])}, but its gt {int(g[i])} has label {int(gl[g][i])}")
    neg_ = gi == 0
    bad = neg_ & ~((lab == -1) & (mo == -O2M_INF) & (am == 0))
    if bad.any():
        q = int(np.nonzero(bad)[0][0])
        raise Inadmissible(f"o2m query {q}: background, yet (label, max_overlap, metric) = ({int(lab[q])}, {mo[q]!r}, {am[q]!r}), "
                           f"expected (-1, -1e8, 0) exactly")
    sel_i = (iou[pos, g], ei[pos, g])
    sel_m = (dec["met"][0][pos, g], bound(dec["met"])[pos, g])
    _within("o2m max_overlaps(pos)", mo[pos], sel_i)
    _within("o2m assign_metrics(pos)", am[pos], sel_m)
    stats["iou_ratio"], stats["met_ratio"] = ratio(mo[pos], sel_i), ratio(am[pos], sel_m)
    if "labels_full" in res:
        lf, bt, nm = o2m_targets(inputs, gi, num_classes, dec)
        got_lf = np.asarray(res["labels_full"])
        if not np.array_equal(got_lf, lf):
            q = int(np.nonzero(got_lf != lf)[0][0])
            raise Inadmissible(f"o2m query {q}: labels_full {int(got_lf[q])}, expected {int(lf[q])} (gt_inds {int(gi[q])})")
        bad = neg_ & (np.any(_f(res["bbox_targets"]) != 0, 1) | (_f(res["norm_metrics"]) != 0))
        if bad.any():
            q = int(np.nonzero(bad)[0][0])
            raise Inadmissible(f"o2m query {q}: background, yet bbox_targets {_f(res['bbox_targets'])[q].tolist()} / norm_metrics "
                               f"{_f(res['norm_metrics'])[q]!r} are not exactly 0")
        _within("o2m bbox_targets", res["bbox_targets"], bt)
        _within("o2m norm_metrics", res["norm_metrics"], nm)
        stats["bt_ratio"], stats["nm_ratio"] = ratio(res["bbox_targets"], bt), ratio(res["norm_metrics"], nm)
    return stats


def o2m_ambiguity(inputs, topk=13, dynamic_k=False, alpha=1.0, beta=6.0):
    """Share of (query, gt) top-k memberships the checker lets go either way (inputs and bounds alone)."""
    d = o2m_decisions(inputs, topk, dynamic_k, alpha, beta)
    return float((d["certain"] != d["possible"]).mean()) if d["certain"].size else 0.0


# ------------------------------------------------------------------------------------------------------------------
# teacher decoding + NMS
# ------------------------------------------------------------------------------------------------------------------
def nms_quantities(logits, bbox_pred, img_h, img_w, score_thr=0.01):
    """-> scores (value, err) (Q, C), boxes: list of four (value, err) (Q,), maxc (the reference's boxes.max())."""
    with np.errstate(all="ignore"):
        one = const(1.0)
        s = div(one, add(one, exp_(neg(inp(logits)))))
        box = _decode(np.asarray(bbox_pred, np.float32), img_w, img_h, clip=True)
        cand = (s[0] > score_thr).any(1)
        maxc = max([float(c[0][cand].max()) for c in box]) if cand.any() else 0.0
        return s, box, maxc


def _pair_iou(box_a, box_b, off):
    """IoU (value, err) of boxes a (n, 4 pairs) against b (m, 4 pairs) in the class-offset frame (mmcv nms, offset 0)."""
    with np.errstate(all="ignore"):
        a = [(c[0][:, None], c[1][:, None] + 2 * U * np.abs(c[0][:, None] + off)) for c in box_a]
        b = [(c[0][None, :], c[1][None, :] + 2 * U * np.abs(c[0][None, :] + off)) for c in box_b]
        zero = const(0.0)
        w = fmax(sub(fmin(a[2], b[2]), fmax(a[0], b[0])), zero)
        h = fmax(sub(fmin(a[3], b[3]), fmax(a[1], b[1])), zero)
        inter = mul(w, h)
        sa, sb = mul(sub(a[2], a[0]), sub(a[3], a[1])), mul(sub(b[2], b[0]), sub(b[3], b[1]))
        v, e = div(inter, sub(add(sa, sb), inter))
        nan = np.isnan(v)                           # 0 / 0: "not above the threshold" in the reference and in the kernels
        return np.where(nan, 0.0, v), np.where(nan | ~np.isfinite(e), np.inf, e)


def _take(box, idx):
    return [(c[0][idx], c[1][idx]) for c in box]


def check_nms(logits, bbox_pred, img_h, img_w, dets, labels, score_thr=0.01, iou_thr=0.6, max_per_img=300, mutant=None,
              iou_exact=False):
    """dets (k, 5), labels (k,) of one image.  iou_exact: the case is built so that every IoU is exact in fp32 (the caller
    shows that), so the IoU allowance is zero and the strictness of `>` is decided."""
    logits = np.asarray(logits, np.float32)
    Q, C = logits.shape
    dets, labels = _f(dets).reshape(-1, 5), np.asarray(labels).reshape(-1)
    k = len(labels)
    stats = dict(score_ratio=0.0, box_ratio=0.0, used_allowance=0, returned=k)
    if len(dets) != k or k > max_per_img:
        raise Inadmissible(f"nms: {len(dets)} dets / {k} labels, max_per_img {max_per_img}")
    if Q == 0 or C == 0:
        if k:
            raise Inadmissible("nms: detections without queries")
        return stats
    thr = float(np.float32(score_thr))
    ithr = float(np.float32(iou_thr))
    s, box, maxc = nms_quantities(logits, bbox_pred, img_h, img_w, thr)
    es = bound(s)
    if np.any((labels < 0) | (labels >= C)):
        raise Inadmissible("nms: label outside [0, C)")
    # every returned detection is the decode of a real (query, class), each used once
    used = np.zeros((Q, C), bool)
    qs = np.empty(k, np.int64)
    bv, be = np.stack([c[0] for c in box], 1), np.stack([bound(c) for c in box], 1)
    for i in range(k):
        c = labels[i]
        ok = np.all(np.abs(bv - dets[i, :4]) <= be, 1) & (np.abs(s[0][:, c] - dets[i, 4]) <= es[:, c]) & ~used[:, c]
        if not ok.any():
            raise Inadmissible(f"nms det {i}: box {dets[i, :4].tolist()} score {dets[i, 4]!r} label {int(c)} is the decode of no "
                               f"unused (query, class) within bound")
        # among exact duplicates any will do; prefer the closest score
        q = int(np.nonzero(ok)[0][np.argmin(np.abs(s[0][ok, c] - dets[i, 4]))])
        used[q, c] = True
        qs[i] = q
        stats["score_ratio"] = max(stats["score_ratio"], abs(s[0][q, c] - dets[i, 4]) / es[q, c])
        rb = np.abs(bv[q] - dets[i, :4]) / np.where(be[q] > 0, be[q], np.inf)
        stats["box_ratio"] = max(stats["box_ratio"], float(rb.max()))
    sr, er = s[0][qs, labels], es[qs, labels]
    bad = ~(sr > thr - er)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise Inadmissible(f"nms det {i}: score {sr[i]!r} is not above score_thr {thr!r} (allowance {er[i]:.3e})")
    bad = ~(sr[:-1] >= sr[1:] - (er[:-1] + er[1:]))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise Inadmissible(f"nms det {i}, {i + 1}: scores {sr[i]!r} < {sr[i + 1]!r} beyond {er[i] + er[i + 1]:.3e}: not sorted")
    stats["used_allowance"] += int((sr <= thr + er).sum() + (sr[:-1] < sr[1:]).sum())
    full = k == max_per_img
    low = sr[-1] if k else np.inf
    classes = range(C) if mutant != "class_agnostic" else [None]
    for c in classes:
        kc = np.arange(k) if c is None else np.nonzero(labels == c)[0]
        off = 0.0 if c is None else c * (maxc + 1.0)
        kb = _take(box, qs[kc])
        if len(kc) > 1:                                     # no two returned detections of the class overlap
            v, e = _pair_iou(kb, kb, off)
            if iou_exact:
                e = np.zeros_like(e)
            over = np.triu(v > ithr + e, 1)
            if over.any():
                i, j = (int(x) for x in np.argwhere(over)[0])
                raise Inadmissible(f"nms dets {int(kc[i])}, {int(kc[j])} of class {c}: IoU {v[i, j]!r} > iou_thr {ithr!r} + allowance "
                                   f"{e[i, j]:.3e}, margin {v[i, j] - ithr:.3e}")
            stats["used_allowance"] += int(np.triu(v > ithr, 1).sum())
        if c is None:
            continue
        cq = np.nonzero((s[0][:, c] > thr + es[:, c]) & ~used[:, c])[0]          # sure candidates that were not returned
        if not len(cq):
            continue
        cut = full & (s[0][cq, c] <= low + 2 * es[cq, c])
        dom = np.zeros(len(cq), bool)
        sure = np.zeros(len(cq), bool)
        step = max(1, (1 << 22) // max(len(kc), 1))
        for a in range(0, len(cq), step):
            sl = slice(a, a + step)
            if len(kc):
                v, e = _pair_iou(_take(box, cq[sl]), kb, off)
                if iou_exact:
                    e = np.zeros_like(e)
                higher = sr[kc][None, :] >= s[0][cq[sl], c][:, None] - 2 * es[cq[sl], c][:, None]
                dom[sl] = (higher & (v > ithr - e)).any(1)
                sure[sl] = ((sr[kc][None, :] > s[0][cq[sl], c][:, None]) & (v > ithr + e)).any(1)
        bad = ~(dom | cut)
        if bad.any():
            q = int(cq[bad][0])
            raise Inadmissible(f"nms candidate (query {q}, class {c}): score {s[0][q, c]!r} > score_thr + {es[q, c]:.3e}, not returned, "
                               f"no returned detection of its class suppresses it and the output "
                               f"{'is full but its lowest score is ' + repr(low) if full else 'is not full'}")
        stats["used_allowance"] += int((~sure & ~(full & (s[0][cq, c] < low))).sum())
    return stats


def nms_ambiguity(logits, bbox_pred, img_h, img_w, score_thr=0.01, iou_thr=0.6):
    """Share of candidates whose threshold or suppression status the checker lets go either way (inputs alone): a score within
    its bound of score_thr, or an IoU within its bound of iou_thr against a same-class candidate of higher or near score."""
    logits = np.asarray(logits, np.float32)
    Q, C = logits.shape
    thr, ithr = float(np.float32(score_thr)), float(np.float32(iou_thr))
    s, box, maxc = nms_quantities(logits, bbox_pred, img_h, img_w, thr)
    es = bound(s)
    n_cand = n_amb = 0
    for c in range(C):
        cq = np.nonzero(s[0][:, c] > thr - es[:, c])[0]
        if not len(cq):
            continue
        amb = np.abs(s[0][cq, c] - thr) <= es[cq, c]
        b = _take(box, cq)
        step = max(1, (1 << 22) // len(cq))
        for a in range(0, len(cq), step):
            v, e = _pair_iou(_take(box, cq[a:a + step]), b, c * (maxc + 1.0))
            near = np.abs(v - ithr) <= e
            higher = s[0][cq, c][None, :] >= s[0][cq[a:a + step], c][:, None] - 2 * es[cq[a:a + step], c][:, None]
            np.fill_diagonal(near[:, a:a + step], False)
            amb[a:a + step] |= (near & higher).any(1)
        n_cand += len(cq)
        n_amb += int(amb.sum())
    return n_amb / max(n_cand, 1)


# ------------------------------------------------------------------------------------------------------------------
# mean + std filter
# ------------------------------------------------------------------------------------------------------------------
def pseudo_threshold(scores, mutant=None):
    """mean + unbiased std of the fp32 scores -> (value, err); NaN for K == 1 (and K == 0).  Any summation order."""
    sc = _f(np.asarray(scores, np.float32))
    K = len(sc)
    if K < 2:
        return np.float64("nan"), np.float64(0.0)
    with np.errstate(all="ignore"):
        mean = sc.mean()
        e_mean = 2 * U * (K * np.abs(sc).sum() / K + abs(mean)) + TINY
        d = sc - mean
        e_d = e_mean + 2 * U * np.abs(d)
        ss = (d * d).sum()
        e_ss = (2 * np.abs(d) * e_d).sum() + 2 * U * (K + 1) * ss + TINY
        var = _r(ss / (K if mutant == "population_std" else K - 1), e_ss / (K - 1))
        std = sqrt_(var)
        return add((mean, e_mean), std)


def check_pseudo_filter(proposal, labels, out_boxes, out_labels, out_scores, thr=None, mutant=None):
    prop = np.asarray(proposal, np.float32).reshape(-1, 5)
    K = len(prop)
    ob, ol, os_ = np.asarray(out_boxes).reshape(-1, 4), np.asarray(out_labels).reshape(-1), np.asarray(out_scores).reshape(-1)
    stats = dict(thr_ratio=0.0, used_allowance=0, kept=len(os_))
    t, e = pseudo_threshold(prop[:, 4], mutant)
    if K < 2:
        if len(os_) or len(ob) or len(ol):
            raise Inadmissible(f"pseudo filter: K = {K} must keep nothing")
        if thr is not None and K == 1 and not np.isnan(thr):
            raise Inadmissible(f"pseudo filter: K = 1 threshold {thr!r}, expected NaN")
        return stats
    if thr is not None:
        if not abs(float(thr) - t) <= e:
            raise Inadmissible(f"pseudo filter threshold: got {float(thr)!r}, fp64 {t!r}, |diff| {abs(float(thr) - t):.3e} > {e:.3e}")
        stats["thr_ratio"] = abs(float(thr) - t) / e
    sc = _f(prop[:, 4])
    valid = ((prop[:, 2] - prop[:, 0]) > 0) & ((prop[:, 3] - prop[:, 1]) > 0)            # exact fp32 differences' signs
    must = valid & (sc - t > e)
    may = valid & (sc - t >= -e)
    # the returned rows are rows of the input, in order: match them greedily
    idx, j = [], 0
    for i in range(len(os_)):
        while j < K and not (may[j] and np.array_equal(prop[j, :4], ob[i]) and prop[j, 4] == os_[i]
                             and (labels is None or np.asarray(labels)[j] == ol[i])):
            if must[j]:
                raise Inadmissible(f"pseudo filter item {j}: score {sc[j]!r} - thr {t!r} = {sc[j] - t:.3e} > allowance {e:.3e}, "
                                   f"yet it is dropped (or out of order)")
            j += 1
        if j == K:
            raise Inadmissible(f"pseudo filter: returned row {i} (score {os_[i]!r}) is no admissible input row in order "
                               f"(thr {t!r} +- {e:.3e})")
        idx.append(j)
        j += 1
    rest = np.nonzero(must[j:])[0]
    if len(rest):
        q = int(rest[0]) + j
        raise Inadmissible(f"pseudo filter item {q}: score {sc[q]!r} - thr {t!r} = {sc[q] - t:.3e} > allowance {e:.3e}, yet dropped")
    idx = np.asarray(idx, np.int64)
    stats["used_allowance"] = int((~must[idx]).sum()) if len(idx) else 0
    return stats


def pseudo_ambiguity(proposal):
    prop = np.asarray(proposal, np.float32).reshape(-1, 5)
    if len(prop) < 2:
        return 0.0
    t, e = pseudo_threshold(prop[:, 4])
    return float((np.abs(_f(prop[:, 4]) - t) <= e).mean())


# ------------------------------------------------------------------------------------------------------------------
# weak -> strong box warp
# ------------------------------------------------------------------------------------------------------------------
def transform_bboxes(boxes, M, out_h, out_w, mutant=None):
    """boxes (K, 4) xyxy, M (3, 3) -> (value, err) (K, 4): four corners through the homography, min / max, clip."""
    with np.errstate(all="ignore"):
        b = inp(np.asarray(boxes, np.float32).reshape(-1, 4)[:, :4])
        m = [const(v) for v in np.asarray(M, np.float32).reshape(9)]
        x0, y0, x1, y1 = (_col(b, k) for k in range(4))
        corners = [(x0, y0), (x1, y1)] if mutant == "two_corners" else [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        us, vs = [], []
        for px, py in corners:
            x = add(add(mul(m[0], px), mul(m[1], py)), m[2])
            y = add(add(mul(m[3], px), mul(m[4], py)), m[5])
            z = add(add(mul(m[6], px), mul(m[7], py)), m[8])
            us.append(div(x, z)); vs.append(div(y, z))
        def red(f, xs):
            r = xs[0]
            for x in xs[1:]:
                r = f(r, x)
            return r
        zero, W, H = const(0.0), inp(out_w), inp(out_h)
        out = [fmin(fmax(red(fmin, us), zero), W), fmin(fmax(red(fmin, vs), zero), H),
               fmin(fmax(red(fmax, us), zero), W), fmin(fmax(red(fmax, vs), zero), H)]
        return np.stack([o[0] for o in out], -1), np.stack([bound(o) for o in out], -1)


def check_transform(boxes, M, out_h, out_w, out, mutant=None):
    ref = transform_bboxes(boxes, M, out_h, out_w, mutant)
    got = _f(out).reshape(-1, np.shape(out)[-1] if np.ndim(out) > 1 else 4)[:, :4]
    _within("transform_bboxes", got, ref)
    return dict(box_ratio=ratio(got, ref), used_allowance=0)

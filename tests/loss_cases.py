"""The inputs of tests/test_loss_ref64.py (CPU: eval_f32 and the C oracle must be admissible on each, every mutant rejected on
some) and of tests/test_gpu_loss_admissible.py (GPU: the kernels must be).  Plain helper module, numpy only.  Every case is
deterministic, named, and says what it aims at.  A set_loss case is ONE launch of three segments -- matched (focal), warm-up
(task-aligned focal) and dn -- of the same layout, so every case runs all three segment kinds.

Base layout: nl 2, B 2, Q 70 (140 rows: two full 64-row chunks and a 12-row tail), C 80 (the float4 path), dn single_pad 6 x 3
groups.  `targets` of a case: {segment index: [(layer, image, row), ...]} -- the rows it is about; the CPU test asserts that the
gradient elements of those rows have a finite bound (saturated warm-up rows: finite and non-negative results instead).

Cases of the issue that are worded differently here, and why:
  * "wm != 0 with wsum == 0 but a single positive weight" cannot hold as written (wm is wsum / 4).  What separates statistic 6
    (wsum > 0) from statistic 7 (any w > 0) is a row whose weights cancel: (0.5, -0.5, 0, 0) in `weights`.
  * "a box of 2^-12 of the image on the 1333 x 800 image, so that uraw is near eps from above": that box has an area of 0.06 px^2,
    five orders above eps = 1e-6.  It is kept as worded (`boxes_tiny_1333`: inexact corners, ties by identical inputs), and
    `tiny_equal` in `boxes_dyadic` (sides 2^-20 of 512 px, area 2^-22 px^2 < eps, nonzero sides) is the row on which the union
    clamp is active with a nonzero area gradient behind it.
"""
import numpy as np

import set_loss_ref64 as R

F = np.float32
P_DEF = dict(alpha=0.25, gamma=2.0, cls_weight=2.0, l1_weight=5.0, iou_weight=2.0, iou_eps=1e-6, bg_cls_weight=0.0)
WH_ORD = [[640.0, 480.0], [1333.0, 800.0]]
WH_DY = [[512.0, 512.0], [1024.0, 768.0]]
SPECIAL = [0.0, 2.0 ** -10, -2.0 ** -10, 8.0, -8.0, 16.5, -16.5, 17.5, -17.5, 30.0, -30.0, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4,
           1e-40]
METRICS = [0.0, 2.0 ** -20, 0.5, 1.0]


def _boxes(r, shape):
    return np.concatenate([r.random(shape + (2,)) * 0.8 + 0.1, r.random(shape + (2,)) * 0.4 + 0.02], -1).astype(F)


def _xyxy(c, wh):
    w, h = wh
    return (np.stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2], -1).astype(np.float64)
            * [w, h, w, h]).astype(F)


def base(name, aim, seed, nl=2, B=2, Q=70, C=80, sp=6, groups=3, counts=(3, 5), wh=WH_ORD, ordinary=False, **params):
    r = np.random.default_rng(seed)
    P = dict(P_DEF, **params)
    wh = np.asarray(wh, F)[:B]
    segs = []
    for kind in (R.MATCHED, R.WARMUP):
        warm = kind == R.WARMUP
        x = (r.standard_normal((nl, B, Q, C)) * 3).astype(F)
        if warm:
            x = np.clip(x * F(0.5), -6.0, 6.0).astype(F)
        labels = np.where(r.random((nl, B, Q)) < 0.2, r.integers(0, C, (nl, B, Q)), C)
        pos = labels < C
        tg = (_boxes(r, (nl, B, Q)) * pos[..., None]).astype(F)
        bw = np.repeat(pos[..., None], 4, -1).astype(F)
        metrics = None
        if warm:
            metrics = (r.random((nl, B, Q)) * pos).astype(F)
            bw = bw * metrics[..., None]
        segs.append(dict(kind=kind, cls=x, boxes=_boxes(r, (nl, B, Q)), labels=labels, label_weights=None if warm else
                         np.ones((nl, B, Q), F), bbox_targets=tg, bbox_weights=bw, metrics=metrics, wh=wh, params=P))
    qd = sp * groups
    gts = [_xyxy(_boxes(r, (n,)), wh[b]) for b, n in enumerate(counts)]
    labs = [r.integers(0, C, n) for n in counts]
    segs.append(dict(kind=R.DN, cls=(r.standard_normal((nl, B, qd, C)) * 3).astype(F), boxes=_boxes(r, (nl, B, qd)), gts=gts,
                     labs=labs, single_pad=sp, groups=groups, wh=wh, params=P))
    coef = (r.random((3 * nl, 5)) + 0.5).astype(F)
    return dict(name=name, aim=aim, segs=segs, coef=coef, ordinary=ordinary, saturated=False, targets={}, unaligned=False)


def _make_pos(seg, l, b, q, c, metric=0.5):
    """row (l, b, q) of a matched / warm-up segment becomes a positive of class c with unit (warm-up: metric) box weights"""
    seg["labels"][l, b, q] = c
    if seg["kind"] == R.WARMUP:
        seg["metrics"][l, b, q] = metric
        seg["bbox_weights"][l, b, q] = metric
    else:
        seg["bbox_weights"][l, b, q] = 1.0
    if not seg["bbox_targets"][l, b, q].any():
        seg["bbox_targets"][l, b, q] = [0.5, 0.5, 0.25, 0.25]


def logits_grid(gamma, alpha, bg):
    """Every special logit at the labelled class AND off it, in all three segments (layer 0, image 0, rows 0..17); the warm-up
    rows cycle the metrics 0 (on a positive row), 2^-20, 0.5, 1.  Aims: the -100 clamp of both logs, the max((1-p)p, 1e-12)
    clamp, p(1-p) underflow, expf overflow (|x| >= 88.8), the softplus / log1p branch of the focal element at both signs, and
    for gamma != 2 powf, the ad > 0 guard and the sign.  dn: single_pad 9 x 2 groups with 9 gts, so all 18 rows are positives."""
    p = base(f"logits_g{gamma:g}", logits_grid.__doc__, 100 + int(gamma * 10), sp=9, groups=2, counts=(9, 2), gamma=gamma,
             alpha=alpha, bg_cls_weight=bg)
    C = 80
    for si, seg in enumerate(p["segs"]):
        rows = []
        for r_, v in enumerate(SPECIAL):
            if seg["kind"] == R.DN:
                c = int(seg["labs"][0][r_ % 9])
            else:
                c = (7 * r_) % C
                _make_pos(seg, 0, 0, r_, c, METRICS[r_ % 4])
            seg["cls"][0, 0, r_, c] = v
            seg["cls"][0, 0, r_, (c + 1) % C] = v
            rows.append((0, 0, r_))
        p["targets"][si] = rows
    p["saturated"] = True
    return p


# name, prediction, target (normalised cxcywh, dyadic: every corner is exact on 512 x 512 and 1024 x 768)
BOX_FAMILY = [
    ("equal", (0.5, 0.5, 0.25, 0.25), (0.5, 0.5, 0.25, 0.25)),                    # bitwise equal: every max / min ties, sign(0)
    ("shared_edge", (0.5625, 0.5, 0.125, 0.125), (0.5, 0.5, 0.25, 0.25)),        # right edges tie, the rest decided
    ("touching", (0.75, 0.5, 0.25, 0.125), (0.5, 0.5, 0.25, 0.25)),              # rb - lt == 0 in x: the >= 0 gate at zero (the
                                                                                   # heights differ, or dO = 1/e - 1/u would be 0)
    ("disjoint", (0.125, 0.125, 0.125, 0.125), (0.5, 0.5, 0.25, 0.25)),
    ("contained", (0.5, 0.5, 0.125, 0.125), (0.5, 0.5, 0.25, 0.25)),
    ("zero_width", (0.5, 0.5, 0.0, 0.25), (0.5, 0.5, 0.25, 0.25)),
    ("same_point", (0.5, 0.5, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0)),                   # both clamps active, erb - elt == 0
    ("tiny_equal", (0.5, 0.5, 2.0 ** -20, 2.0 ** -20), (0.5, 0.5, 2.0 ** -20, 2.0 ** -20)),   # uraw, eraw < eps with nonzero sides
]


def _plant_boxes(p, family, layers=(0, 1)):
    n = len(family)
    pred = np.asarray([f[1] for f in family], F)
    tgt = np.asarray([f[2] for f in family], F)
    for si, seg in enumerate(p["segs"]):
        B = seg["cls"].shape[1]
        rows = []
        for b in range(B):
            if seg["kind"] == R.DN:
                seg["gts"][b] = _xyxy(tgt, seg["wh"][b])
                seg["labs"][b] = np.arange(n) % seg["cls"].shape[3]
                for g in range(seg["groups"]):
                    seg["boxes"][:, b, g * seg["single_pad"]:g * seg["single_pad"] + n] = pred
            else:
                for l in layers:
                    for q in range(n):
                        _make_pos(seg, l, b, q, q % seg["cls"].shape[3])
                        seg["bbox_targets"][l, b, q] = tgt[q]
                        seg["boxes"][l, b, q] = pred[q]
            rows += [(l, b, q) for l in layers for q in range(n)]
        p["targets"][si] = rows
    return p


def boxes_dyadic():
    """The box family above on 512 x 512 and 1024 x 768, where every corner is exact in fp32 and the ties are exact: the tie
    rule dmax_a / dmin_a == 0.5, the gates rb - lt >= 0 and erb - elt >= 0 at exactly zero, fmaxf(uraw, eps) / fmaxf(eraw, eps)
    with the clamp active and the dmax_a(uraw, eps) factor of the gradient, sign(0) of the L1 gradient."""
    p = base("boxes_dyadic", boxes_dyadic.__doc__, 31, wh=WH_DY, sp=8, groups=2, counts=(8, 8))
    return _plant_boxes(p, BOX_FAMILY)


def boxes_tiny_1333():
    """A box of 2^-12 of the image on 1333 x 800 against itself and against one twice as wide: corners are not exact there, so
    the ties of row 0 hold by identical inputs alone.  (The dn segment divides the rounded gt by the size again: its targets
    differ from the prediction in the last bit, and its rows are hulls or decided by a hair -- not named as targets.)"""
    p = base("boxes_tiny_1333", boxes_tiny_1333.__doc__, 32, wh=[[1333.0, 800.0], [512.0, 512.0]], sp=6, groups=3, counts=(2, 2))
    t = 2.0 ** -12
    fam = [("tiny_equal_1333", (0.5, 0.5, t, t), (0.5, 0.5, t, t)), ("tiny_wider_1333", (0.5, 0.5, 2 * t, t), (0.5, 0.5, t, t))]
    _plant_boxes(p, fam)
    del p["targets"][2]
    return p


def weights_and_labels():
    """Labels -1, C and C + 5 (all background), label_weights 0 and 0.3, bbox_weights (0.5, 0, 0, 0), (0, 0, 0, 0) on a positive
    row, (1, 1, 1, 1) and the cancelling (0.5, -0.5, 0, 0) (statistic 6 != statistic 7), a warm-up metric of 0 on a positive row,
    alpha 0.5, bg_cls_weight 0.1, and layer 1 without any positive row: both normalisers clamp to 1 and the GIoU scale is 0."""
    p = base("weights_and_labels", weights_and_labels.__doc__, 33, alpha=0.5, bg_cls_weight=0.1)
    C = 80
    for si, seg in enumerate(p["segs"][:2]):
        seg["labels"][1] = C
        seg["bbox_weights"][1] = 0.0
        if seg["kind"] == R.WARMUP:
            seg["metrics"][1] = 0.0
        for q, c in enumerate((3, 4, 5, 6)):
            _make_pos(seg, 0, 0, q, c, 0.0 if q == 1 else 0.5)
        seg["labels"][0, 0, 4:7] = [-1, C, C + 5]
        seg["bbox_weights"][0, 0, 0] = [0.5, 0, 0, 0]
        seg["bbox_weights"][0, 0, 1] = 0.0
        seg["bbox_weights"][0, 0, 2] = 1.0
        seg["bbox_weights"][0, 0, 3] = [0.5, -0.5, 0, 0]
        if seg["kind"] == R.MATCHED:
            seg["label_weights"][0, 0, 0] = 0.0
            seg["label_weights"][0, 0, 2:7] = 0.3
        p["targets"][si] = [(0, 0, q) for q in range(7)]
    return p


def set_loss_cases():
    cases = [base("ordinary_a", "seeded, the ranges of test_gpu_set_loss._problem", 1, ordinary=True),
             base("ordinary_b", "seeded, the ranges of test_gpu_set_loss._problem", 2, ordinary=True, counts=(6, 0)),
             base("layout_C7", "C 7: the element path (C % 4 != 0)", 3, C=7),
             base("layout_C80_unaligned", "C 80 through views whose pointer is 4 bytes off the 16-byte grid: the element path", 4),
             base("layout_C1", "C 1", 5, C=1),
             base("layout_Q1", "Q 1 (dn: one query, one gt in image 0, none in image 1)", 6, Q=1, sp=1, groups=1, counts=(1, 0)),
             base("dn_groups1", "dn: single_pad 6, one group", 7, groups=1),
             base("dn_G_eq_pad", "dn: G == single_pad in image 0 (no padding row)", 8, counts=(6, 1)),
             base("dn_G0", "dn: no gt in any image: every dn loss and every dn gradient is an exact 0", 9, counts=(0, 0))]
    cases[3]["unaligned"] = True
    cases += [logits_grid(2.0, 0.25, 0.0), logits_grid(1.5, 0.5, 0.1), logits_grid(1.0, 0.25, 0.1), logits_grid(3.0, 0.5, 0.0)]
    cases += [weights_and_labels(), boxes_dyadic(), boxes_tiny_1333()]
    return cases


# ----------------------------------------------------------------------------------------------------------------------
# tal_loss entry
# ----------------------------------------------------------------------------------------------------------------------
def _tal(name, aim, x, lab, met, gamma=2.0, prob=False, ordinary=False, saturated=False, targets=()):
    return dict(name=name, aim=aim, logits=np.ascontiguousarray(x, F), labels=np.asarray(lab, np.int64), metrics=np.asarray(met, F),
                gamma=gamma, input_is_prob=prob, ordinary=ordinary, saturated=saturated, targets=list(targets))


def _tal_random(r, N, C, scale=1.5):
    x = np.clip(r.standard_normal((N, C)) * scale, -6.0, 6.0).astype(F)
    lab = np.where(r.random(N) < 0.3, r.integers(0, C, N), C)
    met = (r.random(N) * (lab < C)).astype(F)
    return x, lab, met


def tal_cases():
    out = []
    r = np.random.default_rng(50)
    for N, C in ((1, 1), (341, 3), (128, 8), (205, 5)):
        x, lab, met = _tal_random(r, N, C)
        if N == 1:
            lab, met = np.array([0]), np.array([0.5], F)
        out.append(_tal(f"layout_{N * C}", f"N x C = {N * C} elements: around one workgroup's 1024", x, lab, met, ordinary=True))
    x, lab, met = _tal_random(r, 13108, 80)
    out.append(_tal("layout_second_trip", "13108 x 80 > 1024 workgroups x 1024 elements: the grid-stride loop's second trip", x, lab,
                    met, ordinary=True))
    for gamma in (2.0, 1.5, 1.0, 3.0):
        x, lab, met = _tal_random(r, 64, 40)
        tg = []
        for i, v in enumerate(SPECIAL):
            c = (3 * i) % 40
            lab[i], met[i] = c, METRICS[i % 4]
            x[i, c], x[i, (c + 1) % 40] = v, v
            tg += [(i, c), (i, (c + 1) % 40)]
        out.append(_tal(f"logits_g{gamma:g}", "every special logit at the labelled class and off it, metrics 0 / 2^-20 / 0.5 / 1; "
                        "gamma != 2: powf, the ad > 0 guard and the sign, value and gradient", x, lab, met, gamma, saturated=True,
                        targets=tg))
    for gamma in (2.0, 1.5):
        ps = [0.0, 2.0 ** -149, 0.5, 1.0 - 2.0 ** -24, 1.0]
        x = (r.random((32, 8)) * 0.98 + 0.01).astype(F)
        lab = np.where(r.random(32) < 0.4, r.integers(0, 8, 32), 8)
        met = (r.random(32) * (lab < 8)).astype(F)
        tg = []
        for i, v in enumerate(ps):
            lab[i], met[i] = i, METRICS[(i + 1) % 4]
            x[i, i], x[i, i + 1] = v, v
            tg += [(i, i), (i, i + 1)]
        lab[6], met[6] = 2, F(0.3)
        x[6, 2] = met[6]                                   # p == s bitwise: d == 0, the ad > 0 guard
        lab[7], met[7], x[7, 3] = 3, 0.5, 0.5
        tg += [(6, 2), (7, 3)]
        out.append(_tal(f"prob_g{gamma:g}", "input_is_prob with p in {0, 2^-149, 0.5, 1 - 2^-24, 1} on and off the labelled class, and "
                        "p == s bitwise (gamma 1.5: powf(0, 0.5) and the guard)", x, lab, met, gamma, prob=True, targets=tg))
    return out


def focal_cases():
    out = []
    r = np.random.default_rng(70)
    for name, N, C, gamma, alpha, weighted in (("focal_C80", 70, 80, 2.0, 0.25, True), ("focal_C7_g1.5", 70, 7, 1.5, 0.5, False)):
        x = (r.standard_normal((N, C)) * 3).astype(F)
        lab = np.where(r.random(N) < 0.3, r.integers(0, C, N), C)
        for i, v in enumerate(SPECIAL):
            c = i % C
            lab[i] = c
            x[i, c], x[i, (c + 1) % C] = v, v
        w = (r.random(N)).astype(F) if weighted else None
        if weighted:
            w[:2] = [0.0, 0.3]
        out.append(dict(name=name, aim="FocalLoss drop-in: special logits on and off the label, row weights 0 / 0.3", logits=x, labels=lab,
                        weights=w, alpha=alpha, gamma=gamma))
    return out

"""The inputs of tests/test_assign_ref64.py (CPU: the oracle must be admissible on each) and of
tests/test_gpu_assign_admissible.py (GPU: the kernels must be).  Plain helper module, numpy only.  Problems of one batch share
(Q, C) so that the batched entry points take a whole family in one launch.  `ordinary` batches are seeded random inputs,
continuous and well separated, on which exact equality with the oracle holds as well: for O2M and NMS the generators of the
existing parity tests; for the matcher the batch of test_assign_batch_ragged_like_a_loss_call itself (N(0, 3) logits, 0...15
gts: admissible and equal to the oracle, no cap on the open share) and a second one with the logits of a trained head and few
gts, for which the 1 % cap on the allowance is asserted (ordinary_hungarian says why).  Every other batch is adversarial and
says what it aims at.  Also the small accessors both test modules share."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    """tests/golden/<name> grouped by case: {'case': {'field': array}} for keys 'case.field'."""
    z = np.load(os.path.join(GOLD, name))
    cases = {}
    for k in z.files:
        if "." in k:
            c, f = k.split(".", 1)
            cases.setdefault(c, {})[f] = z[k]
    return cases


def h_inputs(p):
    return dict(bbox_pred=p["bbox_pred"], cls_pred=p["cls"], gt_bboxes=p["gt_bboxes"], gt_labels=p["gt_labels"],
                img_w=p["img_w"], img_h=p["img_h"])


def o_inputs(p):
    return dict(bbox_pred=p["bbox_pred"], cls_prob=p["cls"], gt_bboxes=p["gt_bboxes"], gt_labels=p["gt_labels"],
                img_w=p["img_w"], img_h=p["img_h"])

F = np.float32
SEED_HUNGARIAN = 87
MAX_SMALL_G = 5


def _boxes(rng, n, lo=0.02, hi=0.5):
    return np.concatenate([rng.random((n, 2)), rng.random((n, 2)) * (hi - lo) + lo], -1).astype(F)


def _gts(rng, n, w=1000.0, h=600.0, sw=300.0, sh=200.0):
    xy = rng.random((n, 2)) * [w, h]
    return np.concatenate([xy, xy + rng.random((n, 2)) * [sw, sh] + 16], -1).astype(F)


def _to_cxcywh(gt, w, h):
    n = gt / np.asarray([w, h, w, h], F)
    return np.stack([(n[:, 0] + n[:, 2]) / 2, (n[:, 1] + n[:, 3]) / 2, n[:, 2] - n[:, 0], n[:, 3] - n[:, 1]], -1).astype(F)


def _prob(name, bp, cls, gt, gl, w=1333.0, h=800.0):
    return dict(name=name, bbox_pred=np.ascontiguousarray(bp, F), cls=np.ascontiguousarray(cls, F),
                gt_bboxes=np.ascontiguousarray(gt, F).reshape(-1, 4), gt_labels=np.asarray(gl, np.int64), img_w=float(w),
                img_h=float(h))


def adversarial_problems(Q, C, kind, seed=0):
    """kind 'logit' (Hungarian / NMS: cls are logits) or 'prob' (O2M: probabilities).  Each problem names its aim."""
    rng = np.random.default_rng(seed)

    def cls(n=Q):
        x = (rng.standard_normal((n, C)) * 3).astype(F)
        return x if kind == "logit" else (1 / (1 + np.exp(-x))).astype(F)

    def near(gt, w=1333.0, h=800.0, noise=0.05):
        bp = _boxes(rng, Q)
        src = rng.integers(0, len(gt), Q // 2)
        bp[:Q // 2] = (_to_cxcywh(gt[src], w, h) * (1 + rng.normal(0, noise, (Q // 2, 4)))).clip(0.001, 0.999)
        return bp

    out = []
    G = min(5, Q)
    gt, gl = _gts(rng, G), rng.integers(0, C, G)
    # every prediction duplicated 2-8 times exactly: all costs / metrics / scores of a group tie, the matching must still be one
    base, c0 = near(gt)[:max(Q // 4, 1)], cls(max(Q // 4, 1))
    rep = np.resize(np.repeat(np.arange(len(base)), rng.integers(2, 9, len(base))), Q)
    out.append(_prob("dup_predictions", base[rep], c0[rep], gt, gl))
    # two identical gts with the same label, three with different labels: equal columns, ties between gts
    g2 = np.concatenate([gt, gt[:1]])
    out.append(_prob("dup_gt_same_label", near(g2), cls(), g2, np.concatenate([gl, gl[:1]])))
    g3 = np.concatenate([gt, gt[1:2], gt[1:2]])
    out.append(_prob("dup_gt_diff_label", near(g3), cls(), g3, np.concatenate([gl, (gl[1:2] + 1) % C, (gl[1:2] + 2) % C])))
    # prediction exactly equal to a gt (power-of-two image so that the normalisation is exact): L1 = 0, IoU = 1
    ge = (np.floor(rng.random((G, 4)) * 8) * 32).astype(F)
    ge[:, 2:] = ge[:, :2] + (np.floor(rng.random((G, 2)) * 6) + 1) * 32
    bp = _boxes(rng, Q)
    bp[:G] = _to_cxcywh(ge, 512, 512)
    out.append(_prob("pred_equals_gt", bp, cls(), ge, gl, 512, 512))
    # degenerate predictions: w = 0, h = 0, both, negative w (the eps of the union, the clamps of overlap and enclosure)
    bp = near(gt)
    bp[0::4, 2] = 0; bp[1::4, 3] = 0; bp[2::8, 2:] = 0; bp[3::8, 2] *= -1
    out.append(_prob("degenerate_pred", bp, cls(), gt, gl))
    # gts of zero area (pseudo labels clipped to a border), and a prediction that equals one: union and enclosure are 0
    gz = gt.copy()
    gz[0, 2] = gz[0, 0]; gz[1, 3] = gz[1, 1]; gz[2, 2:] = gz[2, :2]
    bp = near(gt)
    bp[0] = [gz[2, 0] / 1333, gz[2, 1] / 800, 0, 0]
    out.append(_prob("zero_area_gt", bp, cls(), gz, gl))
    # the same on a power-of-two image, where prediction and zero-area gt are the same point exactly: enclosing area 0, which
    # only its 1e-6 clamp keeps from 0 / 0
    gp = np.concatenate([np.asarray([[256, 512, 256, 512]], F), gt[1:] * F(0.5)])
    bp = near(gp, 1024, 1024)
    bp[0] = [0.25, 0.5, 0, 0]
    out.append(_prob("pred_equals_zero_area_gt", bp, cls(), gp, gl, 1024, 1024))
    # boxes wholly outside the image and larger than it (no clip in the assigners; the clip of the teacher's decode)
    bp = near(gt)
    bp[0::3, :2] += 1.5; bp[1::3, :2] -= 1.5; bp[2::6, 2:] = 3.0
    out.append(_prob("outside_and_oversized", bp, cls(), gt, gl))
    # an image of 1 x 1 and one of 1333 x 1: every pixel quantity is tiny, the 1e-6 clamps come into reach
    g1 = np.concatenate([rng.random((G, 2)) * 0.5, rng.random((G, 2)) * 0.5 + 0.5], -1).astype(F)
    out.append(_prob("image_1x1", near(g1, 1, 1), cls(), g1, gl, 1, 1))
    gw = g1 * np.asarray([1333, 1, 1333, 1], F)
    out.append(_prob("image_1333x1", near(gw, 1333, 1), cls(), gw, gl, 1333, 1))
    # saturation: 1 - p cancels (|x| >= 17), exp overflows (90); for O2M probabilities exactly 0 and 1
    vals = np.asarray([15, -15, 17, -17, 40, -40, 90, -90], F)
    cs = vals[rng.integers(0, 8, (Q, C))]
    if kind == "prob":
        cs = np.asarray([0, 1, 1e-30, 1 - 2.0 ** -24, 0.5, 2.0 ** -126, 1, 0], F)[rng.integers(0, 8, (Q, C))]
    out.append(_prob("saturated", near(gt), cs, gt, gl))
    # all-equal logits and boxes: every cost / metric / score ties
    one = np.tile(_to_cxcywh(gt[:1], 1333, 800), (Q, 1))
    out.append(_prob("all_equal", one, np.full((Q, C), 0.25, F), gt, gl))
    # quantised inputs: logits on a grid of 1/4 (probabilities 1/8), boxes on 1/64: many metrics and IoUs tie exactly
    bq = (np.round(near(gt, 1024, 1024, 0.2) * 64) / 64).astype(F)
    bq[:, 2:] = np.maximum(bq[:, 2:], 1 / 64)
    cq = np.round(cls() * (4 if kind == "logit" else 8)) / (4 if kind == "logit" else 8)
    out.append(_prob("quantised", bq, cq, np.round(gt * 0.75 / 16) * 16 + [0, 0, 16, 16], gl, 1024, 1024))
    # G = 1, G = Q, G = Q + 1 (more gts than queries)
    out.append(_prob("G1", near(gt), cls(), gt[:1], gl[:1]))
    for n, nm in ((Q, "G_eq_Q"), (Q + 1, "G_eq_Q_plus_1")):
        gg = _gts(rng, n)
        out.append(_prob(nm, near(gg), cls(), gg, rng.integers(0, C, n)))
    return out


def ordinary_hungarian():
    """The loss-call shape of tests/test_gpu_matcher.py::test_assign_batch_ragged_like_a_loss_call: 7 layers x 5 images,
    0...100 gts.  Logits as a trained head gives them, N(-2, 1.5), rather than N(0, 3): at a logit of 10 the fp32 rounding of
    1 - p alone moves -log(1 - p + eps) by 5e-3, and the allowance on an optimum of such pairs would exceed 1 % of the gap to the
    second-best assignment (test_assign_ref64.py asserts that cap for this seed).  0...5 gts (and the fixed 0 and 100): the
    allowance is a sum over the G optimal pairs, about 2.5e-5 each from the rounding of 1333-pixel coordinates, while the gap to
    the second-best of 900 x G random costs shrinks with G (about 0.01 at G = 12), so beyond a handful of gts no seed meets 1 %."""
    rng = np.random.default_rng(SEED_HUNGARIAN)
    B, Q, C = 35, 900, 80
    counts = [int(x) for x in rng.integers(0, MAX_SMALL_G + 1, B)]
    counts[3], counts[7] = 0, 100
    bp = np.concatenate([rng.random((B, Q, 2)), rng.random((B, Q, 2)) * 0.5 + 0.01], -1).astype(F)
    cp = (rng.standard_normal((B, Q, C)) * 1.5 - 2).astype(F)
    out = []
    for b in range(B):
        xy = rng.random((counts[b], 2)) * [1000, 600]
        wh = rng.random((counts[b], 2)) * [300, 200] + 16
        out.append(_prob(f"loss_call[{b}]", bp[b], cp[b], np.concatenate([xy, xy + wh], -1),
                         rng.integers(0, C, counts[b]), 1333 - 7 * (b % 3), 800))
    return out


def loss_call_hungarian():
    """Exactly the inputs of tests/test_gpu_matcher.py::test_assign_batch_ragged_like_a_loss_call: N(0, 3) logits, 0...15 gts."""
    rng = np.random.default_rng(77)
    B, Q, C = 35, 900, 80
    counts = [int(x) for x in rng.integers(0, 16, B)]
    counts[3], counts[7] = 0, 100
    bp = np.concatenate([rng.random((B, Q, 2)), rng.random((B, Q, 2)) * 0.5 + 0.01], -1).astype(F)
    cp = (rng.standard_normal((B, Q, C)) * 3).astype(F)
    out = []
    for b in range(B):
        xy = rng.random((counts[b], 2)) * [1000, 600]
        wh = rng.random((counts[b], 2)) * [300, 200] + 16
        out.append(_prob(f"ragged_loss_call[{b}]", bp[b], cp[b], np.concatenate([xy, xy + wh], -1),
                         rng.integers(0, C, counts[b]), 1333 - 7 * (b % 3), 800))
    return out


def hungarian_batches():
    out = [dict(name="ordinary_35x900x80", ordinary=True, problems=ordinary_hungarian()),
           dict(name="ordinary_ragged_loss_call", ordinary=True, problems=loss_call_hungarian()),
           dict(name="adversarial_Q48_C8", ordinary=False, problems=adversarial_problems(48, 8, "logit", 1))]
    for Q, C in ((1023, 1), (1025, 365), (2047, 3), (2049, 2)):       # one below / above 1024 and 2048; C = 1 and C = 365
        rng = np.random.default_rng(Q)
        gt = _gts(rng, 3)
        out.append(dict(name=f"boundary_Q{Q}_C{C}", ordinary=False,
                        problems=[_prob(f"Q{Q}", _boxes(rng, Q), rng.standard_normal((Q, C)) * 3, gt, rng.integers(0, C, 3))]))
    return out


def _o2m_random(seed, Q, C, G, iw=640, ih=480):
    """tests/test_gpu_o2m.py::test_o2m_random_vs_oracle's generator."""
    rng = np.random.default_rng(seed)
    gt = np.concatenate([rng.random((G, 2)) * [400, 300], np.zeros((G, 2))], -1)
    gt[:, 2:] = gt[:, :2] + rng.random((G, 2)) * 200 + 10
    gt = gt.astype(F)
    bp = _boxes(rng, Q, 0.02, 0.42)
    if G:
        src = rng.integers(0, G, Q // 2)
        bp[:Q // 2] = (_to_cxcywh(gt[src], iw, ih) * (1 + rng.normal(0, 0.1, (Q // 2, 4)))).clip(0.001, 0.999)
    return _prob(f"random_Q{Q}_G{G}", bp, rng.random((Q, C)) ** 2, gt, rng.integers(0, C, G), iw, ih)


MODES = [("static", 13, False), ("teacher_k1", 1, False), ("dynamic_k", 13, True)]


def o2m_batches():
    out = [dict(name="ordinary_900x80", ordinary=True, modes=MODES,
                problems=[_o2m_random(100 + g, 900, 80, g) for g in (7, 0, 1, 30, 100)]),
           dict(name="ordinary_Q2048_G1024", ordinary=True, modes=MODES[:1], problems=[_o2m_random(5, 2048, 91, 1024)]),
           dict(name="adversarial_Q48_C8", ordinary=False, modes=MODES, problems=adversarial_problems(48, 8, "prob", 2)),
           # Q = k and Q = k + 1: the top-k takes every query / all but one
           dict(name="adversarial_Q13", ordinary=False, modes=MODES, problems=adversarial_problems(13, 4, "prob", 3)),
           dict(name="adversarial_Q14", ordinary=False, modes=MODES, problems=adversarial_problems(14, 4, "prob", 4))]
    # one below / above 1024, one below 2048; Q = 2049 is refused by the entry point ("at most 2048 queries", kept by
    # test_o2m_errors_and_teacher_assign), and Q < k raises torch.topk's error as the reference does (same test)
    for Q, C in ((1023, 1), (1025, 365), (2047, 3)):
        out.append(dict(name=f"boundary_Q{Q}_C{C}", ordinary=False, modes=MODES[:1] + MODES[2:],
                        problems=[_o2m_random(Q, Q, C, 5)]))
    return out


def nms_random_batch(seed, B, Q, C, bias, quant=None, spread=2.0):
    """tests/test_gpu_nms.py::_random_batch."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(bias, spread, (B, Q, C)).astype(F)
    if quant:
        logits = (np.round(logits * quant) / quant).astype(F)
    k = max(Q // 8, 1)
    cxcy = rng.random((B, Q, 2))
    wh = rng.random((B, Q, 2)) * 0.3 + 0.02
    for b in range(B):
        src = rng.integers(0, k, Q - k)
        cxcy[b, k:] = cxcy[b, src] + rng.normal(0, 0.01, (Q - k, 2))
        wh[b, k:] = wh[b, src] * (1 + rng.normal(0, 0.05, (Q - k, 2)))
    bbox = np.concatenate([cxcy, wh], -1).astype(F)
    shapes = [(int(rng.integers(400, 900)), int(rng.integers(500, 1400))) for _ in range(B)]
    return logits, bbox, shapes


def _nms(name, ordinary, logits, bbox, shapes, names=None, score_thr=0.01, iou_thr=0.6, max_per_img=300, iou_exact=False):
    return dict(name=name, ordinary=ordinary, logits=np.ascontiguousarray(logits, F), bbox=np.ascontiguousarray(bbox, F),
                shapes=shapes, names=names or [f"{name}[{b}]" for b in range(len(shapes))], score_thr=score_thr,
                iou_thr=iou_thr, max_per_img=max_per_img, iou_exact=iou_exact)


def nms_batches():
    out = [_nms("ordinary_5x900x80", True, *nms_random_batch(11, 5, 900, 80, -5.0))]
    # the adversarial family of the assigners, as teacher outputs (logits shifted down so that the threshold matters)
    probs = [p for p in adversarial_problems(48, 4, "logit", 5) if not p["name"].startswith("G")]
    out.append(_nms("adversarial_Q48_C4", False, np.stack([p["cls"] - 3 for p in probs]), np.stack([p["bbox_pred"] for p in probs]),
                    [(int(p["img_h"]), int(p["img_w"])) for p in probs], [p["name"] for p in probs]))
    # a score exactly at score_thr (sigmoid(0) = 0.5 in any precision; `>` is strict) among scores around it
    rng = np.random.default_rng(6)
    lg = np.round(rng.normal(0, 0.5, (2, 40, 3)) * 4) / 4
    out.append(_nms("score_at_threshold", False, lg, _boxes(rng, 80).reshape(2, 40, 4), [(480, 640)] * 2, score_thr=0.5))
    # IoU exactly at iou_threshold from power-of-two pixel sizes: [0,0,64,64] against [0,0,64,32] is 2048 / 4096 = 0.5 with
    # every intermediate exact in fp32, class 0 (offset 0): `>` must keep both, without any allowance
    bx = np.asarray([[[0.25, 0.25, 0.5, 0.5], [0.25, 0.125, 0.5, 0.25], [0.75, 0.75, 0.25, 0.25]]], F)
    out.append(_nms("iou_at_threshold_exact", False, np.asarray([[[2.0], [1.0], [0.0]]], F), bx, [(128, 128)], iou_thr=0.5,
                    iou_exact=True))
    # candidate count = max_per_img - 1, max_per_img, max_per_img + 1: ten separated boxes, all candidates, all kept
    grid = np.asarray([[[0.05 + 0.1 * i, 0.5, 0.05, 0.05] for i in range(10)]], F)
    for m in (9, 10, 11):
        out.append(_nms(f"count_vs_max_per_img_{m}", False, np.linspace(1, 3, 10, dtype=F).reshape(1, 10, 1), grid, [(500, 500)],
                        max_per_img=m))
    # Q = 2049 is refused by the entry point ("at most 2048 queries", kept by test_nms_errors): 2047 is the last size below
    for Q, C in ((1023, 1), (1025, 2), (2047, 2), (7, 365)):
        out.append(_nms(f"boundary_Q{Q}_C{C}", False, *nms_random_batch(Q, 1, Q, C, -2.0)))
    return out


def filter_cases():
    """(name, ordinary, proposal (K, 5), labels (K,))."""
    rng = np.random.default_rng(8)

    def prop(K):
        xy = rng.random((K, 2)) * 500
        return np.concatenate([xy, xy + rng.random((K, 2)) * 200 + 4, np.sort(rng.random((K, 1)), 0)[::-1]], -1).astype(F)
    eq = prop(50); eq[:, 4] = 0.3                       # std = 0: the threshold is the common score, `>=` keeps all or none
    neg = prop(40); neg[::3, 2] = neg[::3, 0] - 5; neg[1::7, 3] = neg[1::7, 1]     # negative w, zero h
    out = [("K300", True, prop(300)), ("K57", True, prop(57)), ("all_equal", False, eq), ("K2", False, prop(2)),
           ("K2_equal", False, eq[:2]), ("K1", False, prop(1)), ("K0", False, prop(0)), ("negative_w_zero_h", False, neg)]
    return [(n, o, p, rng.integers(0, 80, len(p))) for n, o, p in out]


def transform_cases():
    """(name, boxes (K, 4), M (3, 3), (out_h, out_w)): scale + flip, rotations, a mild perspective, boxes past the border."""
    rng = np.random.default_rng(9)
    out = []
    for i, (ang, persp) in enumerate(((0.0, 0.0), (0.3, 0.0), (-1.2, 0.0), (0.2, 1e-4))):
        xy = rng.random((60, 2)) * [600, 400] - 50
        b = np.concatenate([xy, xy + rng.random((60, 2)) * 200], -1).astype(F)
        b[::10, 2:] = b[::10, :2]                          # zero-area boxes
        c, s = np.cos(ang), np.sin(ang)
        M = np.asarray([[0.8 * c * (-1 if i == 0 else 1), -0.8 * s, 300.0 * (i == 0) + 20], [0.8 * s, 0.8 * c, 5.0],
                        [persp, -persp, 1.0]], F)
        out.append((f"warp{i}", b, M, (400, 600)))
    return out

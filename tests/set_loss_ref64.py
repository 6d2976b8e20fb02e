"""numpy float64 restatement of the set-prediction losses of ``csrc/set_loss.hip`` (DINODETRSSODHead.loss_single /
loss_single_dn, dino_detr_ssod_head.py:626-883, with mmdet py_sigmoid_focal_loss, L1Loss, GIoULoss and the warm-up
task-aligned focal loss), values and gradients, for checking the kernels at shapes no fixture can hold.

``segment_stats`` returns, per layer, the ten raw statistics the kernel reduces (cls sum, L1 sum / xy / hw, GIoU sum,
positive rows, rows with sum w > 0, rows with any w > 0, sum of the positives' w_0, sum of the metrics);
``finalize`` turns them into the five losses and the backward scales exactly as the kernel's finalize does;
``segment_grads`` gives d (sum_k coef_k * term_k) / d logits and / d boxes.
"""
import numpy as np

MATCHED, DN, WARMUP = 0, 1, 2


def dn_targets(gt_bboxes, gt_labels, single_pad, groups, img_wh, num_classes):
    """_get_target_single_dn (dino_detr_ssod_head.py:885-960) for every image -> labels (B,Q), label_weights (B,Q),
    bbox_targets (B,Q,4), bbox_weights (B,Q,4)."""
    B, Q = len(gt_bboxes), single_pad * groups
    labels = np.full((B, Q), num_classes, np.int64)
    lw = np.zeros((B, Q))
    tg = np.zeros((B, Q, 4))
    bw = np.zeros((B, Q, 4))
    for b in range(B):
        g = np.asarray(gt_bboxes[b], np.float64).reshape(-1, 4)
        G = g.shape[0]
        if G == 0:
            continue
        lw[b] = 1.0
        w, h = img_wh[b]
        n = g / np.array([w, h, w, h])
        cxcywh = np.stack([(n[:, 0] + n[:, 2]) / 2, (n[:, 1] + n[:, 3]) / 2, n[:, 2] - n[:, 0], n[:, 3] - n[:, 1]], -1)
        for k in range(groups):
            rows = k * single_pad + np.arange(G)
            labels[b, rows] = np.asarray(gt_labels[b]).reshape(-1)
            tg[b, rows] = cxcywh
            bw[b, rows] = 1.0
    return labels, lw, tg, bw


def _focal(x, t, alpha, gamma):
    z = np.where(t, -x, x)
    a = np.where(t, alpha, 1.0 - alpha)
    ez = np.exp(-np.abs(z))
    s = np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))
    oms = np.where(z >= 0, ez / (1.0 + ez), 1.0 / (1.0 + ez))
    sp = np.maximum(z, 0.0) + np.log1p(ez)
    sg = s ** gamma
    dz = a * sg * (gamma * oms * sp + s)
    return a * sg * sp, np.where(t, -dz, dz)


def _tal(x, st, gamma):
    p = 1.0 / (1.0 + np.exp(-x))
    with np.errstate(divide="ignore"):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log(1.0 - p), -100.0)
    ce = -(st * lp + (1.0 - st) * l1p)
    d = st - p
    mod = np.abs(d) ** gamma
    dmod = -gamma * np.abs(d) ** (gamma - 1.0) * np.sign(d) if gamma != 2.0 else -2.0 * d
    dce = (p - st) / np.maximum((1.0 - p) * p, 1e-12)
    return mod * ce, (dmod * ce + mod * dce) * (p * (1.0 - p))


def _xyxy(b, f):
    return np.stack([(b[..., 0] - 0.5 * b[..., 2]) * f[..., 0], (b[..., 1] - 0.5 * b[..., 3]) * f[..., 1],
                     (b[..., 0] + 0.5 * b[..., 2]) * f[..., 0], (b[..., 1] + 0.5 * b[..., 3]) * f[..., 1]], -1)


def _dmax(a, b):
    return np.where(a > b, 1.0, np.where(a == b, 0.5, 0.0))


def giou(b, tg, f, eps):
    """1 - giou per row (bbox_overlaps mode='giou', is_aligned) and d/d b (cxcywh), torch's max/min tie rule."""
    p, g = _xyxy(b, f), _xyxy(tg, f)
    a1 = (p[..., 2] - p[..., 0]) * (p[..., 3] - p[..., 1])
    a2 = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
    lt, rb = np.maximum(p[..., :2], g[..., :2]), np.minimum(p[..., 2:], g[..., 2:])
    wh = np.maximum(rb - lt, 0.0)
    elt, erb = np.minimum(p[..., :2], g[..., :2]), np.maximum(p[..., 2:], g[..., 2:])
    ewh = np.maximum(erb - elt, 0.0)
    ov = wh[..., 0] * wh[..., 1]
    uraw = a1 + a2 - ov
    u = np.maximum(uraw, eps)
    eraw = ewh[..., 0] * ewh[..., 1]
    e = np.maximum(eraw, eps)
    loss = 1.0 - (ov / u - (e - u) / e)
    dU = (ov / (u * u) - 1.0 / e) * _dmax(uraw, eps)
    dE = (u / (e * e)) * _dmax(eraw, eps)
    dO = -1.0 / u - dU
    dp = np.zeros(p.shape)
    dp[..., 2] += dU * (p[..., 3] - p[..., 1]); dp[..., 0] -= dU * (p[..., 3] - p[..., 1])
    dp[..., 3] += dU * (p[..., 2] - p[..., 0]); dp[..., 1] -= dU * (p[..., 2] - p[..., 0])
    for k in range(2):
        dwh = dO * wh[..., 1 - k] * (rb[..., k] - lt[..., k] >= 0)
        dp[..., k + 2] += dwh * _dmax(g[..., k + 2], p[..., k + 2])
        dp[..., k] -= dwh * _dmax(p[..., k], g[..., k])
        dewh = dE * ewh[..., 1 - k] * (erb[..., k] - elt[..., k] >= 0)
        dp[..., k + 2] += dewh * _dmax(p[..., k + 2], g[..., k + 2])
        dp[..., k] -= dewh * _dmax(g[..., k], p[..., k])
    ff = np.concatenate([f, f], -1)
    dp = dp * ff
    db = np.stack([dp[..., 0] + dp[..., 2], dp[..., 1] + dp[..., 3], 0.5 * (dp[..., 2] - dp[..., 0]),
                   0.5 * (dp[..., 3] - dp[..., 1])], -1)
    return loss, db


def _rows(kind, labels, label_weights, bbox_targets, bbox_weights, metrics, C):
    labels = np.asarray(labels)
    pos = (labels >= 0) & (labels < C)
    if kind == WARMUP:
        lw = np.asarray(metrics, np.float64)
        bw = np.asarray(bbox_weights, np.float64) * pos[..., None]
    else:
        lw = np.ones(labels.shape) if label_weights is None else np.asarray(label_weights, np.float64)
        bw = np.asarray(bbox_weights, np.float64)
    return labels, pos, lw, np.asarray(bbox_targets, np.float64), bw


def segment(kind, cls, boxes, labels, label_weights, bbox_targets, bbox_weights, img_wh, metrics=None, alpha=0.25,
            gamma=2.0, eps=1e-6, coef=None):
    """One segment: cls (nl,B,Q,C), boxes (nl,B,Q,4) (fp32 inputs, evaluated in fp64), targets (nl,B,Q[,4]) (dn:
    broadcast the dn_targets over the layers).  Returns stats (nl, 10) and, with ``coef`` (nl, 5) = upstream grad x scale
    per term, the gradients (d cls, d boxes)."""
    x = np.asarray(cls, np.float64)
    b = np.asarray(boxes, np.float64)
    nl, B, Q, C = x.shape
    labels, pos, lw, tg, bw = _rows(kind, labels, label_weights, bbox_targets, bbox_weights, metrics, C)
    onehot = labels[..., None] == np.arange(C)
    if kind == WARMUP:
        lc, dlc = _tal(x, np.where(onehot, lw[..., None], 0.0), gamma)
    else:
        lc, dlc = _focal(x, onehot, alpha, gamma)
        lc, dlc = lc * lw[..., None], dlc * lw[..., None]
    f = np.broadcast_to(np.asarray(img_wh, np.float64)[None, :, None, :], (nl, B, Q, 2))
    d = b - tg
    l1 = np.abs(d) * bw
    wm = bw.sum(-1) / 4.0
    gl, gdb = giou(b, tg, f, eps)
    st = np.zeros((nl, 10))
    red = (1, 2)
    st[:, 0] = lc.sum((1, 2, 3))
    st[:, 1] = l1.sum((1, 2, 3))
    st[:, 2] = l1[..., :2].sum((1, 2, 3))
    st[:, 3] = l1[..., 2:].sum((1, 2, 3))
    st[:, 4] = np.where(wm != 0, gl * wm, 0.0).sum(red)
    st[:, 5] = pos.sum(red)
    st[:, 6] = (bw.sum(-1) > 0).sum(red)
    st[:, 7] = (bw > 0).any(-1).sum(red)
    st[:, 8] = np.where(pos, bw[..., 0], 0.0).sum(red)
    st[:, 9] = lw.sum(red) if kind == WARMUP else 0.0
    if coef is None:
        return st
    c = np.asarray(coef, np.float64)[:, None, None, :]
    gx = dlc * c[..., 0:1]
    sg = np.sign(d) * bw
    gb = sg * (c[..., 1:2] + np.concatenate([c[..., 3:4], c[..., 3:4], c[..., 4:5], c[..., 4:5]], -1))
    gb = gb + np.where((wm != 0)[..., None], gdb * (wm[..., None] * c[..., 2:3]), 0.0)
    return st, gx, gb


def norm_inputs(kind, st, rows, bg_cls_weight=0.0):
    """(cls, reg) normaliser inputs before any cross-rank mean, per layer."""
    if kind == WARMUP:
        return np.stack([st[:, 9], st[:, 8]], -1)
    if kind == DN:
        return np.stack([st[:, 5] + st[:, 5] * bg_cls_weight, st[:, 5]], -1)
    return np.stack([st[:, 5] + (rows - st[:, 5]) * bg_cls_weight, st[:, 6]], -1)


def finalize(kind, st, norms, cls_weight, l1_weight, iou_weight):
    """losses (nl, 5) in the order cls, bbox, iou, bbox_xy, bbox_hw and the scales (nl, 5) the backward uses."""
    ncls, nreg = np.maximum(norms[:, 0], 1.0), np.maximum(norms[:, 1], 1.0)
    sc = np.stack([cls_weight / ncls, l1_weight / nreg, np.where(st[:, 7] > 0, iou_weight / nreg, 0.0),
                   l1_weight / nreg, l1_weight / nreg], -1)
    sums = np.stack([st[:, 0], st[:, 1], st[:, 4], st[:, 2], st[:, 3]], -1)
    return sums * sc, sc

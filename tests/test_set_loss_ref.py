"""CPU: the float64 restatement of the set-prediction losses (tests/set_loss_ref64.py) against a torch float64
autograd composition that follows the reference's own op sequence: mmdet ``py_sigmoid_focal_loss`` (focal_loss.py:12-57),
``weight_reduce_loss``, ``l1_loss``, ``GIoULoss`` + ``bbox_overlaps(mode='giou', is_aligned=True)`` and
``bbox_cxcywh_to_xyxy`` as ``loss_single`` / ``loss_single_dn`` call them (dino_detr_ssod_head.py:626-883), plus the
warm-up ``task_aigned_focal_loss``.  Values and gradients agree to 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import set_loss_ref64 as R


def _focal_torch(pred, labels, weight, alpha, gamma):
    C = pred.shape[1]
    target = F.one_hot(labels, C + 1)[:, :C].type_as(pred)
    p = pred.sigmoid()
    pt = (1 - p) * target + p * (1 - target)
    fw = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * fw
    return (loss * weight.view(-1, 1)).sum()


def _tal_torch(pred, labels, metric, gamma):
    C = pred.shape[1]
    p = pred.sigmoid()
    s = F.one_hot(labels, C + 1)[:, :C].type_as(pred) * metric[:, None]
    return ((s - p).abs().pow(gamma) * F.binary_cross_entropy(p, s, reduction="none")).sum()


def _xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _giou_rows(p, g, eps):
    area1 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    area2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    lt, rb = torch.max(p[:, :2], g[:, :2]), torch.min(p[:, 2:], g[:, 2:])
    wh = (rb - lt).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    union = torch.max(area1 + area2 - ov, p.new_tensor([eps]))
    elt, erb = torch.min(p[:, :2], g[:, :2]), torch.max(p[:, 2:], g[:, 2:])
    ewh = (erb - elt).clamp(min=0)
    enc = torch.max(ewh[:, 0] * ewh[:, 1], p.new_tensor([eps]))
    return 1 - (ov / union - (enc - union) / enc)


def _layer_torch(kind, x, b, labels, lw, tg, bw, wh, metrics, alpha, gamma, eps):
    """raw sums of one layer (cls, l1, l1 xy, l1 hw, giou) as loss_single computes them before the normalisers"""
    B, Q, C = x.shape
    xr, br = x.reshape(-1, C), b.reshape(-1, 4)
    lab = labels.reshape(-1)
    if kind == R.WARMUP:
        cls = _tal_torch(xr, lab, metrics.reshape(-1), gamma)
        pos = ((lab >= 0) & (lab < C)).to(x.dtype)
        bw = bw * pos.view(B, Q, 1)
    else:
        cls = _focal_torch(xr, lab, lw.reshape(-1), alpha, gamma)
    bwr, tgr = bw.reshape(-1, 4), tg.reshape(-1, 4)
    f = wh[:, None, :].repeat(1, Q, 2).reshape(-1, 4)
    l1 = (br - tgr).abs() * bwr
    if not torch.any(bwr > 0):
        gi = (br * bwr).sum()
    else:
        gi = (_giou_rows(_xyxy(br) * f, _xyxy(tgr) * f, eps) * bwr.mean(-1)).sum()
    return torch.stack([cls, l1.sum(), l1[:, :2].sum(), l1[:, 2:].sum(), gi])


def _case(seed, kind, nl=2, B=3, Q=17, C=80, zero_layer=None, big=30.0):
    r = np.random.default_rng(seed)
    x = (r.standard_normal((nl, B, Q, C)) * 3).astype(np.float32)
    x[0, 0, 0, :4] = [big, -big, 0.5 * big, -0.5 * big]
    b = np.concatenate([r.random((nl, B, Q, 2)), r.random((nl, B, Q, 2)) * 0.4 + 0.02], -1).astype(np.float32)
    wh = np.array([[640.0, 480.0], [1333.0, 800.0], [512.0, 512.0]])[:B]
    labels = np.where(r.random((nl, B, Q)) < 0.3, r.integers(0, C, (nl, B, Q)), C)
    lw = np.ones((nl, B, Q))
    tg = np.concatenate([r.random((nl, B, Q, 2)), r.random((nl, B, Q, 2)) * 0.4 + 0.02], -1) * (labels < C)[..., None]
    bw = np.repeat((labels < C)[..., None], 4, -1).astype(np.float64)
    metrics = None
    if kind == R.WARMUP:
        metrics = r.random((nl, B, Q)) * (labels < C)
        bw = bw * metrics[..., None]
    if zero_layer is not None:
        bw[zero_layer] = 0.0
    return dict(x=x, b=b, wh=wh, labels=labels, lw=lw, tg=tg, bw=bw, metrics=metrics)


@pytest.mark.parametrize("kind,zero", [(R.MATCHED, None), (R.MATCHED, 1), (R.WARMUP, None)])
def test_ref64_matches_torch_composition(kind, zero):
    c = _case(3 + kind, kind, zero_layer=zero)
    nl = c["x"].shape[0]
    coef = np.random.default_rng(9).random((nl, 5)) + 0.5
    st, gx, gb = R.segment(kind, c["x"], c["b"], c["labels"], c["lw"], c["tg"], c["bw"], c["wh"], metrics=c["metrics"],
                           coef=coef)
    x = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(c["b"].astype(np.float64)).requires_grad_(True)
    tot = 0
    for i in range(nl):
        m = None if c["metrics"] is None else torch.from_numpy(c["metrics"][i])
        sums = _layer_torch(kind, x[i], b[i], torch.from_numpy(c["labels"][i]), torch.from_numpy(c["lw"][i]),
                            torch.from_numpy(c["tg"][i]), torch.from_numpy(c["bw"][i]), torch.from_numpy(c["wh"]), m,
                            0.25, 2.0, 1e-6)
        np.testing.assert_allclose(st[i, :5], sums.detach().numpy(), rtol=1e-12, atol=1e-300)
        tot = tot + (sums * torch.from_numpy(coef[i])[[0, 1, 3, 4, 2]]).sum()
    tot.backward()
    # TAL: at |x| = 30, 1 - sigmoid(x) ~ 1e-13 keeps only ~3 significant digits in fp64 on either side
    atol = (1e-9 if kind == R.WARMUP else 1e-12) * np.abs(gx).max()
    np.testing.assert_allclose(gx, x.grad.numpy(), rtol=1e-12, atol=atol)
    np.testing.assert_allclose(gb, b.grad.numpy(), rtol=1e-12, atol=1e-12 * np.abs(gb).max())
    if zero is not None:
        assert st[zero, 7] == 0 and st[zero, 4] == 0


def test_dn_targets_follow_get_target_single_dn():
    gts = [np.array([[10.0, 20.0, 110.0, 220.0], [0.0, 0.0, 5.0, 5.0]]), np.zeros((0, 4))]
    labs = [np.array([3, 7]), np.zeros(0, np.int64)]
    lab, lw, tg, bw = R.dn_targets(gts, labs, 6, 2, [(200.0, 400.0), (100.0, 100.0)], 80)
    assert lab.shape == (2, 12) and list(lab[0, [0, 1, 6, 7]]) == [3, 7, 3, 7] and (lab[0, [2, 3, 4, 5, 8]] == 80).all()
    assert (lab[1] == 80).all() and (lw[1] == 0).all() and (lw[0] == 1).all()
    np.testing.assert_allclose(tg[0, 6], [0.3, 0.3, 0.5, 0.5])
    assert bw[0, :, 0].sum() == 4 and bw[1].sum() == 0


def test_finalize_normalisers():
    st = np.zeros((2, 10))
    st[:, 0], st[:, 1], st[:, 5], st[:, 6], st[:, 7] = 8.0, 6.0, 4.0, 3.0, [3.0, 0.0]
    st[:, 4] = 5.0
    n = R.norm_inputs(R.MATCHED, st, rows=100, bg_cls_weight=0.1)
    np.testing.assert_allclose(n, [[4 + 96 * 0.1, 3], [4 + 96 * 0.1, 3]])
    losses, sc = R.finalize(R.MATCHED, st, n, 2.0, 5.0, 2.0)
    np.testing.assert_allclose(losses[0], [8 * 2 / 13.6, 6 * 5 / 3, 5 * 2 / 3, 0, 0])
    assert losses[1, 2] == 0 and sc[1, 2] == 0                 # GIoULoss: no weight > 0 -> 0
    np.testing.assert_allclose(R.norm_inputs(R.DN, st, rows=100, bg_cls_weight=0.5)[0], [6.0, 4.0])

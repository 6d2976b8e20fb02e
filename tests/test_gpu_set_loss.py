"""GPU: the set-prediction loss kernels (csrc/set_loss.hip) against the float64 restatement tests/set_loss_ref64.py --
every segment kind at small shapes (logits up to +-30, an image without ground truth, Q < G, a layer whose bbox weights
are all zero), SSOD bench shapes, bitwise determinism, ``loss_set`` end to end with no host sync, and ``FocalLoss``.

Tolerances.  Values: each term is a sum of fp32-evaluated elements accumulated in fp64, so its relative error is that of
one element, a few fp32 ulps (3e-6 x max(|ref|, 1e-3) as test_gpu_tal.py).  Gradients: rtol 3e-5, atol 3e-6 x max|g| for
the logits; the box gradients carry the GIoU's image-scale differences (x2 - x1 of coordinates up to ~1333 px for boxes
down to 2% of the image), whose fp32 rounding is ~50 u relative: atol 2e-5 x max|g|."""
# These tolerances are kept as the older estimates; the derived per-element bounds are in tests/test_gpu_loss_admissible.py.
import numpy as np
import pytest
import torch

import set_loss_ref64 as R

pytestmark = pytest.mark.gpu
WH = np.array([[640.0, 480.0], [1333.0, 800.0], [512.0, 512.0], [800.0, 1199.0]])


def _boxes(r, shape):
    return np.concatenate([r.random(shape + (2,)) * 0.8 + 0.1, r.random(shape + (2,)) * 0.4 + 0.02], -1).astype(np.float32)


def _gts(r, B, counts, wh, C):
    gts, labs = [], []
    for b in range(B):
        n = counts[b]
        c = _boxes(r, (n,)).astype(np.float64)
        w, h = wh[b]
        xyxy = np.stack([c[:, 0] - c[:, 2] / 2, c[:, 1] - c[:, 3] / 2, c[:, 0] + c[:, 2] / 2, c[:, 1] + c[:, 3] / 2], -1)
        gts.append((xyxy * [w, h, w, h]).astype(np.float32))
        labs.append(r.integers(0, C, n))
    return gts, labs


def _matched_targets(r, nl, B, Q, C, warm=False, zero_layer=None):
    labels = np.where(r.random((nl * B, Q)) < 0.2, r.integers(0, C, (nl * B, Q)), C)
    tg = _boxes(r, (nl * B, Q)) * (labels < C)[..., None]
    bw = np.repeat((labels < C)[..., None], 4, -1).astype(np.float32)
    lw = np.ones((nl * B, Q), np.float32)
    metrics = None
    if warm:
        metrics = (r.random((nl * B, Q)) * (labels < C)).astype(np.float32)
        bw = bw * metrics[..., None]
    if zero_layer is not None:
        bw[zero_layer * B:(zero_layer + 1) * B] = 0.0
    return dict(labels=labels, label_weights=lw, bbox_targets=tg.astype(np.float32), bbox_weights=bw, metrics=metrics)


def _problem(seed=0, nl=3, B=3, Q=60, C=80, nl_dn=3, single_pad=10, groups=4, warm=False, counts=None, scale=3.0):
    """One outputs tensor (nl, B, pad + Q, C) sliced into dn / matched parts as head.py:491-501 does."""
    r = np.random.default_rng(seed)
    pad = single_pad * groups
    out_cls = (r.standard_normal((nl, B, pad + Q, C)) * scale).astype(np.float32)
    if warm:
        # the task-aligned loss takes log(p), log(1 - p) of the fp32 sigmoid, as the reference does: past |x| ~ 8 the fp32
        # 1 - p keeps too few digits for an fp64 comparison, and past ~17 it is 0 and the log clamps at -100 by design
        out_cls = np.clip(out_cls * 0.5, -6.0, 6.0)
    else:
        out_cls[0, 0, pad, :4] = [30.0, -30.0, 15.0, -15.0]
    out_box = _boxes(r, (nl, B, pad + Q))
    enc_cls = (r.standard_normal((B, Q, C)) * scale).astype(np.float32)
    if warm:
        enc_cls = np.clip(enc_cls * 0.5, -6.0, 6.0)
    enc_box = _boxes(r, (B, Q))
    wh = WH[:B]
    counts = counts if counts is not None else [min(single_pad, 3 + 2 * b) for b in range(B)]
    gts, labs = _gts(r, B, counts, wh, C)
    mt = _matched_targets(r, nl + 1, B, Q, C, warm=warm, zero_layer=1)
    return dict(out_cls=out_cls, out_box=out_box, enc_cls=enc_cls, enc_box=enc_box, wh=wh, gts=gts, labs=labs, mt=mt,
                pad=pad, single_pad=single_pad, groups=groups, nl=nl, B=B, Q=Q, C=C, warm=warm)


P2 = dict(alpha=0.25, gamma=2.0, cls_weight=2.0, l1_weight=5.0, iou_weight=2.0, iou_eps=1e-6, bg_cls_weight=0.0)


def _segments(p, dev, params=P2):
    import semi_detr_amd as s
    from semi_detr_amd import set_loss as sl
    t = {k: (torch.from_numpy(np.asarray(v)).to(dev) if v is not None else None) for k, v in p["mt"].items()}
    cls = torch.from_numpy(p["out_cls"]).to(dev).requires_grad_(True)
    box = torch.from_numpy(p["out_box"]).to(dev).requires_grad_(True)
    ecls = torch.from_numpy(p["enc_cls"]).to(dev).requires_grad_(True)
    ebox = torch.from_numpy(p["enc_box"]).to(dev).requires_grad_(True)
    wh = torch.from_numpy(p["wh"]).to(dev, torch.float32)
    nl, B, pad = p["nl"], p["B"], p["pad"]
    kind = sl.WARMUP if p["warm"] else sl.MATCHED
    mp = dict(params)
    if p["warm"]:
        mp.pop("alpha")

    def matched(lo, hi, c, b):
        return s.SetLossSegment(kind, c, b, labels=t["labels"][lo:hi], label_weights=None if p["warm"] else
                                t["label_weights"][lo:hi], bbox_targets=t["bbox_targets"][lo:hi],
                                bbox_weights=t["bbox_weights"][lo:hi],
                                metrics=t["metrics"][lo:hi] if p["warm"] else None, img_wh=wh, **mp)

    segs = [matched(0, nl * B, cls[:, :, pad:], box[:, :, pad:]),
            matched(nl * B, (nl + 1) * B, ecls[None], ebox[None]),
            s.SetLossSegment(sl.DN, cls[:, :, :pad], box[:, :, :pad], gt_bboxes=[torch.from_numpy(g).to(dev) for g in p["gts"]],
                             gt_labels=[torch.from_numpy(g).to(dev) for g in p["labs"]], single_pad=p["single_pad"],
                             dn_groups=p["groups"], img_wh=wh, **params)]
    return segs, (cls, box, ecls, ebox)


def _reference(p, coef_of, params=P2):
    """per-segment (losses, scales, d cls, d box) from set_loss_ref64; coef_of(T index range) -> upstream grads"""
    nl, B, Q, C, pad = p["nl"], p["B"], p["Q"], p["C"], p["pad"]
    kind = R.WARMUP if p["warm"] else R.MATCHED
    mt = p["mt"]
    sh = lambda a, n, q: a.reshape((n, B, q) + a.shape[2:])  # noqa: E731
    res = []
    cw = params["cls_weight"]
    parts = [(kind, p["out_cls"][:, :, pad:], p["out_box"][:, :, pad:], slice(0, nl * B), nl),
             (kind, p["enc_cls"][None], p["enc_box"][None], slice(nl * B, (nl + 1) * B), 1)]
    t0 = 0
    for kd, x, b, sl_, n in parts:
        m = None if mt["metrics"] is None else sh(mt["metrics"][sl_], n, Q)
        args = (kd, x, b, sh(mt["labels"][sl_], n, Q), None if p["warm"] else sh(mt["label_weights"][sl_], n, Q),
                sh(mt["bbox_targets"][sl_], n, Q), sh(mt["bbox_weights"][sl_], n, Q), p["wh"])
        st = R.segment(*args, metrics=m, alpha=params["alpha"], gamma=params["gamma"], eps=params["iou_eps"])
        losses, sc = R.finalize(kd, st, R.norm_inputs(kd, st, B * Q, params["bg_cls_weight"]), cw, params["l1_weight"],
                                params["iou_weight"])
        _, gx, gb = R.segment(*args, metrics=m, alpha=params["alpha"], gamma=params["gamma"], eps=params["iou_eps"],
                              coef=sc * coef_of(t0, n))
        res.append((losses, sc, gx, gb))
        t0 += n
    lab, lw, tg, bw = R.dn_targets(p["gts"], p["labs"], p["single_pad"], p["groups"], p["wh"], C)
    rep = lambda a: np.broadcast_to(a, (nl,) + a.shape)  # noqa: E731
    args = (R.DN, p["out_cls"][:, :, :pad], p["out_box"][:, :, :pad], rep(lab), rep(lw), rep(tg), rep(bw), p["wh"])
    st = R.segment(*args, alpha=params["alpha"], gamma=params["gamma"], eps=params["iou_eps"])
    losses, sc = R.finalize(R.DN, st, R.norm_inputs(R.DN, st, B * pad, params["bg_cls_weight"]), cw,
                            params["l1_weight"], params["iou_weight"])
    _, gx, gb = R.segment(*args, alpha=params["alpha"], gamma=params["gamma"], eps=params["iou_eps"],
                          coef=sc * coef_of(t0, nl))
    res.append((losses, sc, gx, gb))
    return res


def _check_values(got, ref, tol=3e-6):
    got = np.asarray(got, np.float64)
    bad = np.abs(got - ref) > tol * np.maximum(np.abs(ref), 1e-3)
    assert not bad.any(), (got[bad], ref[bad])


def _run_and_check(p, box_atol=2e-5, val_tol=3e-6):
    import semi_detr_amd as s
    dev = torch.device("cuda")
    segs, (cls, box, ecls, ebox) = _segments(p, dev)
    info = {}
    terms = s.set_losses(segs, info=info)
    T = len(terms)
    coef = np.random.default_rng(1).random((T, 5)) + 0.5
    tot = sum((t * float(c)) for row, cr in zip(terms, coef) for t, c in zip(row, cr))
    tot.backward()
    got = torch.stack([torch.stack(r) for r in terms]).detach().cpu().numpy()
    ref = _reference(p, lambda t0, n: coef[t0:t0 + n])
    nl, pad = p["nl"], p["pad"]
    _check_values(got[:nl], ref[0][0], val_tol)
    _check_values(got[nl:nl + 1], ref[1][0], val_tol)
    _check_values(got[nl + 1:], ref[2][0], val_tol)
    # gradients: the matched and dn slices of one outputs tensor, and the encoder's
    gcls, gbox = cls.grad.cpu().numpy(), box.grad.cpu().numpy()
    for g, r_, atol in ((gcls[:, :, pad:], ref[0][2], 3e-6), (gcls[:, :, :pad], ref[2][2], 3e-6),
                        (ecls.grad.cpu().numpy()[None], ref[1][2], 3e-6), (gbox[:, :, pad:], ref[0][3], box_atol),
                        (gbox[:, :, :pad], ref[2][3], box_atol), (ebox.grad.cpu().numpy()[None], ref[1][3], box_atol)):
        np.testing.assert_allclose(g, r_, rtol=3e-5, atol=atol * max(np.abs(r_).max(), 1e-30))
    return info


@pytest.mark.parametrize("warm", [False, True])
def test_kernel_matches_ref64_small(warm):
    # image 2 has no ground truth (dn label_weights = 0), layer 1 has all-zero bbox weights (GIoULoss's early return)
    p = _problem(seed=4 + warm, warm=warm, counts=[3, 10, 0])
    info = _run_and_check(p)
    st = info["stats"].cpu().numpy()
    assert st[1, 7] == 0 and info["losses"][1, 2].item() == 0.0


def test_kernel_unaligned_strides_take_the_scalar_path():
    p = _problem(seed=11, nl=2, B=2, Q=37, C=7, single_pad=6, groups=3, counts=[6, 2])
    _run_and_check(p)


@pytest.mark.parametrize("B", [4, 1])
def test_bench_shapes_match_ref64(B):
    # SSOD unsup (B 4) and sup (B 1): 6 decoder layers + encoder, Q 900, C 80, dn pad 200 (10 groups of 20)
    p = _problem(seed=20 + B, nl=6, B=B, Q=900, C=80, single_pad=20, groups=10,
                 counts=[min(10, 2 + 3 * b) for b in range(B)], scale=2.0)
    _run_and_check(p, val_tol=1e-5)


def test_determinism_bitwise():
    import semi_detr_amd as s
    p = _problem(seed=7, nl=6, B=4, Q=900, single_pad=20, groups=10, counts=[10, 4, 0, 7])
    outs = []
    for _ in range(2):
        segs, ins = _segments(p, torch.device("cuda"))
        terms = s.set_losses(segs)
        sum(t for row in terms for t in row).backward()
        outs.append([torch.stack([torch.stack(r) for r in terms]).detach().cpu()] + [x.grad.cpu() for x in ins])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


class _L:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _head(warm=False):
    from semi_detr_amd import TargetAssigner
    h = TargetAssigner(num_classes=80, in_warm_up=warm)
    h.loss_cls1 = _L(gamma=2.0, loss_weight=2.0)
    h.loss_cls2 = _L(gamma=2.0, alpha=0.25, loss_weight=2.0)
    h.loss_bbox = _L(loss_weight=5.0)
    h.loss_iou = _L(loss_weight=2.0, eps=1e-6)
    h.bg_cls_weight, h.sync_cls_avg_factor = 0.0, False
    return h


def _e2e_inputs(seed, nl=6, B=2, Q=300, C=80, single_pad=20, groups=5):
    r = np.random.default_rng(seed)
    pad = single_pad * groups
    dev = torch.device("cuda")
    out_cls = torch.from_numpy((r.standard_normal((nl, B, pad + Q, C)) * 2).astype(np.float32)).to(dev)
    out_box = torch.from_numpy(_boxes(r, (nl, B, pad + Q))).to(dev)
    enc_cls = torch.from_numpy((r.standard_normal((B, Q, C)) * 2).astype(np.float32)).to(dev)
    enc_box = torch.from_numpy(_boxes(r, (B, Q))).to(dev)
    counts = [7, 0][:B] if B == 2 else [5] * B
    gts, labs = _gts(r, B, counts, WH[:B], C)
    metas = [dict(img_shape=(int(WH[b][1]), int(WH[b][0]), 3)) for b in range(B)]
    dn_meta = dict(num_dn_group=groups, pad_size=pad, num_dn_group_2=groups, pad_size_2=pad)
    for t in (out_cls, out_box, enc_cls, enc_box):
        t.requires_grad_(True)
    return dict(out_cls=out_cls, out_box=out_box, enc_cls=enc_cls, enc_box=enc_box, pad=pad, metas=metas, dn_meta=dn_meta,
                gts=[torch.from_numpy(g).to(dev) for g in gts], labs=[torch.from_numpy(g).to(dev) for g in labs])


def _call_loss(h, d, is_pseudo_label=False):
    import semi_detr_amd as s
    pad = d["pad"]
    return s.loss_set(h, d["out_cls"][:, :, pad:], d["out_box"][:, :, pad:], d["enc_cls"], d["enc_box"],
                      d["out_cls"][:, :, :pad], d["out_box"][:, :, :pad], d["gts"], d["labs"], None, d["metas"],
                      d["dn_meta"], None, is_pseudo_label)


def _keys(nl):
    ks = []
    terms = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
    ks += ["enc_" + k for k in terms] + list(terms) + ["dn_" + k for k in terms]
    for i in range(nl - 1):
        ks += [f"d{i}.{k}" for k in terms] + [f"d{i}.dn_{k}" for k in terms]
    return ks


def test_loss_set_end_to_end_matches_ref64_and_does_not_sync():
    from semi_detr_amd.targets import _targets_stacked
    h = _head()
    d = _e2e_inputs(3)
    nl, B, pad = 6, 2, d["pad"]
    Q, C = d["out_cls"].shape[2] - pad, 80
    # the targets loss_set will use: one batch of (nl + 1) x B problems, encoder labels all zero
    cls_t = torch.cat([d["out_cls"].detach()[:, :, pad:].reshape(nl * B, Q, C), d["enc_cls"].detach()])
    box_t = torch.cat([d["out_box"].detach()[:, :, pad:].reshape(nl * B, Q, 4), d["enc_box"].detach()])
    t = _targets_stacked(h, cls_t, box_t, d["gts"] * nl + d["gts"], d["labs"] * nl + [torch.zeros_like(l) for l in d["labs"]],
                         d["metas"] * (nl + 1), check=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = _call_loss(h, d)
        tot = sum(out.values())
        tot.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert list(out) == _keys(nl)
    p = dict(out_cls=d["out_cls"].detach().cpu().numpy(), out_box=d["out_box"].detach().cpu().numpy(),
             enc_cls=d["enc_cls"].detach().cpu().numpy(), enc_box=d["enc_box"].detach().cpu().numpy(), wh=WH[:B],
             gts=[g.cpu().numpy() for g in d["gts"]], labs=[g.cpu().numpy() for g in d["labs"]],
             mt=dict(labels=t["labels"].cpu().numpy(), label_weights=t["label_weights"].cpu().numpy(),
                     bbox_targets=t["bbox_targets"].cpu().numpy(), bbox_weights=t["bbox_weights"].cpu().numpy(),
                     metrics=None), pad=pad, single_pad=20, groups=5, nl=nl, B=B, Q=Q, C=C, warm=False)
    ref = _reference(p, lambda t0, n: np.ones((n, 5)))
    names = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
    for k, v in zip(names, ref[1][0][0]):
        assert abs(out["enc_" + k].item() - v) <= 3e-6 * max(abs(v), 1e-3), k
    for i in range(nl):
        pre = "" if i == nl - 1 else f"d{i}."
        for k, v, vd in zip(names, ref[0][0][i], ref[2][0][i]):
            assert abs(out[pre + k].item() - v) <= 3e-6 * max(abs(v), 1e-3), pre + k
            assert abs(out[pre + "dn_" + k].item() - vd) <= 3e-6 * max(abs(vd), 1e-3), pre + "dn_" + k
    g = d["out_cls"].grad.cpu().numpy()
    np.testing.assert_allclose(g[:, :, pad:], ref[0][2], rtol=3e-5, atol=3e-6 * np.abs(ref[0][2]).max())
    np.testing.assert_allclose(g[:, :, :pad], ref[2][2], rtol=3e-5, atol=3e-6 * np.abs(ref[2][2]).max())
    gb = d["out_box"].grad.cpu().numpy()
    np.testing.assert_allclose(gb[:, :, pad:], ref[0][3], rtol=3e-5, atol=2e-5 * np.abs(ref[0][3]).max())


def test_loss_set_warm_up_on_pseudo_labels_zeroes_dn():
    h = _head(warm=True)
    d = _e2e_inputs(5, nl=2, Q=120)
    out = _call_loss(h, d, is_pseudo_label=True)
    assert list(out) == _keys(2)
    assert all(out[k].item() == 0.0 for k in out if "dn_" in k)
    assert all(torch.isfinite(out[k]).item() for k in out)
    sum(out.values()).backward()
    assert torch.isfinite(d["out_cls"].grad).all() and torch.isfinite(d["out_box"].grad).all()


@pytest.mark.parametrize("weighted,avg", [(False, 7.0), (True, 7.0), (True, None), (False, None)])
def test_focal_loss_drop_in(weighted, avg):
    import semi_detr_amd as s
    r = np.random.default_rng(3)
    N, C = 300, 80
    x = (r.standard_normal((N, C)) * 4).astype(np.float32)
    x[0, :2] = [30.0, -30.0]
    lab = np.where(r.random(N) < 0.3, r.integers(0, C, N), C)
    w = r.random(N).astype(np.float32) if weighted else np.ones(N, np.float32)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    crit = s.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0)
    loss = crit(xt, torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda() if weighted else None, avg_factor=avg)
    loss.backward()
    z = np.zeros((1, 1, N, 4))
    st, gx, _ = R.segment(R.MATCHED, x[None, None], z, lab[None, None], w[None, None], z, z, WH[:1], coef=np.ones((1, 5)))
    div = avg if avg is not None else N * C
    ref = 2.0 * st[0, 0] / div
    assert abs(loss.item() - ref) <= 3e-6 * max(abs(ref), 1e-3)
    np.testing.assert_allclose(xt.grad.cpu().numpy(), 2.0 * gx[0, 0] / div, rtol=3e-5,
                               atol=3e-6 * np.abs(gx).max() * 2.0 / div)

"""GPU: the set-loss kernels against the reference's own ``loss()`` (tests/golden/set_loss.npz), through the kernel alone
on the stored targets and end to end through ``loss_set`` with this project's ``get_targets`` (after asserting that its
targets equal the stored ones).  Tolerances as tests/test_gpu_set_loss.py: values 3e-6 x max(|ref|, 1e-3); gradients
rtol 3e-5 with atol 3e-6 x max|g| for the logits and 2e-5 x max|g| for the boxes (the GIoU's image-scale differences).
The box VALUES get 3e-5: here the matched queries sit within ~0.004 of their targets (the cost margins the assignment
needs), so |b - t| and the GIoU's overlaps are differences of coordinates ~0.5 whose fp32 rounding (u x 0.5 ~ 3e-8, in
the targets as well as in the kernel) is ~1e-5 of the difference, and a loss over a handful of positive rows does not
average it away."""
import numpy as np
import pytest
import torch

import set_loss_fixture as F

pytestmark = pytest.mark.gpu


class _L:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _head(warm):
    from semi_detr_amd import TargetAssigner
    h = TargetAssigner(num_classes=80, in_warm_up=warm)
    h.loss_cls1 = _L(gamma=2.0, loss_weight=2.0)
    h.loss_cls2 = _L(gamma=2.0, alpha=0.25, loss_weight=2.0)
    h.loss_bbox, h.loss_iou = _L(loss_weight=5.0), _L(loss_weight=2.0, eps=1e-6)
    h.bg_cls_weight, h.sync_cls_avg_factor = 0.0, False
    return h


def _inputs(c):
    return [torch.from_numpy(c[k]).cuda().requires_grad_(True) for k in F.INPUTS]


def _check(c, values, ins):
    ref = c["values"]
    got = np.asarray(values, np.float64)
    tol = np.asarray([3e-5 if ("bbox" in k or "iou" in k) else 3e-6 for k in c["keys"]])
    bad = np.abs(got - ref) > tol * np.maximum(np.abs(ref), 1e-3)
    assert not bad.any(), [(k, g, r) for k, g, r, b in zip(c["keys"], got, ref, bad) if b]
    for k, t in zip(F.INPUTS, ins):
        want = c["grad_" + k]
        atol = (3e-6 if k.endswith("cls") else 2e-5) * max(np.abs(want).max(), 1e-30)
        np.testing.assert_allclose(t.grad.cpu().numpy(), want, rtol=3e-5, atol=atol, err_msg=k)


@pytest.mark.parametrize("name", F.NAMES)
def test_kernel_alone_matches_reference_fixture(name):
    import semi_detr_amd as s
    from semi_detr_amd import set_loss as sl
    c = F.case(name)
    nl, B = c["nl"], c["B"]
    ins = _inputs(c)
    dev = ins[0].device
    warm = bool(c["warm_up"])
    t = {k: torch.from_numpy(c[k]).to(dev) for k in ("labels", "label_weights", "bbox_targets", "bbox_weights")}
    if warm:
        t["norm_metrics"] = torch.from_numpy(c["norm_metrics"]).to(dev)
    wh = torch.from_numpy(c["wh"]).to(dev, torch.float32)
    common = dict(img_wh=wh, cls_weight=2.0, l1_weight=5.0, iou_weight=2.0)

    def matched(lo, hi, x, b):
        return s.SetLossSegment(sl.WARMUP if warm else sl.MATCHED, x, b, labels=t["labels"][lo:hi],
                                label_weights=None if warm else t["label_weights"][lo:hi],
                                bbox_targets=t["bbox_targets"][lo:hi], bbox_weights=t["bbox_weights"][lo:hi],
                                metrics=t["norm_metrics"][lo:hi] if warm else None, **common)

    segs = [matched(0, nl * B, ins[0], ins[1]), matched(nl * B, (nl + 1) * B, ins[2][None], ins[3][None]),
            s.SetLossSegment(sl.DN, ins[4], ins[5], gt_bboxes=[torch.from_numpy(g).to(dev) for g in c["gt_list"]],
                             gt_labels=[torch.from_numpy(g).to(dev) for g in c["lab_list"]],
                             single_pad=int(c["single_pad"]), dn_groups=int(c["groups"]), **common)]
    terms = s.set_losses(segs)
    rows = F.key_rows(c["keys"], nl)
    out = [terms[rows[k][0]][rows[k][1]] for k in c["keys"]]
    sum(float(cf) * v for cf, v in zip(c["coef"], out)).backward()
    _check(c, [v.item() for v in out], ins)


@pytest.mark.parametrize("name", F.NAMES)
def test_loss_set_end_to_end_matches_reference_fixture(name):
    import semi_detr_amd as s
    from semi_detr_amd.targets import _targets_stacked
    c = F.case(name)
    nl, B, Q = c["nl"], c["B"], c["Q"]
    warm = bool(c["warm_up"])
    h = _head(warm)
    ins = _inputs(c)
    gts = [torch.from_numpy(g).cuda() for g in c["gt_list"]]
    labs = [torch.from_numpy(g).cuda() for g in c["lab_list"]]
    metas = [dict(img_shape=(int(hw[0]), int(hw[1]), 3)) for hw in c["img_hw"]]
    pad = int(c["single_pad"]) * int(c["groups"])
    dn_meta = dict(num_dn_group=int(c["groups"]), pad_size=pad, num_dn_group_2=int(c["groups"]), pad_size_2=pad)
    # the targets loss_set builds equal the ones the reference's get_targets produced
    cls_t = torch.cat([ins[0].detach().reshape(nl * B, Q, -1), ins[2].detach()])
    box_t = torch.cat([ins[1].detach().reshape(nl * B, Q, 4), ins[3].detach()])
    t = _targets_stacked(h, cls_t, box_t, gts * nl + gts, labs * nl + [torch.zeros_like(x) for x in labs],
                         metas * (nl + 1), check=True)
    assert np.array_equal(t["labels"].cpu().numpy(), c["labels"])
    for k in ("bbox_targets", "bbox_weights") + (("norm_metrics",) if warm else ("label_weights",)):
        np.testing.assert_allclose(t[k].cpu().numpy(), c[k], rtol=2e-6, atol=1e-7, err_msg=k)
    out = s.loss_set(h, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], gts, labs, None, metas, dn_meta, None,
                     bool(c["is_pseudo_label"]))
    assert list(out) == c["keys"]
    sum(float(cf) * out[k] for cf, k in zip(c["coef"], c["keys"])).backward()
    _check(c, [out[k].item() for k in c["keys"]], ins)

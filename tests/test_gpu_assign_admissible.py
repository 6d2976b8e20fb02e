"""The decision kernels (match_cost + lsap, o2m, nms, pseudo_label, the box warp) against the fp64 statements of
tests/assign_ref64.py, through the public classes and their batched entry points: a result is ADMISSIBLE when every continuous
quantity is within its derived fp32 bound, every decision differs from the fp64 decision only where the fp64 margin is within
that bound, and the structural conditions (a matching, no two kept boxes of a class overlap, ...) hold with no allowance.
Ordinary batches are, as in the existing parity tests, also equal to the C oracle; adversarial ones (duplicates, degenerate
boxes, saturated logits, size boundaries, exact ties: tests/assign_cases.py says what each aims at) are admissible only.

With -s every test prints, per case, the worst err / bound of each continuous quantity and the number of decisions that used
their allowance."""
import numpy as np
import pytest
import torch

import assign_cases as ac
import assign_ref64 as ar
import oracle
from assign_cases import golden as _npz, h_inputs, o_inputs

pytestmark = pytest.mark.gpu

DINO_ASSIGNER = dict(cls_cost=dict(type="FocalLossCost", weight=2.0),
                     reg_cost=dict(type="BBoxL1Cost", weight=5.0, box_format="xywh"),
                     iou_cost=dict(type="IoUCost", iou_mode="giou", weight=2.0))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _meta(p):
    return dict(img_shape=(int(p["img_h"]), int(p["img_w"]), 3))


def _row(case, st):
    print(f"  {case:46s} " + " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in st.items()))


def _guard(case, fn):
    try:
        return fn()
    except ar.Inadmissible as e:
        raise AssertionError(f"{case}: {e}") from None


@pytest.mark.parametrize("batch", ac.hungarian_batches(), ids=lambda b: b["name"])
def test_hungarian_admissible(batch):
    from semi_detr_amd import HungarianAssigner
    ps = batch["problems"]
    asg = HungarianAssigner(**DINO_ASSIGNER)
    args = (_t(np.stack([p["bbox_pred"] for p in ps])), _t(np.stack([p["cls"] for p in ps])), [_t(p["gt_bboxes"]) for p in ps],
            [_t(p["gt_labels"]) for p in ps], [_meta(p) for p in ps])
    res, costs, _ = asg.assign_batch(*args, return_cost=True)
    tg = asg.get_targets_batch(*args, num_classes=ps[0]["cls"].shape[1])
    print(f"\n{batch['name']}")
    for b, p in enumerate(ps):
        gi, lab = res[b].gt_inds.cpu().numpy(), res[b].labels.cpu().numpy()
        cost = costs[b].cpu().numpy() if len(p["gt_labels"]) else None
        st = _guard(p["name"], lambda: ar.check_hungarian(h_inputs(p), gi, lab, cost, num_pos=int(tg["num_pos"][b])))
        assert np.array_equal(tg["gt_inds"][b].cpu().numpy(), gi), p["name"]
        _row(p["name"], st)
        if batch["ordinary"]:
            ogi, olab, _, _ = oracle.hungarian_assign(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"])
            assert np.array_equal(gi, ogi) and np.array_equal(lab, olab), p["name"]


def test_individual_costs_admissible_pred_xyxy_contract():
    """cls_cost / reg_cost / iou_cost called one by one (dino_detr_ssod.py:265-271): the second contract of the kernel, boxes
    handed over as x1 y1 x2 y2 and gts already normalised."""
    from semi_detr_amd import HungarianAssigner
    asg = HungarianAssigner(**DINO_ASSIGNER)
    print()
    for p in ac.ordinary_hungarian()[:2] + ac.adversarial_problems(48, 8, "logit", 1):
        if not len(p["gt_labels"]):
            continue
        f = np.asarray([p["img_w"], p["img_h"]] * 2, np.float32)
        b = p["bbox_pred"]
        xyxy = (np.concatenate([b[:, :2] - np.float32(0.5) * b[:, 2:], b[:, :2] + np.float32(0.5) * b[:, 2:]], -1) * f).astype(np.float32)
        ngt = (p["gt_bboxes"] / f).astype(np.float32)
        c1 = asg.cls_cost(_t(p["cls"]), _t(p["gt_labels"])).cpu().numpy()
        c2 = asg.reg_cost(_t(b), _t(ngt)).cpu().numpy()
        c3 = asg.iou_cost(_t(xyxy), _t(p["gt_bboxes"])).cpu().numpy()
        r1 = ar.match_cost(**h_inputs(p))["cls"]
        r2 = ar.match_cost(b, p["cls"], ngt, p["gt_labels"], 1.0, 1.0)["reg"]
        r3 = ar.match_cost(xyxy, p["cls"], p["gt_bboxes"], p["gt_labels"], 1.0, 1.0, pred_xyxy=True)["iou"]
        for key, got, ref in (("cls", c1, r1), ("reg", c2, r2), ("iou", c3, r3)):
            _guard(p["name"], lambda: ar._within(f"{key}_cost", got, ref))
        _row(p["name"], dict(cls_ratio=ar.ratio(c1, r1), reg_ratio=ar.ratio(c2, r2), iou_ratio=ar.ratio(c3, r3)))


@pytest.mark.parametrize("batch", ac.o2m_batches(), ids=lambda b: b["name"])
def test_o2m_admissible(batch):
    from semi_detr_amd import O2MAssigner
    ps = batch["problems"]
    C = ps[0]["cls"].shape[1]
    print(f"\n{batch['name']}")
    for mode, topk, dyn in batch["modes"]:
        out = O2MAssigner(candidate_topk=13).assign_batch(
            _t(np.stack([p["bbox_pred"] for p in ps])), _t(np.stack([p["cls"] for p in ps])), [_t(p["gt_bboxes"]) for p in ps],
            [_t(p["gt_labels"]) for p in ps], [_meta(p) for p in ps], candidate_topk=topk, dynamic_k=dyn)
        keys = ("gt_inds", "labels", "max_overlaps", "assign_metrics", "labels_full", "bbox_targets", "norm_metrics")
        for b, p in enumerate(ps):
            got = {k: out[k][b].cpu().numpy() for k in keys}
            st = _guard(f"{p['name']} / {mode}", lambda: ar.check_o2m(o_inputs(p), got, C, topk, dyn))
            _row(f"{p['name']} / {mode}", st)
            if batch["ordinary"]:
                gi, lab, mo, am = oracle.o2m_assign(p["bbox_pred"], p["cls"], p["gt_bboxes"], p["gt_labels"], p["img_w"], p["img_h"],
                                                    topk=topk, dynamic_k=dyn)
                assert np.array_equal(got["gt_inds"], gi) and np.array_equal(got["labels"], lab), (p["name"], mode)
                assert np.array_equal(got["max_overlaps"], mo) and np.array_equal(got["assign_metrics"], am), (p["name"], mode)


@pytest.mark.parametrize("nb", ac.nms_batches(), ids=lambda b: b["name"])
def test_teacher_pseudo_labels_admissible(nb):
    """Decode + NMS + top max_per_img, then the mean + std filter on what NMS returned, chained on the device."""
    from semi_detr_amd import teacher_pseudo_labels
    metas = [dict(img_shape=(h, w, 3)) for h, w in nb["shapes"]]
    boxes, labels, scores, props = teacher_pseudo_labels(_t(nb["logits"]), _t(nb["bbox"]), metas, score_thr=nb["score_thr"],
                                                         iou_threshold=nb["iou_thr"], max_per_img=nb["max_per_img"],
                                                         return_proposals=True)
    print(f"\n{nb['name']}")
    for b, (h, w) in enumerate(nb["shapes"]):
        dets, labs = props[b][0].cpu().numpy(), props[b][1].cpu().numpy()
        st = _guard(nb["names"][b], lambda: ar.check_nms(nb["logits"][b], nb["bbox"][b], h, w, dets, labs, nb["score_thr"],
                                                         nb["iou_thr"], nb["max_per_img"], iou_exact=nb["iou_exact"]))
        sf = _guard(nb["names"][b], lambda: ar.check_pseudo_filter(dets, labs, boxes[b].cpu().numpy(), labels[b].cpu().numpy(),
                                                                   scores[b].cpu().numpy()))
        st.update(filter_kept=sf["kept"], filter_used_allowance=sf["used_allowance"])
        _row(nb["names"][b], st)
        if nb["ordinary"]:
            od, ol = oracle.pseudo_nms(nb["logits"][b], nb["bbox"][b], h, w)
            assert np.array_equal(labs, ol) and np.array_equal(dets[:, :4], od[:, :4])
            keep, _ = oracle.pseudo_label_filter(od)
            assert np.array_equal(boxes[b].cpu().numpy(), od[keep, :4])
    if nb["name"] == "iou_at_threshold_exact":
        assert len(props[0][1]) == 3            # IoU == iou_threshold suppresses nothing: `>` is strict


def test_pseudo_filter_admissible():
    """All filter cases as one ragged launch, thresholds included (std = 0, K = 2, K = 1 -> NaN and nothing, K = 0)."""
    from semi_detr_amd import filter_pseudo_labels
    cases = ac.filter_cases()
    b, l, s, thr = filter_pseudo_labels([_t(p) for _, _, p, _ in cases], [_t(lab) for _, _, _, lab in cases], return_threshold=True)
    thr = thr.cpu().numpy()
    print()
    for i, (name, _, prop, lab) in enumerate(cases):
        st = _guard(name, lambda: ar.check_pseudo_filter(prop, lab, b[i].cpu().numpy(), l[i].cpu().numpy(), s[i].cpu().numpy(),
                                                         thr[i] if len(prop) else None))
        _row(name, st)
        if name in ("K1", "K0"):
            assert st["kept"] == 0


def test_transform_bboxes_derived_bound():
    """The warp against its derived bound (the atol of 5e-4 / 2e-4 in test_gpu_nms.py is a guess and stays there)."""
    from semi_detr_amd import transform_bboxes
    cases = [(n, g["boxes"][:, :4].copy(), g["M"], tuple(float(v) for v in g["out_shape"])) for n, g in _npz("transform.npz").items()
             if len(g["boxes"])] + ac.transform_cases()
    outs = transform_bboxes([_t(b) for _, b, _, _ in cases], [torch.from_numpy(M) for _, _, M, _ in cases],
                            [hw for _, _, _, hw in cases])
    print()
    for (name, boxes, M, (h, w)), out in zip(cases, outs):
        _row(name, _guard(name, lambda: ar.check_transform(boxes, M, h, w, out.cpu().numpy())))

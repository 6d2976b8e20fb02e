#!/usr/bin/env python
"""Generate tests/golden/set_loss.npz from the REFERENCE's own ``DINODETRSSODHead.loss`` / ``loss_single`` /
``loss_single_dn`` / ``get_targets`` / ``_get_target_single`` / ``get_targets_dn`` / ``_get_target_single_dn`` /
``prep_for_dn`` (detr_od/models/dense_heads/dino_detr_ssod_head.py:328-339, :508-1205), imported by path and run unbound
on a stand-in ``self``, with the vendored mmdet ``FocalLoss`` (its CPU path, ``py_sigmoid_focal_loss``), ``L1Loss``,
``GIoULoss``, ``bbox_overlaps``, ``PseudoSampler``, the reference's ``TaskAlignedFocalLoss`` and its
``HungarianAssigner`` / ``O2MAssigner`` (the DINO SSOD config's loss and assigner settings).  ``mmcv.jit`` /
``force_fp32`` are identity stubs, ``mmcv.ops`` a dummy (the CPU path never calls it), ``reduce_mean`` is mmdet's
single-process identity and ``.cuda()`` is the identity (the dn targets call it).  Runs where the reference tree and scipy
exist; what it writes is data.

    python tools/gen_set_loss_golden.py

Every case runs in float64 with autograd.  Stored per case ``<case>.``: the float32 inputs (``all_cls``, ``all_box``,
``enc_cls``, ``enc_box``, ``dn_cls``, ``dn_box``), the ground truths (``gt_boxes`` concatenated, ``gt_counts``,
``gt_labels``), ``img_hw``, the dn meta, the flags, the targets the reference's ``get_targets`` produced for the decoder
layers then the encoder (``labels`` / ``label_weights`` / ``bbox_targets`` / ``bbox_weights`` (+ ``norm_metrics`` in
warm-up), stacked over (nl + 1) x B problems), the loss dict (``keys`` in order, ``values`` float64) and the float64
gradients of ``sum_k coef_k * loss_k`` w.r.t. the six inputs (``coef`` stored).
"""
import functools
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF, _load, load_hungarian_assigner  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "set_loss.npz")
MMD = REF + "/thirdparty/mmdetection/mmdet"


class _Reg:
    def __init__(self, *a, **k):
        pass

    def register_module(self, *a, **k):
        return lambda c: c


def _mod(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    m.__path__ = getattr(m, "__path__", [])
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _multi_apply(func, *args, **kwargs):       # mmdet/core/utils/misc.py:11-30
    pfunc = functools.partial(func, **kwargs) if kwargs else func
    return tuple(map(list, zip(*map(pfunc, *args))))


def load_reference():
    _, _, mc, tr, iou = __import__("oracle.gen_golden", fromlist=["import_reference"]).import_reference()
    hung = load_hungarian_assigner(mc)
    ident_deco = lambda *a, **k: (lambda f: f)  # noqa: E731
    _mod("mmcv", jit=ident_deco)
    _mod("mmcv.ops", sigmoid_focal_loss=None)
    _mod("mmcv.cnn", Conv2d=None, Linear=None, build_activation_layer=None, bias_init_with_prob=None)
    _mod("mmcv.cnn.bricks")
    _mod("mmcv.cnn.bricks.transformer", FFN=None, build_positional_encoding=None)
    _mod("mmcv.runner", force_fp32=ident_deco, get_dist_info=lambda: (0, 1))
    _mod("mmdet.core", bbox_cxcywh_to_xyxy=tr.bbox_cxcywh_to_xyxy, bbox_xyxy_to_cxcywh=tr.bbox_xyxy_to_cxcywh,
         build_assigner=None, build_sampler=None, multi_apply=_multi_apply, reduce_mean=lambda t: t,
         multiclass_nms=None, bbox_overlaps=iou.bbox_overlaps)
    _mod("mmdet.models")
    _mod("mmdet.models.builder", HEADS=_Reg(), LOSSES=_Reg(), build_loss=None)
    _mod("mmdet.models.utils", build_transformer=None)
    _mod("mmdet.models.utils.transformer", inverse_sigmoid=None)
    _mod("mmdet.models.dense_heads")
    _mod("mmdet.models.dense_heads.anchor_free_head", AnchorFreeHead=nn.Module)
    _mod("mmdet.models.losses")
    lu = _load("mmdet.models.losses.utils", MMD + "/models/losses/utils.py", "mmdet.models.losses")
    focal = _load("mmdet.models.losses.focal_loss", MMD + "/models/losses/focal_loss.py", "mmdet.models.losses")
    l1 = _load("mmdet.models.losses.smooth_l1_loss", MMD + "/models/losses/smooth_l1_loss.py", "mmdet.models.losses")
    iou_loss = _load("mmdet.models.losses.iou_loss", MMD + "/models/losses/iou_loss.py", "mmdet.models.losses")
    _mod("reflosses")
    tal = _load("reflosses.task_aligned_focal_loss", REF + "/detr_od/models/losses/task_aligned_focal_loss.py", "reflosses")
    # sampler
    _mod("mmdet.core.bbox.builder", BBOX_ASSIGNERS=_Reg(), BBOX_SAMPLERS=_Reg())
    _mod("mmdet.core.bbox.samplers")
    smp = MMD + "/core/bbox/samplers"
    _load("mmdet.core.bbox.samplers.sampling_result", smp + "/sampling_result.py", "mmdet.core.bbox.samplers")
    _load("mmdet.core.bbox.samplers.base_sampler", smp + "/base_sampler.py", "mmdet.core.bbox.samplers")
    ps = _load("mmdet.core.bbox.samplers.pseudo_sampler", smp + "/pseudo_sampler.py", "mmdet.core.bbox.samplers")
    # O2M assigner (as oracle/gen_golden.py gen_o2m)
    _mod("mmdet.core.bbox.match_costs", build_match_cost=lambda cfg: None)
    _mod("mmdet.core.bbox.assigners")
    _mod("mmdet.core.bbox.assigners.assign_result", AssignResult=object)
    _mod("mmdet.core.bbox.assigners.base_assigner", BaseAssigner=object)
    _mod("detr_ssod")
    _mod("detr_ssod.utils", log_every_n=lambda *a, **k: None, log_image_with_boxes=lambda *a, **k: None)
    _mod("refo2m")
    _load("refo2m.o2m_assign_result", REF + "/detr_od/core/bbox/assigners/o2m_assign_result.py", "refo2m")
    o2m = _load("refo2m.o2m_assigner", REF + "/detr_od/core/bbox/assigners/o2m_assigner.py", "refo2m")
    # the head module itself (its relative `from .dn_components import *` resolves to an empty stub)
    _mod("refhead")
    _mod("refhead.dn_components")
    head = _load("refhead.dino_detr_ssod_head", REF + "/detr_od/models/dense_heads/dino_detr_ssod_head.py", "refhead")
    return dict(head=head.DINODETRSSODHead, focal=focal, l1=l1, iou=iou_loss, tal=tal, hung=hung, o2m=o2m.O2MAssigner,
                sampler=ps.PseudoSampler, lu=lu)


def stand_in(ref, warm):
    """``self`` for the unbound reference methods: dino_detr_ssod_r50_coco_120k.py:30-42 losses, train_cfg assigners."""
    H = ref["head"]
    s = types.SimpleNamespace(num_classes=80, cls_out_channels=80, in_warm_up=warm, bg_cls_weight=0.0,
                              sync_cls_avg_factor=False)
    s.loss_cls1 = ref["tal"].TaskAlignedFocalLoss(use_sigmoid=True, gamma=2.0, loss_weight=2.0)
    s.loss_cls2 = ref["focal"].FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0)
    s.loss_bbox = ref["l1"].L1Loss(loss_weight=5.0)
    s.loss_iou = ref["iou"].GIoULoss(loss_weight=2.0)
    s.assigner1, s.assigner2, s.sampler = ref["o2m"](), ref["hung"], ref["sampler"]()
    for name in ("loss", "loss_single", "loss_single_dn", "get_targets", "_get_target_single", "get_targets_dn",
                 "_get_target_single_dn", "prep_for_dn"):
        setattr(s, name, types.MethodType(getattr(H, name), s))
    captured = []
    inner = s.get_targets

    def get_targets(*a, **k):
        out = inner(*a, **k)
        captured.append(out)
        return out
    s.get_targets = get_targets
    return s, captured


CASES = {
    # name: (nl, B, Q, gt counts, single_pad, groups, warm, is_pseudo_label)
    "hungarian": (2, 3, 16, [4, 0, 3], 8, 2, False, False),
    "hungarian_pseudo": (2, 2, 16, [3, 2], 6, 2, False, True),
    "warm_up": (2, 2, 16, [2, 3], 6, 2, True, False),
    "q_lt_g": (2, 2, 6, [8, 2], 16, 1, False, False),
    "no_gt": (2, 2, 12, [0, 0], 4, 2, False, False),
}
HW = [(480, 640), (800, 1333), (512, 512)]


def inputs(seed, nl, B, Q, counts, single_pad, groups, warm, C=80):
    g = torch.Generator().manual_seed(seed)
    pad = single_pad * groups

    def boxes(*shape):
        return torch.cat([torch.rand(*shape, 2, generator=g) * 0.7 + 0.15, torch.rand(*shape, 2, generator=g) * 0.25 + 0.05], -1)

    all_cls = torch.randn(nl, B, Q, C, generator=g) * 2.5
    all_box = boxes(nl, B, Q)
    enc_cls = torch.randn(B, Q, C, generator=g) * 2.5
    enc_box = boxes(B, Q)
    dn_cls = torch.randn(nl, B, pad, C, generator=g) * 2.5
    dn_box = boxes(nl, B, pad)
    if not warm:     # warm-up: the task-aligned loss's fp32 log(1 - p) saturates there by design (clamp at -100)
        all_cls[0, 0, 0, :4] = torch.tensor([30.0, -30.0, 20.0, -20.0])
    dn_cls[-1, 0, 0, :2] = torch.tensor([-30.0, 30.0])
    gts, labs = [], []
    for b in range(B):
        n = counts[b]
        h, w = HW[b]
        lab = torch.randint(0, C, (n,), generator=g)
        m = min(n, Q)
        cx = boxes(n)
        q = torch.randperm(Q, generator=g)[:m]
        # clear cost margins: the first min(Q, G) ground truths sit on a query of every layer (and the encoder), whose
        # logit for that class is raised; the rest (Q < G) are small boxes far from every query
        cx[:m] = all_box[0, b, q] + torch.randn(m, 4, generator=g) * 0.004
        if n > m:
            cx[m:] = torch.tensor([0.03, 0.03, 0.02, 0.02]) + torch.rand(n - m, 4, generator=g) * 0.005
        for t_cls, t_box in [(all_cls[i, b], all_box[i, b]) for i in range(nl)] + [(enc_cls[b], enc_box[b])]:
            t_box[q] = cx[:m] + torch.randn(m, 4, generator=g) * 0.004
            t_cls[q, lab[:m]] += 8.0
        enc_cls[b, q, 0] += 8.0          # the encoder's labels are all 0
        xyxy = torch.cat([cx[:, :2] - cx[:, 2:] / 2, cx[:, :2] + cx[:, 2:] / 2], -1)
        gts.append((xyxy * torch.tensor([w, h, w, h], dtype=torch.float32)).float())
        labs.append(lab)
    return [t.float() for t in (all_cls, all_box, enc_cls, enc_box, dn_cls, dn_box)], gts, labs


def gen_case(ref, d, name, seed):
    nl, B, Q, counts, single_pad, groups, warm, pseudo = CASES[name]
    ins32, gts, labs = inputs(seed, nl, B, Q, counts, single_pad, groups, warm)
    pad = single_pad * groups
    ins = [t.double().requires_grad_(True) for t in ins32]
    metas = [dict(img_shape=(HW[b][0], HW[b][1], 3)) for b in range(B)]
    dn_meta = dict(num_dn_group=groups, pad_size=pad, num_dn_group_2=groups, pad_size_2=pad)
    s, captured = stand_in(ref, warm)
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self        # _get_target_single_dn calls .cuda()
    try:
        out = ref["head"].loss(s, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], [g.double() for g in gts], labs, None,
                               metas, dn_meta, None, pseudo)
    finally:
        torch.Tensor.cuda = orig_cuda
    keys = list(out)
    coef = 1.0 + 0.05 * np.arange(len(keys))
    tot = sum(float(c) * out[k] for c, k in zip(coef, keys))
    tot.backward()
    p = name + "."
    for k, t in zip(("all_cls", "all_box", "enc_cls", "enc_box", "dn_cls", "dn_box"), ins32):
        d[p + k] = t.numpy()
    for k, t in zip(("all_cls", "all_box", "enc_cls", "enc_box", "dn_cls", "dn_box"), ins):
        d[p + "grad_" + k] = t.grad.numpy()
    d[p + "gt_boxes"] = torch.cat([g.reshape(-1, 4) for g in gts]).numpy()
    d[p + "gt_counts"] = np.asarray(counts, np.int64)
    d[p + "gt_labels"] = torch.cat(labs).numpy().astype(np.int64)
    d[p + "img_hw"] = np.asarray(HW[:B], np.int64)
    d[p + "single_pad"], d[p + "groups"] = np.int64(single_pad), np.int64(groups)
    d[p + "warm_up"], d[p + "is_pseudo_label"] = np.bool_(warm), np.bool_(pseudo)
    d[p + "keys"] = np.asarray(keys)
    d[p + "values"] = np.asarray([float(out[k].detach()) for k in keys], np.float64)
    d[p + "coef"] = coef
    # targets of the decoder layers (in order) then the encoder: nl + 1 get_targets calls of B images each
    assert len(captured) == nl + 1
    names = ["labels", "label_weights", "bbox_targets", "bbox_weights"] + (["norm_metrics"] if warm else [])
    for i, n in enumerate(names):
        v = torch.stack([torch.stack(list(c[i])) for c in captured]).reshape((nl + 1) * B, Q, *([4] if "bbox" in n else []))
        d[p + n] = v.detach().numpy().astype(np.int64 if n == "labels" else np.float64)


def main():
    ref = load_reference()
    d = {}
    for i, name in enumerate(CASES):
        gen_case(ref, d, name, 100 + i)
    d["names"] = np.asarray(list(CASES))
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

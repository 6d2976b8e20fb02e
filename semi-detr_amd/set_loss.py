"""Set-prediction losses of the SSOD head on the MI355X (``csrc/set_loss.hip``).

* ``loss_set`` replaces ``DINODETRSSODHead.loss`` with ``loss_single`` / ``loss_single_dn`` / ``get_targets_dn``
  (detr_od/models/dense_heads/dino_detr_ssod_head.py:508-985): same signature, same dict keys in the same order, and it
  reads the same attributes from ``self``, so it binds as ``DINODETRSSODHead.loss = semi_detr_amd.loss_set``.  The
  targets of every decoder layer and of the encoder proposals come from ONE ``targets._targets_stacked`` batch; the dn
  targets are built inside the loss kernel from the ground truths.  Every focal / L1 / GIoU term of the call is one
  forward launch plus one fixed-order reduce, and the backward of all of them is one launch.  The Hungarian branch reads
  nothing back to the host; with several ranks the normalisers the reference passes through ``reduce_mean`` take one
  all-reduce per call.
* ``FocalLoss`` is a drop-in for mmdet's ``FocalLoss`` (focal_loss.py:107-175), which on a GPU tensor calls the mmcv-full
  CUDA op ``sigmoid_focal_loss``.
* ``set_losses`` is the lower level: a list of ``SetLossSegment`` -> one 0-d loss per (segment, layer, term).
"""
import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from .targets import _targets_stacked

MATCHED, DN, WARMUP, NUM_STATS, NUM_TERMS, MAX_LAYERS = (
    _lib.CONSTANTS["SEMIDETR_SET_LOSS_" + n] for n in ("MATCHED", "DN", "WARMUP", "NUM_STATS", "NUM_TERMS", "MAX_LAYERS"))
TERMS = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
STATS = ("cls_sum", "l1_sum", "l1_xy", "l1_hw", "giou_sum", "num_pos", "num_bw_rows", "num_any_bw_rows", "pos_bw0_sum",
         "metric_sum")


_Segment = _lib.SetLossSegment


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.stride(-1) == 1 else t.contiguous()


class SetLossSegment:
    """One segment of the loss kernel: ``cls`` (nl, B, Q, C) logits and ``boxes`` (nl, B, Q, 4) cxcywh (or None), any
    strides with a unit-stride last dimension, plus the targets of its kind:

    * ``MATCHED`` / ``WARMUP``: ``labels`` (nl*B, Q) int64, ``label_weights`` (nl*B, Q) or None, ``bbox_targets`` /
      ``bbox_weights`` (nl*B, Q, 4), and for ``WARMUP`` ``metrics`` (nl*B, Q) (task-aligned focal classification);
    * ``DN``: ``gt_bboxes`` / ``gt_labels`` lists (one tensor per image, xyxy image scale), ``single_pad``, ``dn_groups``.

    ``img_wh`` (B, 2) fp32 device tensor of (w, h); ``params``: alpha, gamma, cls_weight, l1_weight, iou_weight, iou_eps,
    bg_cls_weight, sync_cls."""

    def __init__(self, kind, cls, boxes=None, labels=None, label_weights=None, bbox_targets=None, bbox_weights=None,
                 metrics=None, gt_bboxes=None, gt_labels=None, single_pad=0, dn_groups=0, img_wh=None, alpha=0.25,
                 gamma=2.0, cls_weight=1.0, l1_weight=1.0, iou_weight=1.0, iou_eps=1e-6, bg_cls_weight=0.0, sync_cls=False):
        if cls.dim() != 4 or (boxes is not None and (boxes.dim() != 4 or boxes.shape[:3] != cls.shape[:3]
                                                     or boxes.shape[3] != 4)):
            raise ValueError(f"set_loss: expected (nl,B,Q,C) logits and (nl,B,Q,4) boxes, got {tuple(cls.shape)}, "
                             f"{None if boxes is None else tuple(boxes.shape)}")
        self.kind, self.cls, self.boxes = kind, cls, boxes
        self.nl, self.B, self.Q, self.C = cls.shape
        dev = cls.device
        c = lambda t, dt: None if t is None else t.detach().to(device=dev, dtype=dt).contiguous()  # noqa: E731
        self.labels, self.label_weights = c(labels, torch.int64), c(label_weights, torch.float32)
        self.bbox_targets, self.bbox_weights = c(bbox_targets, torch.float32), c(bbox_weights, torch.float32)
        self.metrics = c(metrics, torch.float32)
        self.img_wh = c(img_wh, torch.float32)
        self.single_pad, self.dn_groups = int(single_pad), int(dn_groups)
        self.gt_offsets = self.gt_boxes = self.gt_labels = None
        if kind == DN:
            counts = [int(g.shape[0]) for g in gt_bboxes]
            if len(counts) != self.B or any(n > self.single_pad for n in counts):
                raise ValueError(f"set_loss: dn needs one gt list per image and G_b <= single_pad ({counts}, "
                                 f"single_pad {self.single_pad})")
            _, self.gt_offsets = _lib.offsets(counts, dev)
            if sum(counts):
                self.gt_boxes = torch.cat([g.reshape(-1, 4) for g in gt_bboxes]).to(dev, torch.float32).contiguous()
                self.gt_labels = torch.cat([g.reshape(-1) for g in gt_labels]).to(dev, torch.int64).contiguous()
            else:                        # nothing is read; the kernel only needs valid pointers
                self.gt_boxes = torch.zeros((1, 4), dtype=torch.float32, device=dev)
                self.gt_labels = torch.zeros(1, dtype=torch.int64, device=dev)
        self.params = (float(alpha), float(gamma), float(cls_weight), float(l1_weight), float(iou_weight), float(iou_eps),
                       float(bg_cls_weight), int(bool(sync_cls)))

    def struct(self, cls, boxes, grad_logits=None, grad_boxes=None):
        s = _Segment()
        s.kind, s.num_layers, s.num_images, s.num_query, s.num_classes = self.kind, self.nl, self.B, self.Q, self.C
        s.logits = _ptr(cls)
        s.logit_stride[:] = list(cls.stride()[:3])
        if boxes is not None:
            s.boxes = _ptr(boxes)
            s.box_stride[:] = list(boxes.stride()[:3])
        s.labels, s.label_weights = _ptr(self.labels), _ptr(self.label_weights)
        s.bbox_targets, s.bbox_weights, s.metrics = _ptr(self.bbox_targets), _ptr(self.bbox_weights), _ptr(self.metrics)
        s.gt_offsets, s.gt_boxes, s.gt_labels = _ptr(self.gt_offsets), _ptr(self.gt_boxes), _ptr(self.gt_labels)
        s.single_pad, s.dn_groups, s.img_wh = self.single_pad, self.dn_groups, _ptr(self.img_wh)
        (s.alpha, s.gamma, s.cls_weight, s.l1_weight, s.iou_weight, s.iou_eps, s.bg_cls_weight, s.sync_cls) = self.params
        s.grad_logits, s.grad_boxes = _ptr(grad_logits), _ptr(grad_boxes)
        return s


def _table(segs, inputs, grads=None):
    arr = (_Segment * len(segs))()
    for i, sg in enumerate(segs):
        g = grads[2 * i: 2 * i + 2] if grads is not None else (None, None)
        arr[i] = sg.struct(inputs[2 * i], inputs[2 * i + 1], g[0], g[1])
    return arr


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


def _forward(segs, flat, group, finalize=True):
    """Forward launches of ``segs`` over the fp32 inputs ``flat`` -> dict(stats, norms, norms_reduced, losses, scales).
    ``finalize=False``: the raw stats and normaliser inputs only -- no normalisers, so no collective either (losses and
    scales are then left unset)."""
    tab = _table(segs, flat)
    nbytes = int(_lib.lib().semidetr_set_loss_workspace_bytes(tab, len(segs)))
    if nbytes < 0:
        _lib.check(nbytes, "semidetr_set_loss_workspace_bytes")
    T = sum(sg.nl for sg in segs)
    dev = flat[0].device
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    stats = torch.empty((T, NUM_STATS), dtype=torch.float64, device=dev)
    norms = torch.empty((T, 2), dtype=torch.float32, device=dev)
    losses = torch.empty((T, NUM_TERMS), dtype=torch.float32, device=dev)
    scales = torch.empty((T, NUM_TERMS), dtype=torch.float32, device=dev)
    world = _world(group) if finalize else 1
    reduced = None
    fin = finalize and world == 1
    _lib.call("semidetr_set_loss_forward_f32", dev, tab, len(segs), ws, nbytes, stats, norms, losses if fin else None,
              scales if fin else None)
    if finalize and not fin:
        with _lib.device_guard(dev):                         # the collective runs with the tensors' device current
            reduced = norms / world                          # mmdet reduce_mean: divide, then all-reduce SUM
            dist.all_reduce(reduced, op=dist.ReduceOp.SUM, group=group)
        _lib.call("semidetr_set_loss_finalize_f32", dev, tab, len(segs), stats, norms, reduced, losses, scales)
    return dict(stats=stats, norms=norms, norms_reduced=reduced, losses=losses, scales=scales)


class _SetLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, segs, group, info, *inputs):
        ctx.set_materialize_grads(False)
        if not inputs[0].is_cuda:
            raise RuntimeError("set_loss: tensors must live on the GPU (no CPU fallback)")
        flat = [_f32(t.detach()) if t is not None else None for t in inputs]
        r = _forward(segs, flat, group)
        if info is not None:
            info.update(r)
        ctx.segs = segs
        ctx.save_for_backward(r["scales"], *flat)
        ctx.in_meta = [(t.shape, t.dtype) if t is not None else None for t in inputs]
        return tuple(r["losses"].view(-1).unbind(0))

    @staticmethod
    def backward(ctx, *grads):
        scales, *flat = ctx.saved_tensors
        want = ctx.needs_input_grad[3:]
        if not any(want) or all(g is None for g in grads):
            return (None, None, None) + tuple(None for _ in want)
        zero = scales.new_zeros(())
        gout = torch.stack([g.reshape(()).float() if g is not None else zero for g in grads]).contiguous()
        out = [torch.empty(m[0], dtype=torch.float32, device=scales.device) if (w and m is not None) else None
               for w, m in zip(want, ctx.in_meta)]
        tab = _table(ctx.segs, flat, out)
        _lib.call("semidetr_set_loss_backward_f32", scales.device, tab, len(ctx.segs), scales, gout)
        out = [o.to(m[1]) if o is not None and o.dtype != m[1] else o for o, m in zip(out, ctx.in_meta)]
        return (None, None, None) + tuple(out)


def set_losses(segments, group=None, info=None):
    """All terms of the given segments: a list of ``sum(nl)`` lists of 5 0-d fp32 tensors (cls, bbox, iou, bbox_xy,
    bbox_hw), each already divided by its normaliser and multiplied by its loss weight.  ``info`` (a dict) receives the
    raw ``stats`` (T, 10) fp64, ``norms`` (T, 2), ``norms_reduced`` (several ranks) and ``scales`` (T, 5)."""
    inputs = []
    for sg in segments:
        inputs += [sg.cls, sg.boxes]
    outs = _SetLossFn.apply(list(segments), group, info, *inputs)
    return [list(outs[i:i + NUM_TERMS]) for i in range(0, len(outs), NUM_TERMS)]


# ----------------------------------------------------------------------------------------------------------------------
# DINODETRSSODHead.loss

def _prep_for_dn(dn_meta, is_pseudo_label):
    """dino_detr_ssod_head.py:328-339."""
    if is_pseudo_label:
        groups, pad = dn_meta["num_dn_group_2"], dn_meta["pad_size_2"]
    else:
        groups, pad = dn_meta["num_dn_group"], dn_meta["pad_size"]
    assert pad % groups == 0
    return pad // groups, groups


def _weight(loss_mod, name, default):
    return float(getattr(loss_mod, name, default)) if loss_mod is not None else float(default)


def loss_set(self, all_cls_scores, all_bbox_preds, enc_cls_scores, enc_bbox_preds, dn_cls_scores, dn_bbox_preds,
             gt_bboxes_list, gt_labels_list, gt_scores_list=None, img_metas=None, dn_metas=None, gt_bboxes_ignore=None,
             is_pseudo_label=False):
    """``DINODETRSSODHead.loss`` (dino_detr_ssod_head.py:508-624): same arguments, same dict keys in the same order."""
    assert gt_bboxes_ignore is None, f"{self.__class__.__name__} only supports for gt_bboxes_ignore setting to None."
    nl, B, Q, C = all_cls_scores.shape
    dev = all_cls_scores.device
    warm = bool(getattr(self, "in_warm_up", False))
    num_classes = int(self.num_classes)
    gt_bboxes_list, gt_labels_list, img_metas = list(gt_bboxes_list), list(gt_labels_list), list(img_metas)
    has_enc = enc_cls_scores is not None
    # one batch of (nl [+ 1]) x B assignment problems; the encoder's use all-zero labels (head.py:565-574)
    cls_t = all_cls_scores.detach().reshape(nl * B, Q, C)
    box_t = all_bbox_preds.detach().reshape(nl * B, Q, 4)
    gts, labs, metas = gt_bboxes_list * nl, gt_labels_list * nl, img_metas * nl
    if has_enc:
        cls_t = torch.cat([cls_t, enc_cls_scores.detach().reshape(B, Q, C)])
        box_t = torch.cat([box_t, enc_bbox_preds.detach().reshape(B, Q, 4)])
        gts, labs, metas = gts + gt_bboxes_list, labs + [torch.zeros_like(g) for g in gt_labels_list], metas + img_metas
    t = _targets_stacked(self, cls_t.float(), box_t.float(), gts, labs, metas, check=False)
    img_wh = _lib.small_to_device([[float(m["img_shape"][1]), float(m["img_shape"][0])] for m in img_metas], torch.float32, dev)

    iou = self.loss_iou
    common = dict(img_wh=img_wh, l1_weight=_weight(self.loss_bbox, "loss_weight", 1.0),
                  iou_weight=_weight(iou, "loss_weight", 1.0), iou_eps=_weight(iou, "eps", 1e-6),
                  bg_cls_weight=float(getattr(self, "bg_cls_weight", 0.0)),
                  sync_cls=bool(getattr(self, "sync_cls_avg_factor", False)))
    c2 = self.loss_cls2
    focal = dict(alpha=_weight(c2, "alpha", 0.25), gamma=_weight(c2, "gamma", 2.0), cls_weight=_weight(c2, "loss_weight", 1.0))
    if warm:
        c1 = self.loss_cls1
        mcls = dict(kind=WARMUP, gamma=_weight(c1, "gamma", 2.0), cls_weight=_weight(c1, "loss_weight", 1.0))
    else:
        mcls = dict(kind=MATCHED, **focal)

    def matched(lo, hi, cls, boxes):
        return SetLossSegment(cls=cls, boxes=boxes, labels=t["labels"][lo:hi], bbox_targets=t["bbox_targets"][lo:hi],
                              bbox_weights=t["bbox_weights"][lo:hi],
                              label_weights=None if warm else t["label_weights"][lo:hi],
                              metrics=t["norm_metrics"][lo:hi] if warm else None, **mcls, **common)

    segs = [matched(0, nl * B, all_cls_scores, all_bbox_preds)]
    if has_enc:
        segs.append(matched(nl * B, (nl + 1) * B, enc_cls_scores.unsqueeze(0), enc_bbox_preds.unsqueeze(0)))
    with_dn = dn_cls_scores is not None and not (warm and is_pseudo_label)
    if with_dn:
        single_pad, groups = _prep_for_dn(dn_metas, is_pseudo_label)
        segs.append(SetLossSegment(kind=DN, cls=dn_cls_scores, boxes=dn_bbox_preds, gt_bboxes=gt_bboxes_list,
                                   gt_labels=gt_labels_list, single_pad=single_pad, dn_groups=groups, **focal, **common))
    terms = set_losses(segs)
    dec = terms[:nl]
    enc = terms[nl] if has_enc else None
    if with_dn:
        dn = terms[nl + int(has_enc):]
    else:     # head.py:536-541 (warm-up on pseudo labels), or no dn queries at all
        n_dn = dn_cls_scores.shape[0] if dn_cls_scores is not None else nl
        dn = [list(z.unbind(0)) for z in all_cls_scores.new_zeros((n_dn, NUM_TERMS), dtype=torch.float32).unbind(0)]
    out = {}
    if has_enc:
        for k, v in zip(TERMS, enc):
            out["enc_" + k] = v
    for k, v in zip(TERMS, dec[-1]):
        out[k] = v
    for k, v in zip(TERMS, dn[-1]):
        out["dn_" + k] = v
    for i, (d, n) in enumerate(zip(dec[:-1], dn[:-1])):
        for k, v in zip(TERMS, d):
            out[f"d{i}.{k}"] = v
        for k, v in zip(TERMS, n):
            out[f"d{i}.dn_{k}"] = v
    return out


# ----------------------------------------------------------------------------------------------------------------------
# mmdet FocalLoss

class _FocalSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, gamma, alpha):
        if not pred.is_cuda:
            raise RuntimeError("FocalLoss: tensors must live on the GPU (no CPU fallback)")
        if pred.dim() != 2 or target.shape != pred.shape[:1] or (weight is not None and weight.shape != pred.shape[:1]):
            raise ValueError(f"FocalLoss: expected (N,C) pred with (N,) target / weight, got {tuple(pred.shape)}, "
                             f"{tuple(target.shape)}, {None if weight is None else tuple(weight.shape)}")
        x = _f32(pred.detach()).unsqueeze(0).unsqueeze(0)
        seg = SetLossSegment(MATCHED, x, labels=target.reshape(1, -1), label_weights=None if weight is None
                             else weight.reshape(1, -1), gamma=gamma, alpha=alpha)
        r = _forward([seg], [x, None], None, finalize=False)      # mmdet's FocalLoss does no communication
        ctx.seg, ctx.x, ctx.in_dtype = seg, x, pred.dtype
        return r["stats"][0, 0].float()

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        gout = torch.nn.functional.pad(g.reshape(1).float(), (0, NUM_TERMS - 1))
        grad = torch.empty_like(ctx.x, memory_format=torch.contiguous_format)
        tab = _table([ctx.seg], [ctx.x, None], [grad, None])
        _lib.call("semidetr_set_loss_backward_f32", grad.device, tab, 1, None, gout)
        return grad[0, 0].to(ctx.in_dtype), None, None, None, None


class FocalLoss(nn.Module):
    """mmdet ``FocalLoss`` (focal_loss.py:107-175) with use_sigmoid: the sigmoid focal loss of ``py_sigmoid_focal_loss``
    in one streaming launch (log-sigmoid through softplus, stable at any |x|).  ``target`` (N,) class indices in
    [0, C] (C = background), ``weight`` None or (N,).  ``reduction='none'`` is not built (no call site uses it)."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert use_sigmoid is True, "Only sigmoid focal loss supported now."
        self.use_sigmoid, self.gamma, self.alpha = use_sigmoid, gamma, alpha
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert reduction_override in (None, "none", "mean", "sum")
        reduction = reduction_override if reduction_override else self.reduction
        if reduction == "none":
            raise NotImplementedError("FocalLoss: reduction='none' would materialise the element-wise loss")
        if weight is not None and weight.dim() != 1:
            raise NotImplementedError("FocalLoss: only per-row (N,) weights are built")
        total = _FocalSum.apply(pred, target, weight, float(self.gamma), float(self.alpha))
        if avg_factor is None:                       # mmdet weight_reduce_loss (losses/utils.py:29-55)
            loss = total / max(pred.numel(), 1) if reduction == "mean" else total
        elif reduction == "mean":
            loss = total / avg_factor
        else:
            raise ValueError('avg_factor can not be used with reduction="sum"')
        return self.loss_weight * loss

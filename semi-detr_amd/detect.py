"""Decoding detections at evaluation / inference time on the MI355X (``csrc/detect.hip``): the path ``tools/test.py`` takes
through ``simple_test_bboxes`` -> ``get_bboxes`` -> ``_get_bboxes_single`` with ``for_pseudo_label=False``
(detr_od/models/dense_heads/dino_detr_ssod_head.py:1316-1330, 1396-1413; dino_detr_head.py:1082-1095, 1129-1137, 1143-1152)
and mmdet's ``bbox2result`` behind it (thirdparty/mmdetection/mmdet/core/bbox/transforms.py:100-117).

* ``get_bboxes`` replaces the per-image loop: sigmoid, flat ``topk(max_per_img)`` over Q * C scores, ``%`` / ``//``, the box
  gather, cxcywh -> xyxy, scale, clamp, the division by ``scale_factor`` and the ``cat``.  Two launches for the whole batch, no
  host synchronisation (every list entry has k rows).
* ``detection_results`` adds ``bbox2result``: the rows are grouped by class on the device and travel to the host in one pinned,
  non-blocking copy together with the class offsets; the per-class arrays are slices of that copy.

Selection order.  The kernels select on the logits, by (logit descending, flat index ``q * C + c`` ascending): a total order, so
the result is the same run after run.  ``torch.topk`` over the sigmoids leaves the order among equal scores open -- equal logits,
and distinct logits whose fp32 sigmoids coincide (every logit above ~17 gives 1.0) -- and this is one valid resolution of all of
them.  NaN ranks above +inf.

Sigmoid heads only (``loss_cls.use_sigmoid``); the softmax branch (dino_detr_head.py:1138-1141) is not built.  The NMS branch of
the same function is ``pseudo_label.get_bboxes_for_pseudo_label``.
"""
import numpy as np
import torch

from . import _lib

MAX_K = _lib.CONSTANTS["SEMIDETR_DET_MAX_K"]


def _last_layer(all_cls_scores, all_bbox_preds):
    """``all_cls_scores[-1]``, ``all_bbox_preds[-1]`` (dino_detr_ssod_head.py:1316-1317) as contiguous fp32 (B, Q, C) / (B, Q, 4)."""
    cls, box = all_cls_scores[-1], all_bbox_preds[-1]
    if not (isinstance(cls, torch.Tensor) and isinstance(box, torch.Tensor)):
        raise ValueError("detect: all_cls_scores / all_bbox_preds must be (layers, B, Q, C) / (layers, B, Q, 4) tensors or lists "
                         "of per-layer tensors")
    if not (cls.is_cuda and box.is_cuda):
        raise RuntimeError("detect: all_cls_scores and all_bbox_preds must live on the GPU (no CPU fallback)")
    if cls.dim() != 3 or box.shape != cls.shape[:2] + (4,):
        raise ValueError(f"detect: expected cls_scores (B, Q, C) and bbox_preds (B, Q, 4) in the last layer, got "
                         f"{tuple(cls.shape)} and {tuple(box.shape)}")
    if cls.shape[1] == 0 or cls.shape[2] == 0:
        raise ValueError(f"detect: empty cls_scores {tuple(cls.shape)}")
    return cls.detach().to(torch.float32).contiguous(), box.detach().to(torch.float32).contiguous()


def _launch(all_cls_scores, all_bbox_preds, img_metas, rescale, max_per_img, num_query, grouped):
    cls, box = _last_layer(all_cls_scores, all_bbox_preds)
    B, Q, C = cls.shape
    if len(img_metas) != B:
        raise ValueError(f"detect: {len(img_metas)} img_metas for a batch of {B}")
    k = int(max_per_img) if max_per_img is not None else int(num_query) if num_query is not None else Q
    if k > Q * C or k < 0:
        raise RuntimeError("selected index k out of range")          # torch.topk's own error
    if k == 0 or k > MAX_K:
        raise ValueError(f"detect: max_per_img {k} (1..{MAX_K})")
    dev = cls.device
    hw = _lib.small_to_device([[float(m["img_shape"][0]), float(m["img_shape"][1])] for m in img_metas], torch.float32, dev)
    sf = None
    if rescale:
        rows = [[float(v) for v in np.asarray(m["scale_factor"]).reshape(-1)] for m in img_metas]
        if any(len(r) != 4 for r in rows):
            raise ValueError("detect: scale_factor must hold (w_scale, h_scale, w_scale, h_scale)")
        sf = _lib.small_to_device(rows, torch.float32, dev)
    ws_bytes = int(_lib.lib().semidetr_det_workspace_bytes(B, Q, C, k))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    dets = torch.empty((B, k, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    packed = by_class = offsets = None
    if grouped:
        # rows and offsets in one buffer (both are 4-byte types): one copy takes them to the host
        packed = torch.empty(B * k * 5 + B * (C + 1), dtype=torch.float32, device=dev)
        by_class = packed[:B * k * 5]
        offsets = packed[B * k * 5:]
    _lib.call("semidetr_det_decode_f32", dev, cls, box, hw, sf, B, Q, C, k, ws, ws_bytes, dets, labels, by_class, offsets)
    return dets, labels, packed, (B, C, k)


def get_bboxes(all_cls_scores, all_bbox_preds, img_metas, rescale=False, max_per_img=None, num_query=None):
    """``get_bboxes(..., for_pseudo_label=False)`` of both heads.  ``all_cls_scores`` (layers, B, Q, C) raw logits and
    ``all_bbox_preds`` (layers, B, Q, 4) normalised cxcywh (tensors or per-layer lists; the last layer is used); ``img_metas``:
    dicts with 'img_shape' and, for ``rescale``, 'scale_factor'.  ``max_per_img=None`` means ``num_query`` (default: Q), as
    ``test_cfg.get('max_per_img', self.num_query)``.  Returns the reference's result_list on the device:
    [(det_bboxes (k, 5), det_labels (k,)), ...]."""
    dets, labels, _, (B, _, _) = _launch(all_cls_scores, all_bbox_preds, img_metas, rescale, max_per_img, num_query, False)
    return [(dets[b], labels[b]) for b in range(B)]


class PendingDetections:
    """Per-class results whose rows are still on their way to the host (pinned buffer + event): the kernels and the copy are
    queued, ``result()`` waits for the event and slices."""

    def __init__(self, packed, sizes, num_classes):
        self._sizes, self._num_classes = sizes, int(num_classes)
        self._host = torch.empty(packed.shape, dtype=packed.dtype).pin_memory()
        self._host.copy_(packed, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._lists = None

    def result(self):
        if self._lists is None:
            self._event.synchronize()
            B, C, k = self._sizes
            flat = self._host.numpy().copy()
            rows = flat[:B * k * 5].reshape(B, k, 5)
            offs = flat[B * k * 5:].view(np.int32).reshape(B, C + 1)
            empty = np.zeros((0, 5), dtype=np.float32)
            self._lists = [[rows[b, offs[b, c]:offs[b, c + 1]] if c < C else empty for c in range(self._num_classes)]
                           for b in range(B)]
            self._host = None
        return self._lists


def detection_results(all_cls_scores, all_bbox_preds, img_metas, num_classes, rescale=False, max_per_img=None, wait=True):
    """What ``simple_test`` returns: ``bbox2result(det_bboxes, det_labels, num_classes)`` of every image of ``get_bboxes`` -- per
    image a list of ``num_classes`` float32 numpy arrays (n_c, 5), score order kept inside a class.  One pinned copy and one
    event wait; with ``wait=False`` a ``PendingDetections`` whose ``result()`` gives the same lists later."""
    _, _, packed, sizes = _launch(all_cls_scores, all_bbox_preds, img_metas, rescale, max_per_img, None, True)
    pending = PendingDetections(packed, sizes, num_classes)
    return pending.result() if wait else pending

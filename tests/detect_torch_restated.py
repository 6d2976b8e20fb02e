"""The reference's evaluation-time decode as the sequence of torch ops it issues per image (detr_od/models/dense_heads/
dino_detr_ssod_head.py:1316-1330, 1396-1413) and mmdet's bbox2result (mmdet/core/bbox/transforms.py:100-117), written out again
for this project: the baseline of tools/detect_probe.py.  tests/test_detect_ref.py checks it bit for bit against the fixture
that the reference's own functions produced, so that the baseline is the reference's arithmetic and not this project's."""
import numpy as np
import torch


def decode_image(logits, boxes, shape, factor, rescale, k):
    """sigmoid, flat topk, % and //, gather, cxcywh -> xyxy, two strided scales, two strided clamps, divide, cat."""
    classes = logits.shape[-1]
    top, where = logits.sigmoid().view(-1).topk(k)
    names = where % classes
    picked = boxes[where // classes]
    mid_x, mid_y, wide, tall = picked.split((1, 1, 1, 1), dim=-1)
    corners = torch.cat([mid_x - 0.5 * wide, mid_y - 0.5 * tall, mid_x + 0.5 * wide, mid_y + 0.5 * tall], dim=-1)
    corners[:, 0::2] = corners[:, 0::2] * shape[1]
    corners[:, 1::2] = corners[:, 1::2] * shape[0]
    corners[:, 0::2].clamp_(min=0, max=shape[1])
    corners[:, 1::2].clamp_(min=0, max=shape[0])
    if rescale:
        corners /= corners.new_tensor(factor)
    return torch.cat((corners, top.unsqueeze(1)), -1), names


def get_bboxes(all_logits, all_boxes, metas, rescale, k):
    logits, boxes = all_logits[-1], all_boxes[-1]
    return [decode_image(logits[i], boxes[i], metas[i]["img_shape"], metas[i]["scale_factor"], rescale, k)
            for i in range(len(metas))]


def per_class(rows, names, classes):
    """bbox2result: one host round trip, then a boolean-mask selection per class."""
    if rows.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(classes)]
    rows, names = rows.detach().cpu().numpy(), names.detach().cpu().numpy()
    return [rows[names == c, :] for c in range(classes)]


def detection_results(all_logits, all_boxes, metas, classes, rescale, k):
    return [per_class(rows, names, classes) for rows, names in get_bboxes(all_logits, all_boxes, metas, rescale, k)]

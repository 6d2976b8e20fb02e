"""The reference's two-stage query selection as the sequence of torch ops it issues (detr_od/models/utils/transformer.py:
525-575, 1325-1334, 1398), written out again for this project: the baseline of tools/query_select_probe.py.
tests/test_query_select_ref.py checks it bit for bit against the fixture that the reference's own functions produced, so
that the baseline is the reference's arithmetic and not this project's."""
import torch

INF = float("inf")


def gen_proposals(memory, padding_mask, spatial_shapes):
    """Per level: counts of row 0 / column 0, meshgrid, cat, divide, anchors, cat; then compare, all, log, four fills."""
    batch = memory.shape[0]
    dev = memory.device
    per_level, start = [], 0
    for level, (rows, cols) in enumerate(spatial_shapes):
        m = padding_mask[:, start:start + rows * cols].view(batch, rows, cols, 1)
        count_h = torch.sum(~m[:, :, 0, 0], 1)
        count_w = torch.sum(~m[:, 0, :, 0], 1)
        ys, xs = torch.meshgrid(torch.linspace(0, rows - 1, rows, dtype=torch.float32, device=dev),
                                torch.linspace(0, cols - 1, cols, dtype=torch.float32, device=dev), indexing="ij")
        xy = torch.cat([xs.unsqueeze(-1), ys.unsqueeze(-1)], -1)
        denom = torch.cat([count_w.unsqueeze(-1), count_h.unsqueeze(-1)], 1).view(batch, 1, 1, 2)
        xy = (xy.unsqueeze(0).expand(batch, -1, -1, -1) + 0.5) / denom
        size = torch.ones_like(xy) * 0.05 * (2.0 ** level)
        per_level.append(torch.cat((xy, size), -1).view(batch, -1, 4))
        start += rows * cols
    anchors = torch.cat(per_level, 1)
    inside = ((anchors > 0.01) & (anchors < 0.99)).all(-1, keepdim=True)
    anchors = torch.log(anchors / (1 - anchors))
    anchors = anchors.masked_fill(padding_mask.unsqueeze(-1), INF)
    anchors = anchors.masked_fill(~inside, INF)
    kept = memory.masked_fill(padding_mask.unsqueeze(-1), 0.0)
    kept = kept.masked_fill(~inside, 0.0)
    return kept, anchors


def select(class_logits, coord, anchors, memory, k):
    """max over the classes, topk over the tokens, three gathers with repeat-expanded indices, two sigmoids."""
    chosen = torch.topk(class_logits.max(-1)[0], k, dim=1)[1]
    four = chosen.unsqueeze(-1).repeat(1, 1, 4)
    boxes = torch.gather(coord, 1, four)
    first_boxes = torch.gather(anchors, 1, four).sigmoid()
    rows = torch.gather(memory, 1, chosen.unsqueeze(-1).repeat(1, 1, memory.shape[2]))
    return chosen, boxes, first_boxes, rows, boxes.sigmoid()

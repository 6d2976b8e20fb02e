#!/usr/bin/env python
"""Times one SSOD-unsup-shaped (B 4) and one sup-shaped (B 1) head ``loss()``, forward + backward including the targets,
two ways: (a) ``semi_detr_amd.loss_set``; (b) a reference-shaped torch composition written here that follows the op
sequence of ``loss_single`` / ``loss_single_dn`` (dino_detr_ssod_head.py:626-883): per-layer ``.item()`` normalisers,
per-image ``new_tensor`` factors, ``nonzero().unique()``, ``torch.arange(...).cuda()`` dn targets and
``py_sigmoid_focal_loss`` for the mmcv op this stack does not have.  Both use this project's batched ``get_targets``.

    python tools/set_loss_probe.py [--iters N] [--only new|ref]

Prints one JSON line per (shape, path): wall ms per call (synchronised) and event ms.  Kernel counts come from a separate
``rocprofv3 --kernel-trace --stats`` run of the same script with ``--only``.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
WH = ((640, 480), (1333, 800), (512, 512), (800, 1199))


class _Attrs:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_head():
    """The attributes loss() reads, with the SSOD config's values (dino_detr_ssod_r50_coco_120k.py:30-42)."""
    from semi_detr_amd import TargetAssigner
    h = TargetAssigner(num_classes=80)
    h.loss_cls1 = _Attrs(gamma=2.0, loss_weight=2.0)
    h.loss_cls2 = _Attrs(gamma=2.0, alpha=0.25, loss_weight=2.0)
    h.loss_bbox, h.loss_iou = _Attrs(loss_weight=5.0), _Attrs(loss_weight=2.0, eps=1e-6)
    h.bg_cls_weight, h.sync_cls_avg_factor = 0.0, False
    return h


def make_inputs(seed, nl=6, B=4, Q=900, C=80, single_pad=20, groups=10):
    """Seeded head outputs (dn queries first, as outputs_class), 5 ground truths per image, dn meta."""
    g = torch.Generator().manual_seed(seed)
    pad = single_pad * groups
    dev = torch.device("cuda")

    def boxes(*shape):
        return torch.cat([torch.rand(*shape, 2, generator=g) * 0.8 + 0.1, torch.rand(*shape, 2, generator=g) * 0.4 + 0.02], -1)

    out_cls, out_box = torch.randn(nl, B, pad + Q, C, generator=g) * 2, boxes(nl, B, pad + Q)
    enc_cls, enc_box = torch.randn(B, Q, C, generator=g) * 2, boxes(B, Q)
    gts, labs = [], []
    for b in range(B):
        w, h = WH[b]
        c = boxes(5)
        gts.append(torch.cat([c[:, :2] - c[:, 2:] / 2, c[:, :2] + c[:, 2:] / 2], -1) * torch.tensor([w, h, w, h]))
        labs.append(torch.randint(0, C, (5,), generator=g))
    return dict(out_cls=out_cls.to(dev).requires_grad_(True), out_box=out_box.to(dev).requires_grad_(True),
                enc_cls=enc_cls.to(dev).requires_grad_(True), enc_box=enc_box.to(dev).requires_grad_(True), pad=pad,
                gts=[x.to(dev) for x in gts], labs=[x.to(dev) for x in labs],
                metas=[dict(img_shape=(WH[b][1], WH[b][0], 3)) for b in range(B)],
                dn_meta=dict(num_dn_group=groups, pad_size=pad, num_dn_group_2=groups, pad_size_2=pad))


def _xyxy(b):
    cx, cy, w, h = b.split((1, 1, 1, 1), dim=-1)
    return torch.cat([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


def _focal(pred, labels, weight, avg, alpha=0.25, gamma=2.0, lw=2.0):
    C = pred.size(1)
    target = F.one_hot(labels, num_classes=C + 1)[:, :C].type_as(pred)
    p = pred.sigmoid()
    pt = (1 - p) * target + p * (1 - target)
    fw = (alpha * target + (1 - alpha) * (1 - target)) * pt.pow(gamma)
    return lw * (F.binary_cross_entropy_with_logits(pred, target, reduction="none") * fw * weight.view(-1, 1)).sum() / avg


def _giou(p, g, w, avg, eps=1e-6, lw=2.0):
    if not torch.any(w > 0):
        return (p * w).sum()
    a1 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    a2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    wh = (torch.min(p[:, 2:], g[:, 2:]) - torch.max(p[:, :2], g[:, :2])).clamp(min=0)
    ov = wh[:, 0] * wh[:, 1]
    e = p.new_tensor([eps])
    u = torch.max(a1 + a2 - ov, e)
    ewh = (torch.max(p[:, 2:], g[:, 2:]) - torch.min(p[:, :2], g[:, :2])).clamp(min=0)
    en = torch.max(ewh[:, 0] * ewh[:, 1], e)
    return lw * ((1 - (ov / u - (en - u) / en)) * w.mean(-1)).sum() / avg


def _reg(bp, bt, bw, factors, avg):
    l1 = lambda a, b, w: 5.0 * ((a - b).abs() * w).sum() / avg  # noqa: E731
    iou = _giou(_xyxy(bp) * factors, _xyxy(bt) * factors, bw, avg)
    return l1(bp, bt, bw), iou, l1(bp[..., :2], bt[..., :2], bw[..., :2]), l1(bp[..., 2:], bt[..., 2:], bw[..., 2:])


def _factors(bbox_preds, metas):
    fs = []
    for m, bp in zip(metas, bbox_preds):
        h, w, _ = m["img_shape"]
        fs.append(bp.new_tensor([w, h, w, h]).unsqueeze(0).repeat(bp.size(0), 1))
    return torch.cat(fs, 0)


def ref_loss(h, all_cls, all_box, enc_cls, enc_box, dn_cls, dn_box, gts, labs, metas, dn_meta):
    from semi_detr_amd import get_targets
    out = {}

    def single(cls, box, labels_list):
        B = cls.size(0)
        t = get_targets(h, list(cls), list(box), gts, labels_list, None, metas)
        labels, lw, bt, bw = (torch.cat(x, 0) for x in t[:4])
        C = cls.size(-1)
        loss_cls = _focal(cls.reshape(-1, C), labels, lw, max(t[4] * 1.0, 1))
        avg = bw.new_tensor([len(torch.nonzero(bw.sum(-1) > 0, as_tuple=False).squeeze().unique())])
        avg = torch.clamp(avg, min=1).item()
        return (loss_cls,) + _reg(box.reshape(-1, 4), bt, bw, _factors(box, metas), avg)

    def single_dn(cls, box):
        single_pad, scalar = dn_meta["pad_size"] // dn_meta["num_dn_group"], dn_meta["num_dn_group"]
        L, LW, BT, BW, npos = [], [], [], [], 0
        for bp, g, lab, m in zip(box, gts, labs, metas):
            if len(lab) > 0:
                tt = torch.arange(0, len(lab)).long().cuda().unsqueeze(0).repeat(scalar, 1)
                tgt = tt.flatten()
                out_idx = ((torch.tensor(range(scalar)) * single_pad).long().cuda().unsqueeze(1) + tt).flatten()
            else:
                out_idx = tgt = torch.tensor([]).long().cuda()
            labels = lab.new_full((single_pad * scalar,), h.num_classes, dtype=torch.long)
            labels[out_idx] = lab[tgt].long()
            lw = lab.new_ones(single_pad * scalar) if out_idx.size(0) > 0 else lab.new_zeros(single_pad * scalar)
            bt, bw = torch.zeros_like(bp), torch.zeros_like(bp)
            bw[out_idx] = 1.0
            ih, iw, _ = m["img_shape"]
            n = g[tgt, :] / bp.new_tensor([iw, ih, iw, ih]).unsqueeze(0)
            bt[out_idx] = torch.cat([(n[:, :2] + n[:, 2:]) / 2, n[:, 2:] - n[:, :2]], -1)
            L.append(labels), LW.append(lw.float()), BT.append(bt), BW.append(bw)
            npos += out_idx.numel()
        labels, lw, bt, bw = (torch.cat(x, 0) for x in (L, LW, BT, BW))
        C = cls.size(-1)
        loss_cls = _focal(cls.reshape(-1, C), labels, lw, max(npos * 1.0, 1))
        avg = torch.clamp(loss_cls.new_tensor([npos]), min=1).item()
        return (loss_cls,) + _reg(box.reshape(-1, 4), bt, bw, _factors(box, metas), avg)

    names = ("loss_cls", "loss_bbox", "loss_iou", "loss_bbox_xy", "loss_bbox_hw")
    dec = [single(c, b, labs) for c, b in zip(all_cls, all_box)]
    dn = [single_dn(c, b) for c, b in zip(dn_cls, dn_box)]
    enc = single(enc_cls, enc_box, [torch.zeros_like(l) for l in labs])
    out.update({"enc_" + k: v for k, v in zip(names, enc)})
    out.update({k: v for k, v in zip(names, dec[-1])})
    out.update({"dn_" + k: v for k, v in zip(names, dn[-1])})
    for i, (d, n) in enumerate(zip(dec[:-1], dn[:-1])):
        out.update({f"d{i}.{k}": v for k, v in zip(names, d)})
        out.update({f"d{i}.dn_{k}": v for k, v in zip(names, n)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=("new", "ref"), default=None)
    a = ap.parse_args()
    import semi_detr_amd as s
    h = make_head()
    for B, tag in ((4, "unsup"), (1, "sup")):
        d = make_inputs(1, B=B)
        args = (d["out_cls"][:, :, 200:], d["out_box"][:, :, 200:], d["enc_cls"], d["enc_box"], d["out_cls"][:, :, :200],
                d["out_box"][:, :, :200], d["gts"], d["labs"], d["metas"], d["dn_meta"])
        paths = {"new": lambda: s.loss_set(h, *args[:8], None, *args[8:]), "ref": lambda: ref_loss(h, *args)}
        for name, fn in paths.items():
            if a.only and name != a.only:
                continue
            for _ in range(3):
                sum(fn().values()).backward()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.iters):
                sum(fn().values()).backward()
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3 / a.iters
            print(json.dumps(dict(shape=tag, B=B, path=name, wall_ms=round(wall, 3),
                                  event_ms=round(e0.elapsed_time(e1) / a.iters, 3), iters=a.iters)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the de-noising / consistency query builders at SSOD shapes on the GPU against the reference's op sequence restated
with torch on the same GPU (tests/dn_torch_restated.py: the baseline is that sequence, never the new code itself).

    python tools/dn_query_probe.py [--calls 100]          wall time per call (after warm-up), both sides
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o dn -- python tools/dn_query_probe.py --trace
    python tools/dn_query_probe.py --count DIR            kernels per call from that trace

``--trace`` runs one call of each of the six targets, separated by a marker launch (the flat EMA kernel), so that the
trace splits into the targets' kernels.  B = 4 images of 10..30 boxes, 900 queries, hidden 256, dn_number 100; RoIAlign
and the projector are stubs on both sides (they are calls of the caller in both).
"""
import argparse
import csv
import glob
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("prepare_for_cdn", "prepare_for_cdn_plus", "prepare_unsup_cdn")


def targets(B=4, H=256, nq=900, seed=0):
    import dn_torch_restated as T
    import semi_detr_amd as s
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    counts = [int(x) for x in rng.integers(10, 31, B)]
    labs = [torch.from_numpy(rng.integers(0, 80, n)).to(dev) for n in counts]
    boxes = [torch.from_numpy(np.concatenate([rng.random((n, 2)) * 0.6 + 0.2, rng.random((n, 2)) * 0.3 + 0.02], 1)
                              .astype(np.float32)).to(dev) for n in counts]
    pix = [torch.cat([b[:, :2] * 500, b[:, :2] * 500 + b[:, 2:] * 400 + 2], 1).contiguous() for b in boxes]
    det = [torch.cat([p, p[:, :1]], 1).contiguous() for p in pix]
    shapes = [(800, 1200, 3)] * B
    enc = torch.nn.Embedding(81, H).to(dev)
    t = {"labels": labs, "boxes": boxes}
    args = (t, 100, 0.5, 1.0)
    groups = 200 // (2 * max(counts))
    K = 2 * groups * sum(counts)
    rows = torch.randn(5 * sum(counts), H, device=dev)
    img = torch.zeros(B, 3, 8, 8, device=dev)
    info = {"img": img, "img_metas": [{"img_shape": sh} for sh in shapes]}
    head = types.SimpleNamespace(warm_up_step=100, label_enc=enc)
    self = types.SimpleNamespace(curr_step=3, student=types.SimpleNamespace(bbox_head=head),
                                 teacher=types.SimpleNamespace(extract_feat=lambda im: None),
                                 prepare_feats=lambda f, m: (f, None, None), roi_extractor=lambda f, r: None,
                                 projector=lambda x: rows)

    def base_cdn(standin):
        u = torch.rand(K * 10 + (B if standin else 0), device=dev)
        return T.cdn(labs, boxes, enc.weight, u, 100, 0.5, 1.0, nq, 80, standin)

    def base_unsup():
        qb1, bid, mp, lw, rois = T.consistency(pix, det, shapes, shapes, img)
        ql1 = torch.zeros(5 * max(counts), H).to(dev).repeat(B, 1, 1)
        ql1[(bid.long(), mp)] = rows
        u = torch.rand(K * 10 + B, device=dev)
        return T.cdn(labs, boxes, enc.weight, u, 100, 0.5, 1.0, nq, 80, True, pad1=5 * max(counts), single1=max(counts)), ql1, qb1

    new = {"prepare_for_cdn": lambda: s.prepare_for_cdn(args, True, nq, 80, H, enc),
           "prepare_for_cdn_plus": lambda: s.prepare_for_cdn_plus(args, True, nq, 80, H, enc),
           "prepare_unsup_cdn": lambda: s.prepare_unsup_cdn(self, info, info, pix, labs, det, labs, dn_args=args, hidden_dim=H,
                                                            num_queries=nq)}
    base = {"prepare_for_cdn": lambda: base_cdn(False), "prepare_for_cdn_plus": lambda: base_cdn(True),
            "prepare_unsup_cdn": base_unsup}
    return new, base, counts


def wall(fn, calls, warmup=10):
    with torch.no_grad():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def count(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
    segs, cur = [], None
    for r in rows:
        if "ema" in r["Kernel_Name"]:
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None:
            cur.append(r["Kernel_Name"])
    order = [f"{side} {n}" for n in NAMES for side in ("hip", "torch restatement")]
    for name, seg in zip(order, segs):
        print(f"{name:40s} {len(seg):4d} kernels per call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count", metavar="DIR")
    a = ap.parse_args()
    if a.count:
        return count(a.count)
    import semi_detr_amd as s
    new, base, counts = targets()
    if a.trace:
        mark = torch.zeros(64, device="cuda:0")
        with torch.no_grad():
            for n in NAMES:                      # warm-up: allocator, lazy initialisation
                new[n](), base[n]()
            for n in NAMES:
                for side in (new, base):
                    s.ema_update_flat_(mark, mark, 0.5)
                    side[n]()
            s.ema_update_flat_(mark, mark, 0.5)
        torch.cuda.synchronize()
        return
    print(f"{torch.cuda.get_device_name(0)}; B = {len(counts)}, boxes per image {counts}, 900 queries, hidden 256; "
          f"{a.calls} calls after 10 warm-up calls, wall time per call incl. the final synchronize")
    for n in NAMES:
        t_new, t_base = wall(new[n], a.calls), wall(base[n], a.calls)
        print(f"{n:24s} hip {t_new:8.1f} us   torch restatement {t_base:8.1f} us   ratio {t_base / t_new:5.1f}x")


if __name__ == "__main__":
    main()

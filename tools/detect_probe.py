#!/usr/bin/env python
"""Time the evaluation-time decode at DINO's shapes on the GPU against the reference's op sequence restated with torch on the
same GPU in the same process (tests/detect_torch_restated.py, checked bit for bit against the reference's fixture by
tests/test_detect_ref.py: the baseline is that sequence, never the new code itself).

    python tools/detect_probe.py [--calls 200] [--out profiles/detect_probe.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/detect_probe.py --launches hip|torch      (a run of its own)

Q = 900, C = 80, k = 300, B in {1, 4}, mixed image shapes, rescale on.  Two segments, each timed on both sides, alternating:
    get_bboxes          the result list on the device
    detection_results   + bbox2result: per-class numpy arrays on the host
Wall time per call over ``--calls`` calls after warm-up, host clock around work that ends in a synchronise (detection_results
ends in its own event wait / ``.cpu()``); best of ``--rounds`` alternating rounds, and the spread between the rounds is
printed.  ``--launches SIDE`` runs 10 calls of every segment of one side and nothing else, for the kernel trace to count.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(800, 1199, 3), (1333, 750, 3), (800, 1333, 3), (1024, 1024, 3)]
SCALES = [(1.873438, 1.873536), (1.5625, 1.5621094), (2.0828125, 2.0833333), (1.6, 1.6)]
Q, C, K = 900, 80, 300


def segments(B, dev):
    import detect_torch_restated as T
    import semi_detr_amd as s
    g = torch.Generator(device=dev).manual_seed(B)
    cls = torch.randn(6, B, Q, C, device=dev, generator=g) * 2 - 3
    box = torch.rand(6, B, Q, 4, device=dev, generator=g)
    metas = [dict(img_shape=SHAPES[b], scale_factor=np.asarray(SCALES[b] * 2, np.float32)) for b in range(B)]
    hip = {"get_bboxes": lambda: s.get_bboxes(cls, box, metas, rescale=True, max_per_img=K),
           "detection_results": lambda: s.detection_results(cls, box, metas, C, rescale=True, max_per_img=K)}
    base = {"get_bboxes": lambda: T.get_bboxes(cls, box, metas, True, K),
            "detection_results": lambda: T.detection_results(cls, box, metas, C, True, K)}
    return hip, base


def wall(fn, calls, warmup=20, min_seconds=0.25):
    """us per call over at least ``calls`` calls AND at least ``min_seconds`` of work."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    calls = max(calls, int(min_seconds / max((time.perf_counter() - t0) / 10, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--launches", choices=("hip", "torch"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_probe: needs a GPU (no timing is taken on the CPU)")
    dev = torch.device("cuda:0")
    if a.launches:
        for B in (1, 4):
            hip, base = segments(B, dev)
            for fn in (hip if a.launches == "hip" else base).values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
        print(f"detect_probe: 10 calls of get_bboxes and of detection_results at B = 1 and B = 4, side {a.launches}")
        return
    lines = [f"{torch.cuda.get_device_name(0)}; Q = {Q}, C = {C}, k = {K}, rescale on, mixed image shapes; wall time per call in us "
             f"over at least {a.calls} calls and at least 0.25 s after 20 warm-up calls, incl. the final synchronize; "
             f"{a.rounds} alternating rounds, min .. max (the spread between the rounds)"]
    for B in (1, 4):
        hip, base = segments(B, dev)
        for seg in ("get_bboxes", "detection_results"):
            th, tb = [], []
            for _ in range(a.rounds):
                th.append(wall(hip[seg], a.calls))
                tb.append(wall(base[seg], a.calls))
            spread = max(max(th) - min(th), max(tb) - min(tb))
            verdict = "no slower" if min(th) <= min(tb) + spread else "SLOWER"
            lines.append(f"B={B} {seg:18s} hip {min(th):8.1f} .. {max(th):8.1f}   torch restatement {min(tb):8.1f} .. {max(tb):8.1f}   "
                         f"ratio {min(tb) / min(th):5.2f}x   spread {spread:6.1f}   {verdict}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

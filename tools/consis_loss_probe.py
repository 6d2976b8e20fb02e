#!/usr/bin/env python
"""Time the cross-view consistency loss (forward + backward, all decoder layers) at SSOD shapes on the GPU against the
reference's op sequence restated with torch on the same GPU (tests/consis_torch_restated.py: the baseline is that sequence,
never the new code itself).

    python tools/consis_loss_probe.py [--calls 200]       wall time per call (after warm-up), both sides
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o consis -- python tools/consis_loss_probe.py --trace
    python tools/consis_loss_probe.py --count DIR         kernels per call from that trace (tracing only, no counters)

``--trace`` runs one forward + backward of each side, separated by a marker launch (the flat EMA kernel), so that the trace
splits into the two sides' kernels.  L = 6 decoder layers, B = 4 images of 10..30 pseudo boxes (K = 5 x their sum), 900 + pad
queries, D = 256; ``hs`` as the reference builds it, transposed views of (Q, B, D) buffers.  The gradient is taken with
``torch.autograd.grad`` w.r.t. the views, so that no leaf accumulation is counted on either side.
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIDES = ("hip", "torch restatement")


def targets(L=6, B=4, D=256, nq=900, seed=0):
    import consis_cases as C
    import consis_torch_restated as T
    import semi_detr_amd as s
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(seed)
    counts = [int(x) for x in rng.integers(10, 31, B)]
    bid, idx, single, pad = C.layout(counts)
    Q = pad + nq
    gen = torch.Generator(device=dev).manual_seed(seed)
    bufs1 = [torch.randn(Q, B, D, device=dev, generator=gen).requires_grad_(True) for _ in range(L)]
    bufs2 = [(0.8 * b.detach() + 0.6 * torch.randn(Q, B, D, device=dev, generator=gen)) for b in bufs1]
    hs1, hs2 = [b.transpose(0, 1) for b in bufs1], [b.transpose(0, 1) for b in bufs2]
    meta = {"pad_size_1": pad, "known_bid_1": torch.from_numpy(bid).to(dev), "map_known_indice_1": torch.from_numpy(idx).to(dev),
            "loss_weights": torch.ones(len(bid), 1, device=dev)}

    def step(fn):
        def run():
            out = fn(hs1, hs2, meta)
            total = out["consis_loss.d0"]
            for l in range(1, L):
                total = total + out[f"consis_loss.d{l}"]
            return torch.autograd.grad(total, hs1)
        return run
    return {"hip": step(s.consistency_loss), "torch restatement": step(T.consistency_loss)}, counts, len(bid), Q


def wall(fn, calls, warmup=20):
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
        if "ema_flat_kernel" in r["Kernel_Name"]:
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None:
            cur.append((r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    for name, seg in zip(SIDES, segs):
        print(f"{name:20s} {len(seg):4d} kernels per call (forward + backward), {sum(t for _, t in seg) / 1e3:7.1f} us of kernel time")
        names = {}
        for k, t in seg:
            k = k.replace("void ", "").replace("(anonymous namespace)::", "").replace("at::native::", "")[:80]
            n, tt = names.get(k, (0, 0))
            names[k] = (n + 1, tt + t)
        for k, (n, t) in sorted(names.items(), key=lambda kv: -kv[1][1])[:6 if name != "hip" else 20]:
            print(f"    {n:4d} x {t / n / 1e3:6.1f} us  {k}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count", metavar="DIR")
    a = ap.parse_args()
    if a.count:
        return count(a.count)
    import semi_detr_amd as s
    fns, counts, K, Q = targets()
    if a.trace:
        mark = torch.zeros(64, device="cuda:0")
        for side in SIDES:                       # warm-up: allocator, lazy initialisation
            fns[side](), fns[side]()
        for side in SIDES:
            s.ema_update_flat_(mark, mark, 0.5)
            fns[side]()
        s.ema_update_flat_(mark, mark, 0.5)
        torch.cuda.synchronize()
        return
    print(f"{torch.cuda.get_device_name(0)}; L = 6, B = {len(counts)}, pseudo boxes per image {counts}, K = {K}, Q = {Q}, D = 256; "
          f"forward + backward, {a.calls} calls after 20 warm-up calls, wall time per call incl. the final synchronize")
    t = {side: wall(fns[side], a.calls) for side in SIDES}
    t2 = {side: wall(fns[side], a.calls) for side in SIDES}          # a second pass: the spread between the two is the noise
    for side in SIDES:
        print(f"{side:20s} {t[side]:8.1f} us   (second pass {t2[side]:8.1f} us)")
    print(f"ratio torch restatement / hip: {t['torch restatement'] / t['hip']:.1f}x, {t2['torch restatement'] / t2['hip']:.1f}x")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time one forward + backward of ``semi_detr_amd.pyramid_inputs`` against the stock op-by-op chain
(tests/pyramid_inputs_torch_restated.py) on the benchmark's pyramids -- four and five levels, bs 4 and bs 1, mixed image sizes --
and count the launches of each side.

    python tools/pyramid_inputs_probe.py --out profiles/pyramid_inputs_probe.txt

Both sides get the same image sizes, settings and ``level_embed`` and return the same tensors (``pos`` with the level row,
``mask_flatten``, valid ratios, the encoder's reference points); backward is the gradient of ``level_embed`` from a given
upstream gradient of ``pos``.  Timing: events on the stream around ``--calls`` calls, ``--blocks`` blocks per side interleaved
(torch, hip, torch, hip, ...), the upstream gradient rotating over ``--rotate`` (>= 4) tensors; us per call: median of the
blocks (min .. max).  Kernels per call are counted with torch.profiler in a pass of their own.
The bar: hip < torch - 2 x the spread (max - min over the blocks) of torch.  Next to it: the share of the HBM store rate the
``pos`` write reaches if the whole forward + backward time is charged to it (a lower bound of the emit kernel's own rate).
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INPUT = (800, 1333)
PYRAMID4 = [(100, 167), (50, 84), (25, 42), (13, 21)]
IMAGES = [(800, 1333), (800, 1201), (704, 1333), (640, 959)]                 # mixed sizes inside one padded batch
SHAPES = {"N=4, 4 levels": (4, PYRAMID4), "N=1, 4 levels": (1, PYRAMID4), "N=4, 5 levels": (4, PYRAMID4 + [(7, 11)]),
          "N=1, 5 levels": (1, PYRAMID4 + [(7, 11)])}
ENC = dict(num_feats=128, temperatureH=20, temperatureW=20, normalize=True)


def call(side, n, levels, le, g):
    le = le.detach().requires_grad_(True)
    if side == "torch":
        import pyramid_inputs_torch_restated as T
        out = T.chain_from_sizes(IMAGES[:n], INPUT, levels, T.SineEncodingHW(**ENC), le, le.device)
        pos, rest = out["pos"], (out["mask_flatten"], out["valid_ratios"], out["reference_points"])
    else:
        P = importlib.import_module("semi_detr_amd.pyramid_inputs")
        res = P.pyramid_inputs(IMAGES[:n], INPUT, levels, P.SinePositionalEncodingHW(**ENC), level_embed=le, want_reference_points=True,
                               device=le.device)
        pos, rest = res.pos, (res.mask_flatten, res.valid_ratios, res.reference_points)
    return (pos,) + rest, torch.autograd.grad([pos], [le], [g])[0]


def timed(side, n, levels, le, gs, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        call(side, n, levels, le, gs[i % len(gs)])
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def store_rate(shape, dev, calls=20):
    """TB/s of ``fill_`` on (N, S, 256) fp32 tensors, 4 rotating: a pure store stream"""
    outs = [torch.empty(shape, device=dev) for _ in range(4)]
    for o in outs:
        o.fill_(1.0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        outs[i % 4].fill_(1.0)
    stop.record()
    stop.synchronize()
    return outs[0].numel() * 4 * calls / (start.elapsed_time(stop) * 1e-3) / 1e12


def kernels_per_call(side, n, levels, le, g):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(side, n, levels, le, g)
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                key = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:48]
                names[key] = names.get(key, 0) + 1
        return (sum(names.values()), names) if names else None
    except Exception as exc:                                      # the measurement is optional; the timing is not
        print("profiler:", exc)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rotate >= 4, "at least four upstream gradients, so that they come from HBM"
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/pyramid_inputs_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: pyramid masks, sine "
             f"position rows + level row, valid ratios, encoder reference points, forward + backward; {a.calls} calls x {a.blocks} "
             f"interleaved blocks, {a.rotate} rotating upstream gradients; us per call: median of the blocks (min .. max)"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for label, (n, levels) in SHAPES.items():
        rows = sum(h * w for h, w in levels)
        g = torch.Generator(device="cpu").manual_seed(len(label))
        le = torch.randn(len(levels), 256, generator=g).to(dev)
        gs = [torch.randn(n, rows, 256, generator=g).to(dev) for _ in range(a.rotate)]
        tb = store_rate((n, rows, 256), dev)
        (o_t, g_t), (o_h, g_h) = call("torch", n, levels, le, gs[0]), call("hip", n, levels, le, gs[0])
        equal = [bool(torch.equal(x, y)) for x, y in zip(o_t, o_h)]
        gdiff = float((g_t - g_h).abs().max() / g_t.abs().max())
        t = {k: [] for k in ("torch", "hip")}
        for k in t:
            timed(k, n, levels, le, gs, 5)
        for _ in range(a.blocks):
            for k in t:
                t[k].append(timed(k, n, levels, le, gs, a.calls))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = max(t["torch"]) - min(t["torch"])
        verdict = "kept" if med["hip"] < med["torch"] - 2 * spread else "MISSES the bar"
        pos_bytes = n * rows * 1024
        lines.append(f"{label}: {n} x {rows} x 256; bit-equal to the stock chain: pos {equal[0]}, mask_flatten {equal[1]}, valid_ratios "
                     f"{equal[2]}, reference_points {equal[3]}; max |d level_embed, torch - hip| / max |torch| {gdiff:.2e}")
        lines.append(f"  forward + backward  stock chain {med['torch']:9.1f} ({min(t['torch']):.1f} .. {max(t['torch']):.1f})   "
                     f"hip {med['hip']:9.1f} ({min(t['hip']):.1f} .. {max(t['hip']):.1f})   stock / hip = {med['torch'] / med['hip']:.2f}   "
                     f"{verdict} (hip < stock - 2 x stock's spread {spread:.1f});  pos store: {pos_bytes / 2 ** 20:.1f} MiB, "
                     f"{pos_bytes / med['hip'] / 1e6:.3f} TB/s if the whole call is charged to it = "
                     f"{100 * pos_bytes / med['hip'] / 1e6 / tb:.0f} % of fill_'s {tb:.2f} TB/s in this run")
        print("\n".join(lines[-2:]), flush=True)
        flush()
        for k in ("torch", "hip"):
            got = kernels_per_call(k, n, levels, le, gs[0])
            if got is None:
                lines.append(f"{label}: kernels per call, {k}: not measured (the profiler gave no device events)")
            else:
                top = ", ".join(f"{c} x {nm}" for nm, c in sorted(got[1].items(), key=lambda kv: -kv[1])[:8])
                lines.append(f"{label}: kernels per call (forward + backward), {k}: {got[0]}   [{top}{', ...' if len(got[1]) > 8 else ''}]")
            print(lines[-1], flush=True)
        flush()


if __name__ == "__main__":
    main()

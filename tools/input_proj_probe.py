#!/usr/bin/env python
"""Time the norm stage of the input projection plus the layer-0 positional add on the GPU, forward + backward: through
``semi_detr_amd.group_norm_to_tokens`` (csrc/group_norm_tokens.hip) and through the stock torch ops of the restatement
(tests/input_proj_torch_restated.py: ``GroupNorm`` per level, ``flatten(2).transpose(1, 2)``, ``cat``, ``src + pos``).  The convs are
replaced by pre-computed level tensors, so nothing but the norm stage runs.

    python tools/input_proj_probe.py [--calls 30] [--out profiles/input_proj_probe.txt]

torch   tokens = cat([norm_l(x_l).flatten(2).transpose(1, 2)], 1); q = tokens + pos
hip     tokens, q = group_norm_to_tokens(xs, norms, pos)
Both ``tokens`` and ``q`` get an upstream gradient (the encoder reads both); gradients are taken w.r.t. the levels, pos and the
norms' parameters.  Shapes: the bench step's pyramid (levels 100x134, 50x67, 25x34, 13x17) at N = 4 and N = 1 and the five-level
one (a 7x9 level more), in fp32 and with bf16 levels under autocast.  Timed with device events over ``--calls`` calls after a
warm-up, the two sides alternating in ``--blocks`` blocks; every call takes the next of ``--rotate`` (>= 4) input sets, so the
tensors come from HBM.  Algorithmic bytes: forward reads x twice and pos once and writes tokens and q; backward reads gy, gq
and x twice each and writes dx.  The copy rate is a ``copy_`` of the token tensor in the same run.  Kernels per call are counted
with torch.profiler in a pass of their own.
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D = 256
PYRAMID4 = [(100, 134), (50, 67), (25, 34), (13, 17)]
SHAPES = {"N=4, 4 levels": (4, PYRAMID4), "N=1, 4 levels": (1, PYRAMID4), "N=4, 5 levels": (4, PYRAMID4 + [(7, 9)])}


def norms(n, dev):
    torch.manual_seed(0)
    out = [nn.GroupNorm(32, D).to(dev) for _ in range(n)]
    with torch.no_grad():
        for m in out:
            m.weight.normal_(1.0, 0.2)
            m.bias.normal_(0.0, 0.2)
    return out


def glue(side, gn, xs, pos):
    if side == "torch":
        import input_proj_torch_restated as T
        return list(T.norm_tokens(xs, gn, pos))
    from semi_detr_amd import group_norm_to_tokens
    return list(group_norm_to_tokens(xs, gn, pos)[0])


def call(side, gn, ins, seeds, autocast):
    ins = [t.detach().requires_grad_(True) for t in ins]
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        outs = glue(side, gn, ins[:-1], ins[-1])
    params = [p for m in gn for p in (m.weight, m.bias)]
    return outs, torch.autograd.grad(outs, ins + params, seeds)


def timed(side, gn, sets, calls, autocast):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        call(side, gn, *sets[i % len(sets)], autocast)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def copy_rate(shape, dev, calls=20):
    """TB/s of ``dst.copy_(src)`` on (N, S, 256) fp32 tensors, 4 rotating pairs: read + write"""
    pairs = [(torch.randn(shape, device=dev), torch.empty(shape, device=dev)) for _ in range(4)]
    for s, d in pairs:
        d.copy_(s)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        s, d = pairs[i % 4]
        d.copy_(s)
    stop.record()
    stop.synchronize()
    return 2 * pairs[0][0].numel() * 4 * calls / (start.elapsed_time(stop) * 1e-3) / 1e12


def kernels_per_call(side, gn, sets, autocast):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(side, gn, *sets[0], autocast)
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
    assert a.rotate >= 4, "at least four input sets, so that the tensors come from HBM"
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/input_proj_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: GroupNorm of the input "
             f"projection -> tokens, + pos, forward + backward; {a.calls} calls x {a.blocks} alternating blocks, {a.rotate} rotating "
             "input sets; us per call: median of the blocks (min .. max)"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    counted = []
    for label, (n, levels) in SHAPES.items():
        rows = sum(h * w for h, w in levels)
        gn = norms(len(levels), dev)
        tb = copy_rate((n, rows, D), dev)
        for autocast in (False, True):
            g = torch.Generator(device="cpu").manual_seed(len(label))
            xdt = torch.bfloat16 if autocast else torch.float32
            sets = [([torch.randn((n, D) + hw, generator=g).to(dev).to(xdt) for hw in levels] + [torch.randn(n, rows, D, generator=g).to(dev)],
                     [torch.randn(n, rows, D, generator=g).to(dev) for _ in range(2)]) for _ in range(a.rotate)]
            o_t, g_t = call("torch", gn, *sets[0], autocast)
            o_h, g_h = call("hip", gn, *sets[0], autocast)
            diff = max(float((x.detach().float() - y.detach().float()).abs().max() / x.detach().float().abs().max())
                       for x, y in zip(list(o_t) + list(g_t), list(o_h) + list(g_h)))
            t = {k: [] for k in ("torch", "hip")}
            for k in t:
                timed(k, gn, sets, 5, autocast)
            for _ in range(a.blocks):
                for k in t:
                    t[k].append(timed(k, gn, sets, a.calls, autocast))
            med = {k: float(np.median(v)) for k, v in t.items()}
            xb = 2 if autocast else 4
            alg = n * rows * D * ((2 * xb + 4 + 8) + (2 * 4 + 2 * 4 + 2 * xb + xb))      # forward + backward, bytes
            spread = max(t["torch"]) - min(t["torch"])
            verdict = "within the bar" if med["hip"] <= med["torch"] + spread else "MISSES the bar"
            tag = "bf16 x under autocast" if autocast else "fp32"
            lines.append(f"{label}, {tag}: {n} x {rows} x {D}; largest max |torch - hip| / max |torch| over outputs and gradients {diff:.2e}")
            lines.append(f"  forward + backward  torch restatement {med['torch']:9.1f} ({min(t['torch']):.1f} .. {max(t['torch']):.1f})   "
                         f"hip {med['hip']:9.1f} ({min(t['hip']):.1f} .. {max(t['hip']):.1f})   torch / hip = {med['torch'] / med['hip']:.2f}   "
                         f"hip: {alg / med['hip'] / 1e6:.2f} TB/s of {alg / 2 ** 20:.0f} MiB algorithmic; copy_ in this run {tb:.2f} TB/s; "
                         f"{verdict} (hip <= torch + torch's spread {spread:.1f})")
            print("\n".join(lines[-2:]), flush=True)
            flush()
            if n == 4 and len(levels) == 4:
                counted.append((f"{label}, {tag}", gn, sets, autocast))
    for label, gn, sets, autocast in counted:
        for k in ("torch", "hip"):
            got = kernels_per_call(k, gn, sets, autocast)
            if got is None:
                lines.append(f"{label}: kernels per call, {k}: not measured (the profiler gave no device events)")
            else:
                top = ", ".join(f"{c} x {nm}" for nm, c in sorted(got[1].items(), key=lambda kv: -kv[1]))
                lines.append(f"{label}: kernels per call (forward + backward), {k}: {got[0]}   [{top}]")
            print(lines[-1], flush=True)
        flush()


if __name__ == "__main__":
    main()

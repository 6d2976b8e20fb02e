#!/usr/bin/env python
"""Time the reference-point chain of one six-layer decoder pass on the GPU, forward + backward and forward only under
``no_grad``: through ``semi_detr_amd.ref_points`` (csrc/ref_points.hip) and through the stock torch ops of the restatement
(tests/ref_points_torch_restated.py).  The decoder layers and the ``fc_reg`` GEMMs are replaced by pre-computed deltas, so
nothing but the chain runs.

    python tools/ref_points_probe.py [--calls 100] [--out profiles/ref_points_probe.txt]

The chain (detr_od/models/utils/transformer.py:972-987, 1029-1036; dino_detr_ssod_head.py:393-398):
  in front of layer 0      sigmoid, valid-ratio scaling, sine embed                      1 launch   (hip, forward)
  between two layers       refine through inverse_sigmoid, detach, scaling, sine embed   5 launches
  after the last layer     refine                                                        1 launch
  the head                 the six layers' refine again -> outputs_coord                 1 launch of 6 segments
Upstream gradients arrive at layer 0's ``reference_points_input`` and embedding, at the last reference points and at
``outputs_coord``; gradients are taken w.r.t. ``refpoints_unsigmoid`` and all deltas (the points of layers >= 1 are detached,
so their scaling and embedding have no backward, on either side).  Shapes: (nq, bs) = (1100, 4) and (900, 1), 4 levels, fp32.
Timed with device events over ``--calls`` calls after a warm-up, the two sides alternating in ``--blocks`` blocks; every call
takes the next of ``--rotate`` (>= 4) input sets.  Kernels per call are counted with torch.profiler in a pass of their own.
The bar: hip <= torch + the spread (max - min over the blocks) of torch.
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

LAYERS, LEVELS = 6, 4
SHAPES = {"nq 1100, bs 4": (1100, 4), "nq 900, bs 1": (900, 1)}
IDENT = [nn.Identity()] * LAYERS


def chain(side, unsig, deltas, head_deltas, vr):
    """-> (everything the pass computes, the outputs an upstream gradient arrives at)"""
    if side == "torch":
        import ref_points_torch_restated as T
        ref = unsig.sigmoid()
        refs, inputs = [ref], []
        for l in range(LAYERS):
            inputs += list(T.reference_inputs(ref, vr))
            new = T.refine(deltas[l], ref)
            ref = new.detach()
            refs.append(new)
        coord = T.box_outputs(IDENT, head_deltas, [r.transpose(0, 1) for r in refs])
    else:
        from semi_detr_amd import box_outputs
        from semi_detr_amd import ref_points as P
        ref, ref_input, embed = P._apply(P.SIGMOID, 0.0, vr, True, False, False, None, [unsig], "probe")
        refs, inputs = [ref], [ref_input.transpose(0, 1), embed]
        for l in range(LAYERS):
            if l + 1 < LAYERS:
                new, ref_input, embed = P._apply(P.REFINE, 1e-5, vr, True, True, False, [deltas[l]], [ref], "probe")
                inputs += [ref_input.transpose(0, 1), embed]
            else:
                new = P._apply(P.REFINE, 1e-5, None, False, False, False, [deltas[l]], [ref], "probe")[0]
            ref = new.detach()
            refs.append(new)
        coord = box_outputs(IDENT, head_deltas, [r.transpose(0, 1) for r in refs])
    return inputs + refs + [coord], [inputs[0], inputs[1], refs[-1], coord]


def call(side, ins, seeds, train):
    unsig, deltas, head_deltas, vr = ins
    if not train:
        with torch.no_grad():
            return chain(side, unsig, deltas, head_deltas, vr)[0], []
    leaves = [t.detach().requires_grad_(True) for t in [unsig] + deltas + head_deltas]
    everything, outs = chain(side, leaves[0], leaves[1:1 + LAYERS], leaves[1 + LAYERS:], vr)
    return everything, torch.autograd.grad(outs, leaves, seeds)


def timed(side, sets, calls, train):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        call(side, *sets[i % len(sets)], train)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def kernels_per_call(side, sets, train):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(side, *sets[0], train)
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                key = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:40]
                names[key] = names.get(key, 0) + 1
        return (sum(names.values()), names) if names else None
    except Exception as exc:                                      # the count is optional; the timing is not
        print("profiler:", exc)
        return None


def make_set(nq, bs, g, dev):
    unsig = torch.randn(nq, bs, 4, generator=g).to(dev)
    deltas = [(0.1 * torch.randn(nq, bs, 4, generator=g)).to(dev) for _ in range(LAYERS)]
    head_deltas = [(0.1 * torch.randn(bs, nq, 4, generator=g)).to(dev) for _ in range(LAYERS)]
    vr = (0.5 + 0.5 * torch.rand(bs, LEVELS, 2, generator=g)).to(dev)
    seeds = [torch.randn(nq, bs, LEVELS, 4, generator=g).to(dev), torch.randn(nq, bs, 512, generator=g).to(dev),
             torch.randn(nq, bs, 4, generator=g).to(dev), torch.randn(LAYERS, bs, nq, 4, generator=g).to(dev)]
    return (unsig, deltas, head_deltas, vr), seeds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rotate >= 4, "at least four input sets"
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/ref_points_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: the reference-point chain "
             f"of one {LAYERS}-layer decoder pass + the head's coordinate loop; {a.calls} calls x {a.blocks} alternating blocks, "
             f"{a.rotate} rotating input sets; us per call: median of the blocks (min .. max)"]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for label, (nq, bs) in SHAPES.items():
        g = torch.Generator(device="cpu").manual_seed(nq)
        sets = [make_set(nq, bs, g, dev) for _ in range(a.rotate)]
        for train in (True, False):
            o_t, g_t = call("torch", *sets[0], train)
            o_h, g_h = call("hip", *sets[0], train)
            diff = max(float((x.detach() - y.detach()).abs().max() / x.detach().abs().max())
                       for x, y in zip(list(o_t) + list(g_t), list(o_h) + list(g_h)))
            t = {k: [] for k in ("torch", "hip")}
            for k in t:
                timed(k, sets, 5, train)
            for _ in range(a.blocks):
                for k in t:
                    t[k].append(timed(k, sets, a.calls, train))
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = max(t["torch"]) - min(t["torch"])
            verdict = "within the bar" if med["hip"] <= med["torch"] + spread else "MISSES the bar"
            tag = "forward + backward" if train else "forward, no_grad"
            lines.append(f"{label}, {tag}: largest max |torch - hip| / max |torch| over outputs and gradients {diff:.2e}")
            lines.append(f"  torch restatement {med['torch']:9.1f} ({min(t['torch']):.1f} .. {max(t['torch']):.1f})   "
                         f"hip {med['hip']:9.1f} ({min(t['hip']):.1f} .. {max(t['hip']):.1f})   torch / hip = {med['torch'] / med['hip']:.2f}   "
                         f"{verdict} (hip <= torch + torch's spread {spread:.1f})")
            print("\n".join(lines[-2:]), flush=True)
            for k in ("torch", "hip"):
                got = kernels_per_call(k, sets, train)
                if got is None:
                    lines.append(f"  kernels per call, {k}: not measured (the profiler gave no device events)")
                else:
                    top = ", ".join(f"{c} x {nm}" for nm, c in sorted(got[1].items(), key=lambda kv: -kv[1])[:6])
                    lines.append(f"  kernels per call, {k}: {got[0]}   [{top}{', ...' if len(got[1]) > 6 else ''}]")
                print(lines[-1], flush=True)
            flush()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the glue of one transformer layer on the GPU -- the positional add, the residual adds and the LayerNorms, forward +
backward -- through ``semi_detr_amd.add_layer_norm`` (csrc/add_norm.hip) and through the stock torch ops of the restatement
(tests/add_norm_torch_restated.py's layers: ``x + branch``, ``nn.LayerNorm``, ``x + pos``).  The GEMMs and the attentions are
replaced by pre-computed branch tensors, so nothing but the glue runs.

    python tools/add_norm_probe.py [--calls 50] [--out profiles/add_norm_probe.txt]

encoder layer, src (4, 20000, 256):      torch   x1 = norm1(src + b1); x2 = norm2(x1 + b2); q = x2 + pos
                                         hip     x1 = add_ln(b1, src); x2, q = add_ln(b2, x1, pos)
                                         (q is the query of the NEXT layer, as encoder_forward threads it: one positional add per
                                         layer on either side, and the same function, so that the results can be compared)
decoder layer, tgt (1100, 4, 256):       torch   q1 = tgt + pos; t1 = norm2(tgt + b_sa); q2 = t1 + pos; t2 = norm1(t1 + b_ca);
                                                 t3 = norm3(t2 + b_ffn); out = norm(t3)
                                         hip     q1 = tgt + pos (torch); t1, q2 = add_ln(b_sa, tgt, pos); t2 = add_ln(b_ca, t1);
                                                 t3 = add_ln(b_ffn, t2); out = add_ln(t3)
Every tensor a later GEMM or attention would read gets an upstream gradient; gradients are taken w.r.t. the layer input, pos,
the branches and the norms' parameters.  Timed with device events over ``--calls`` calls after a warm-up, the two sides
alternating in ``--blocks`` blocks; every call takes the next of ``--rotate`` (>= 4) input sets, so the tensors come from HBM.
Kernels per call are counted with torch.profiler in a pass of their own.
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 256


def norms(n, dev):
    torch.manual_seed(0)
    out = [nn.LayerNorm(D).to(dev) for _ in range(n)]
    with torch.no_grad():
        for m in out:
            m.weight.normal_(1.0, 0.2)
            m.bias.normal_(0.0, 0.2)
    return out


def encoder_glue(side, ln, src, pos, b1, b2):
    if side == "torch":
        x1 = ln[0](src + b1)
        x2 = ln[1](x1 + b2)
        return [x2 + pos, x2]
    from semi_detr_amd import add_layer_norm
    x1 = add_layer_norm(b1, src, ln[0].weight, ln[0].bias, ln[0].eps)
    x2, q = add_layer_norm(b2, x1, ln[1].weight, ln[1].bias, ln[1].eps, pos=pos)
    return [q, x2]


def decoder_glue(side, ln, tgt, pos, b_sa, b_ca, b_ffn):
    if side == "torch":
        q1 = tgt + pos
        t1 = ln[1](tgt + b_sa)
        q2 = t1 + pos
        t2 = ln[0](t1 + b_ca)
        t3 = ln[2](t2 + b_ffn)
        return [q1, q2, t3, ln[3](t3)]
    from semi_detr_amd import add_layer_norm
    q1 = tgt + pos
    t1, q2 = add_layer_norm(b_sa, tgt, ln[1].weight, ln[1].bias, ln[1].eps, pos=pos)
    t2 = add_layer_norm(b_ca, t1, ln[0].weight, ln[0].bias, ln[0].eps)
    t3 = add_layer_norm(b_ffn, t2, ln[2].weight, ln[2].bias, ln[2].eps)
    return [q1, q2, t3, add_layer_norm(t3, None, ln[3].weight, ln[3].bias, ln[3].eps)]


SHAPES = {"encoder": dict(shape=(4, 20000, D), glue=encoder_glue, inputs=4, outputs=2, norms=2),
          "decoder": dict(shape=(1100, 4, D), glue=decoder_glue, inputs=5, outputs=4, norms=4)}


def call(cfg, side, ln, ins, seeds):
    ins = [t.detach().requires_grad_(True) for t in ins]
    outs = cfg["glue"](side, ln, *ins)
    params = [p for m in ln for p in (m.weight, m.bias)]
    return outs, torch.autograd.grad(outs, ins + params, seeds)


def timed(cfg, side, ln, sets, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        ins, seeds = sets[i % len(sets)]
        call(cfg, side, ln, ins, seeds)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def kernels_per_call(cfg, side, ln, sets):
    """(number of kernels, {name: count}) of one forward + backward, or None where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            call(cfg, side, ln, *sets[0])
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                key = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:64]
                names[key] = names.get(key, 0) + 1
        return (sum(names.values()), names) if names else None
    except Exception as exc:                                      # the measurement is optional; the timing is not
        print("profiler:", exc)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rotate >= 4, "at least four input sets, so that the tensors come from HBM"
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/add_norm_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: glue of one transformer "
             f"layer, forward + backward, D = {D}; {a.calls} calls x {a.blocks} alternating blocks, {a.rotate} rotating input "
             "sets; us per call: median of the blocks (min .. max)"]

    def flush():
        text = "\n".join(lines)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")

    counted = []
    for label, cfg in SHAPES.items():
        ln = norms(cfg["norms"], dev)
        g = torch.Generator(device="cpu").manual_seed(len(label))
        shape = cfg["shape"]
        sets = [([torch.randn(shape, generator=g).to(dev) for _ in range(cfg["inputs"])],
                 [torch.randn(shape, generator=g).to(dev) for _ in range(cfg["outputs"])]) for _ in range(a.rotate)]
        mib = shape[0] * shape[1] * D * 4 / 2 ** 20
        o_t, g_t = call(cfg, "torch", ln, *sets[0])
        o_h, g_h = call(cfg, "hip", ln, *sets[0])
        diff = max(float((x.detach() - y.detach()).abs().max() / x.detach().abs().max())
                   for x, y in zip(list(o_t) + list(g_t), list(o_h) + list(g_h)))
        lines.append(f"{label} layer, {shape[0]} x {shape[1]} x {D} ({mib:.1f} MiB per tensor, {a.rotate} sets of "
                     f"{cfg['inputs'] + cfg['outputs']}): largest max |torch - hip| / max |torch| over outputs and gradients {diff:.2e}")
        t = {k: [] for k in ("torch", "hip")}
        for k in t:
            timed(cfg, k, ln, sets, 10)
        for _ in range(a.blocks):
            for k in t:
                t[k].append(timed(cfg, k, ln, sets, a.calls))
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append(f"  forward + backward  torch restatement {med['torch']:9.1f} ({min(t['torch']):.1f} .. {max(t['torch']):.1f})   "
                     f"hip {med['hip']:9.1f} ({min(t['hip']):.1f} .. {max(t['hip']):.1f})   "
                     f"torch / hip = {med['torch'] / med['hip']:.2f}")
        print("\n".join(lines[-2:]), flush=True)
        flush()
        counted.append((label, cfg, ln, sets))
    for label, cfg, ln, sets in counted:
        for k in ("torch", "hip"):
            n = kernels_per_call(cfg, k, ln, sets)
            if n is None:
                lines.append(f"{label}: kernels per call, {k}: not measured (the profiler gave no device events)")
            else:
                top = ", ".join(f"{c} x {nm}" for nm, c in sorted(n[1].items(), key=lambda kv: -kv[1]))
                lines.append(f"{label}: kernels per call (forward + backward), {k}: {n[0]}   [{top}]")
            print(lines[-1], flush=True)
        flush()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the decoder's self-attention module on the GPU: ``semi_detr_amd.MultiheadAttention`` (csrc/self_attn.hip between two
GEMMs) against ``torch.nn.MultiheadAttention`` called as the reference calls it,
``self.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]`` with ``need_weights`` left at its default
(detr_od/models/utils/transformer.py:810).  Both hold the same weights.

    python tools/self_attn_probe.py [--calls 200] [--out profiles/self_attn_probe.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sa -- python tools/self_attn_probe.py --first-only --calls 20 --blocks 1
    python tools/self_attn_probe.py --dtype bf16 [--out profiles/self_attn_h16_probe.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/self_attn_probe.py --dtype bf16 --arithmetic operand --first-only --calls 20 --blocks 1

``--dtype fp16 | bf16`` runs every arm under ``torch.autocast`` of that type on the same fp32 inputs and weights, and times three
arms: ``torch`` (``nn.MultiheadAttention``), ``hip`` (the mirror with ``arithmetic="fp32"``: exact up-cast, fp32 kernels) and
``h16`` (the mirror with ``arithmetic="operand"``: the 16-bit instances of csrc/self_attn.hip).  ``--arithmetic fp32 | operand`` keeps only that
mirror arm, for a kernel trace of its own.

Shapes: Lq = 1100 with the dn mask of dn_number = 100 (a pad of 200: 100 groups of 2) and Lq = 900 without a mask, B = 4 and
B = 1, E = 256, H = 8.  Per shape and side: forward (under ``no_grad``) and forward + backward (gradients of tgt, pos and the
weights), timed with device events over ``--calls`` calls after a warm-up, the two sides alternating in blocks so that both see
the same machine; every call takes the next of ``--rotate`` input sets (together larger than the L2), so inputs come from HBM.
Peak allocated memory of one forward + backward above what is held before the call is reported for both.  The outputs of the
two sides are compared on the way (largest difference, as a sanity line; the tests carry the bounds).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

E, H = 256, 8
FLOPS_FWD = lambda B, open_: 4.0 * B * H * open_ * 32          # noqa: E731  QK^T and PV over the open elements
SHAPES = [("Lq1100 dn mask", 1100, True), ("Lq900 no mask", 900, False)]


AUTOCAST = None                                       # the 16-bit dtype every arm runs under, None: fp32


def sides(dev, arithmetic=None):
    import semi_detr_amd as s
    torch.manual_seed(0)
    ref = torch.nn.MultiheadAttention(E, H, dropout=0.0).to(dev)
    with torch.no_grad():
        ref.in_proj_bias.normal_(0, 0.1)
    arms = {"torch": ref, "hip": s.MultiheadAttention.adopt(ref)}             # the same Parameter objects
    if AUTOCAST is not None:
        arms["h16"] = s.MultiheadAttention.adopt(ref, arithmetic="operand")
    if arithmetic is not None:
        arms = {k: m for k, m in arms.items() if getattr(m, "arithmetic", None) == arithmetic}
    return arms


def inputs(L, B, masked, rotate, dev):
    from self_attn_cases import dn_mask
    g = torch.Generator(device="cpu").manual_seed(L * 10 + B)
    sets = [tuple(torch.randn(L, B, E, generator=g).to(dev) for _ in range(3)) for _ in range(rotate)]
    mask = torch.from_numpy(dn_mask(1, 100, L - 200)).to(dev) if masked else None
    return sets, mask


def call(m, tgt, pos, mask, backward, gout):
    with torch.autocast("cuda", dtype=AUTOCAST, enabled=AUTOCAST is not None):
        return _call(m, tgt, pos, mask, backward, gout)


def _call(m, tgt, pos, mask, backward, gout):
    if not backward:
        with torch.no_grad():
            q = k = tgt + pos
            return m(q, k, tgt, attn_mask=mask)[0]
    tgt = tgt.detach().requires_grad_(True)
    q = k = tgt + pos
    out = m(q, k, tgt, attn_mask=mask)[0]
    out.backward(gout.to(out.dtype))
    return out


def timed(m, sets, mask, backward, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(calls):
        tgt, pos, gout = sets[i % len(sets)]
        call(m, tgt, pos, mask, backward, gout)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls                # microseconds per call


def peak(m, sets, mask):
    tgt, pos, gout = sets[0]
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    call(m, tgt, pos, mask, True, gout)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rotate", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--first-only", action="store_true", help="only Lq = 1100, B = 4 (for a kernel trace of one shape)")
    ap.add_argument("--dtype", choices=("fp32", "fp16", "bf16"), default="fp32", help="fp16 / bf16: every arm under autocast")
    ap.add_argument("--arithmetic", choices=("fp32", "operand"), default=None, help="only the mirror with this arithmetic")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    global AUTOCAST
    AUTOCAST = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    ms = sides(dev, a.arithmetic)
    first, rest = list(ms)[0], list(ms)[1:]
    lines = [f"# tools/self_attn_probe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: E = {E}, H = {H}, "
             f"{a.calls} calls x {a.blocks} alternating blocks, {a.rotate} rotating input sets; us per call: median of the blocks "
             "(min .. max)" + ("" if AUTOCAST is None else f"; every arm under torch.autocast({a.dtype}): torch = nn.MultiheadAttention, "
                               "hip = mirror arithmetic='fp32', h16 = mirror arithmetic='operand'")]
    for label, L, masked in SHAPES[:1] if a.first_only else SHAPES:
        for B in (4,) if a.first_only else (4, 1):
            sets, mask = inputs(L, B, masked, a.rotate, dev)
            open_ = float((~mask).sum()) if masked else float(L * L)
            outs = {k: call(m, *sets[0][:2], mask, False, None).float() for k, m in ms.items()}
            diff = ", ".join(f"|{first} - {k}| {float((outs[first] - outs[k]).abs().max()):.2e}" for k in rest)
            lines.append(f"{label}, B = {B}: open score elements {open_ / (L * L):.3f} of L^2, attention core "
                         f"{FLOPS_FWD(B, open_) / 1e9:.2f} GFLOP forward; largest difference of the output {diff}")
            for backward in (False, True):
                t = {k: [] for k in ms}
                for k in ms:                                                      # warm-up of both sides at this shape
                    timed(ms[k], sets, mask, backward, 20)
                for _ in range(a.blocks):
                    for k in ms:
                        t[k].append(timed(ms[k], sets, mask, backward, a.calls))
                med = {k: float(np.median(v)) for k, v in t.items()}
                what = "forward + backward" if backward else "forward           "
                lines.append(f"  {what}  " + "   ".join(f"{k} {med[k]:8.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f})" for k in ms) + "   "
                             + "   ".join(f"{first} / {k} = {med[first] / med[k]:.2f}" for k in rest))
            pk = {k: peak(ms[k], sets, mask) for k in ms}
            lines.append("  peak allocated by one forward + backward  " + "   ".join(f"{k} {pk[k]:.1f} MiB" for k in ms))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

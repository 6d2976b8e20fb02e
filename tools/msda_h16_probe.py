#!/usr/bin/env python
"""Time the mixed-precision MSDA op (fp16 / bf16 value map, fp32 locations and weights: semidetr_msda_forward_h16 /
semidetr_msda_backward_h16) against the AMP route it replaces, restated here: ``value.float()`` -> the fp32 op -> ``.to(dtype)``
and the matching backward through autograd -- on the same GPU, the same inputs, in the same process.

    python tools/msda_h16_probe.py [--calls 100] [--rounds 3] [--out profiles/msda_h16_probe.txt]

Shapes (8 heads x 32 channels, 4 levels of the 800 x 1333 pyramid x 4 points; S = 22 223):
    encoder  N = 4, Lq = S      queries are the pixels, samples ~ N(pixel centre, 2 px): the fp32 op runs its window kernels
    decoder  N = 4, Lq = 1100   samples anywhere on the map
    micro    N = 2, Lq = 300
each forward only (no_grad) and forward + backward, fp16 and bf16.  Wall time per call over at least ``--calls`` calls and at
least 0.25 s after 20 warm-up calls (the adaptive forward policy has settled by then), host clock around work that ends in a
synchronise; ``--rounds`` alternating rounds, min .. max, and the spread between the rounds.  The verdict column is the routing
rule of DESIGN.md 2.12: SLOWER = the new op's best round is behind the up-cast route's best by more than the spread.  In brackets:
the FORWARD kernels of the two sides (the backward runs on autograd's thread, whose last-kernels string is its own).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
M, D, P = 8, 32, 4
SHAPES = (("encoder", 4, None), ("decoder", 4, 1100), ("micro", 2, 300))


def inputs(N, Lq, dtype, dev):
    shp = np.asarray(LEVELS, np.int64)
    L, S = len(LEVELS), int((shp[:, 0] * shp[:, 1]).sum())
    g = torch.Generator(device=dev).manual_seed(11)
    tsh = torch.from_numpy(shp).to(dev)
    tls = torch.cat([tsh.new_zeros(1), (tsh[:, 0] * tsh[:, 1]).cumsum(0)[:-1]])
    if Lq is None:      # pixel queries: locations = the query's own pixel centre + N(0, 2 px) of the sampled level
        Lq = S
        cen = np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                              for h, w in LEVELS]).astype(np.float32)
        wh = torch.from_numpy(shp[:, ::-1].astype(np.float32).copy()).to(dev)
        loc = torch.from_numpy(cen).to(dev)[None, :, None, None, None, :] + \
            torch.randn(N, Lq, M, L, P, 2, device=dev, generator=g) * 2.0 / wh[None, None, None, :, None, :]
    else:
        loc = torch.rand(N, Lq, M, L, P, 2, device=dev, generator=g)
    attn = torch.softmax(torch.randn(N, Lq, M, L * P, device=dev, generator=g) * 2, -1).view(N, Lq, M, L, P)
    value = torch.randn(N, S, M, D, device=dev, generator=g).to(dtype)
    gout = torch.randn(N, Lq, M * D, device=dev, generator=g).to(dtype)
    return value, tsh, tls, loc.contiguous(), attn.contiguous(), gout


def sides(args, slot):
    import semi_detr_amd as s
    value, tsh, tls, loc, attn, gout = args

    def new_fwd():
        with torch.no_grad():
            return s.MSDeformAttnMixedFunction.apply(value, tsh, tls, loc, attn, 64)

    def old_fwd():
        with torch.no_grad():
            return s.MSDeformAttnFunction.apply(value.float(), tsh, tls, loc, attn, 64, slot).to(value.dtype)

    leaves = [t.detach().clone().requires_grad_(True) for t in (value, loc, attn)]

    def new_fb():
        out = s.MSDeformAttnMixedFunction.apply(leaves[0], tsh, tls, leaves[1], leaves[2], 64)
        return torch.autograd.grad(out, leaves, gout)

    def old_fb():
        out = s.MSDeformAttnFunction.apply(leaves[0].float(), tsh, tls, leaves[1], leaves[2], 64, slot).to(value.dtype)
        return torch.autograd.grad(out, leaves, gout)

    return {"forward": (new_fwd, old_fwd), "forward+backward": (new_fb, old_fb)}


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
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msda_h16_probe: needs a GPU (no timing is taken on the CPU)")
    import semi_detr_amd as s
    dev = torch.device("cuda:0")
    lib = s._lib.lib()
    lines = [f"{torch.cuda.get_device_name(0)}; M = {M}, D = {D}, L = {len(LEVELS)}, P = {P}, S = 22223; wall time per call in us over at "
             f"least {a.calls} calls and at least 0.25 s after 20 warm-up calls, incl. the final synchronize; {a.rounds} alternating "
             f"rounds, min .. max (the spread between the rounds); up-cast = value.float() -> fp32 op -> .to(dtype), adaptive policy"]
    slot = 200
    for shape, N, Lq in SHAPES:
        for dname, dtype in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            slot += 1
            args = inputs(N, Lq, dtype, dev)
            for seg, (new, old) in sides(args, slot).items():
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(wall(new, a.calls))
                    kn = lib.semidetr_msda_h16_last_kernels().decode()
                    to.append(wall(old, a.calls))
                    ko = lib.semidetr_msda_last_kernels().decode()
                spread = max(max(tn) - min(tn), max(to) - min(to))
                verdict = "no slower" if min(tn) <= min(to) + spread else "SLOWER"
                lines.append(f"{shape:8s} N={N} Lq={args[3].shape[1]:5d} {dname} {seg:16s} h16 {min(tn):8.1f} .. {max(tn):8.1f}   up-cast "
                             f"{min(to):8.1f} .. {max(to):8.1f}   ratio {min(to) / min(tn):5.2f}x   spread {spread:6.1f}   {verdict}   "
                             f"[{kn} | {ko}]")
                print(lines[-1], flush=True)
            del args
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

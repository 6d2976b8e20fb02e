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

    python tools/msda_h16_probe.py --route fused16 [--out profiles/msda_h16_fused_probe.txt]

times MSDeformAttn itself (256 channels, the four Linear layers included on both sides) under torch.autocast (fp16, bf16) and as a
.half() module, with ``fuse_prologue_16bit`` True (softmax, locations and padding mask inside the 16-bit kernels:
semidetr_msda_fused_forward_h16 / _backward_h16) against False (the op-by-op prologue in torch + the 16-bit op), the two sides
alternating in one process on three rotating input sets:
    encoder  N = 4, Lq = S, band padding mask      no_grad
    decoder  N = 4, Lq = 1100, 4-d boxes           no_grad
    train    N = 2, Lq = 300, 4-d boxes            forward + backward (600 rows: the largest call the 16-bit backward takes)
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


FUSED_SHAPES = (("encoder", 4, None, False), ("decoder", 4, 1100, False), ("train", 2, 300, True))
VARIANTS = (("autocast_fp16", torch.float16, True), ("autocast_bf16", torch.bfloat16, True), ("half_module", torch.float16, False))


def module_inputs(N, Lq, dev, seed):
    """(query, reference_points, input_flatten, shapes, starts, padding_mask) of one module call, fp32."""
    shp = np.asarray(LEVELS, np.int64)
    L, S = len(LEVELS), int((shp[:, 0] * shp[:, 1]).sum())
    g = torch.Generator(device=dev).manual_seed(seed)
    tsh = torch.from_numpy(shp).to(dev)
    tls = torch.cat([tsh.new_zeros(1), (tsh[:, 0] * tsh[:, 1]).cumsum(0)[:-1]])
    src = torch.randn(N, S, M * D, device=dev, generator=g)
    if Lq is None:      # encoder: the queries are the pixels, 2-d points at the pixel centres, images padded below / right
        cen = np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                              for h, w in LEVELS]).astype(np.float32)
        ref = torch.from_numpy(cen).to(dev)[None, :, None, :].expand(N, S, L, 2).contiguous()
        rows = []
        for fh, fw in ((1.0, 1.0), (1.0, 0.9), (0.94, 1.0), (0.88, 0.8))[:N]:
            per = []
            for h, w in LEVELS:
                mk = np.zeros((h, w), bool)
                mk[int(np.ceil(fh * h)):, :] = True
                mk[:, int(np.ceil(fw * w)):] = True
                per.append(mk.reshape(-1))
            rows.append(np.concatenate(per))
        return src + 0.1 * torch.randn(src.shape, device=dev, generator=g), ref, src, tsh, tls, torch.from_numpy(np.stack(rows)).to(dev)
    query = torch.randn(N, Lq, M * D, device=dev, generator=g)
    box = torch.cat([torch.rand(N, Lq, L, 2, device=dev, generator=g), torch.rand(N, Lq, L, 2, device=dev, generator=g) * 0.3 + 0.05], -1)
    return query, box, src, tsh, tls, None


def fused16_main(a):
    import semi_detr_amd as s
    dev = torch.device("cuda:0")
    lib = s._lib.lib()
    lines = [f"{torch.cuda.get_device_name(0)}; MSDeformAttn(256, 4, 8, 4), S = 22223; wall time per module call in us over at least "
             f"{a.calls} calls and at least 0.25 s after 20 warm-up calls, incl. the final synchronize; {a.rounds} alternating rounds on "
             f"three rotating input sets, min .. max (the spread between the rounds); fused16 = fuse_prologue_16bit True, parent = False "
             f"(op-by-op prologue in torch + the 16-bit op)"]
    for shape, N, Lq, train in FUSED_SHAPES:
        sets = [module_inputs(N, Lq, dev, 21 + i) for i in range(3)]
        for vname, dtype, autocast in VARIANTS:
            torch.manual_seed(3)
            m = s.MSDeformAttn(M * D, len(LEVELS), M, P).to(dev)
            with torch.no_grad():      # learned-looking offsets and weights instead of the initial star / zeros
                m.sampling_offsets.weight.normal_(0, 0.02)
                m.attention_weights.weight.normal_(0, 0.05)
            calls = sets
            if not autocast:
                m = m.half()
                calls = [tuple(t.half() if t.is_floating_point() else t for t in c[:3]) + c[3:] for c in sets]
            if train:
                calls = [(c[0].clone().requires_grad_(True), c[1], c[2].clone().requires_grad_(True)) + c[3:] for c in calls]
            turn = [0]

            def run(fused):
                m.fuse_prologue_16bit = fused
                c = calls[turn[0] % len(calls)]
                turn[0] += 1
                with torch.autocast("cuda", dtype=dtype, enabled=autocast), torch.set_grad_enabled(train):
                    out = m(*c)
                if train:
                    torch.autograd.grad(out.float().square().mean(), [c[0], c[2]] + list(m.parameters()))
                return out

            tn, to = [], []
            for _ in range(a.rounds):
                tn.append(wall(lambda: run(True), a.calls))
                kn = lib.semidetr_msda_h16_last_kernels().decode()
                to.append(wall(lambda: run(False), a.calls))
                ko = lib.semidetr_msda_h16_last_kernels().decode()
            spread = max(max(tn) - min(tn), max(to) - min(to))
            verdict = "no slower" if min(tn) <= min(to) + spread else "SLOWER"
            seg = "forward+backward" if train else "forward"
            lines.append(f"{shape:8s} N={N} Lq={calls[0][0].shape[1]:5d} {vname:13s} {seg:16s} fused16 {min(tn):8.1f} .. {max(tn):8.1f}   parent "
                         f"{min(to):8.1f} .. {max(to):8.1f}   ratio {min(to) / min(tn):5.2f}x   spread {spread:6.1f}   {verdict}   "
                         f"[{kn} | {ko}]")
            print(lines[-1], flush=True)
        del sets, calls
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


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
    ap.add_argument("--route", choices=("op", "fused16"), default="op",
                    help="op: the 16-bit op against the up-cast route; fused16: the module with fuse_prologue_16bit against without")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msda_h16_probe: needs a GPU (no timing is taken on the CPU)")
    if a.route == "fused16":
        return fused16_main(a)
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

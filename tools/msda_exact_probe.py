#!/usr/bin/env python
"""Time the exact MSDA backward (semidetr_msda_backward_exact_f32: grad_value as the exact, order-independent sum of its
contributions) against the default backward of the same build -- what reproducible training costs per layer call.

    python tools/msda_exact_probe.py [--calls 30] [--rounds 3] [--out profiles/msda_exact_probe.txt]

Shapes (8 heads x 32 channels, 4 levels of the 800 x 1333 pyramid x 4 points; S = 22 223), fp32:
    encoder  N = 4, Lq = S      queries are the pixels, samples ~ N(pixel centre, 2 px)
    decoder  N = 4, Lq = 1100   samples anywhere on the map
    micro    N = 2, Lq = 300
Backward only (the compiled front end's ms_deform_attn_exact_backward / ms_deform_attn_backward, allocations included on both
sides).  Protocol of tools/msda_h16_probe.py: both sides alternating in one process on three rotating input sets, wall time per
call over at least ``--calls`` calls and at least 0.25 s after 20 warm-up calls, host clock around work that ends in a
synchronise; ``--rounds`` rounds, min .. max, and the spread between the rounds.  Then the exact route's kernels one by one, from
torch.profiler's device-side kernel records of a few calls (mean per call).  Nothing is gated on these numbers: the route is
opt-in."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from msda_h16_probe import D, LEVELS, M, P, SHAPES, inputs, wall  # noqa: E402

STAGES = ("msda_bwd_gather_d32", "exact_clear", "exact_count", "exact_scan", "exact_fill", "exact_reduce")


def stage_times(fn, calls=5):
    """mean device time per call of each kernel of the exact route, us -> {stage: us} (torch.profiler)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for st in STAGES:
            if st in ev.key:
                dev_total = getattr(ev, "device_time_total", None)
                if dev_total is None:
                    dev_total = ev.cuda_time_total
                out[st] = out.get(st, 0.0) + dev_total / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msda_exact_probe: needs a GPU (no timing is taken on the CPU)")
    import semi_detr_amd as s
    import MultiScaleDeformableAttention as MSDA  # noqa: E402  (registered by the package import above)
    dev = torch.device("cuda:0")
    lib = s._lib.lib()
    lines = [f"{torch.cuda.get_device_name(0)}; M = {M}, D = {D}, L = {len(LEVELS)}, P = {P}, S = 22223, fp32; BACKWARD only, wall time per "
             f"call in us over at least {a.calls} calls and at least 0.25 s after 20 warm-up calls, incl. the final synchronize; "
             f"{a.rounds} alternating rounds on three rotating input sets, min .. max (the spread between the rounds); exact = "
             f"ms_deform_attn_exact_backward, default = ms_deform_attn_backward of the same build (adaptive policy)"]
    slot = 210
    for shape, N, Lq in SHAPES:
        slot += 1
        sets = []
        for i in range(3):
            value, tsh, tls, loc, attn, gout = inputs(N, Lq, torch.float32, dev)
            sets.append((value, tsh, tls, loc + 1e-3 * i, attn, gout))
        turn = [0]

        def pick():
            turn[0] += 1
            return sets[turn[0] % 3]

        def exact():
            v, sh, ls, lc, at, g = pick()
            return MSDA.ms_deform_attn_exact_backward(v, sh, ls, lc, at, g, 64, slot)

        def default():
            v, sh, ls, lc, at, g = pick()
            return MSDA.ms_deform_attn_backward(v, sh, ls, lc, at, g, 64, slot)

        for v, sh, ls, lc, at, _ in sets:      # the forward that precedes a backward in training: it feeds the slot's sample counts
            MSDA.ms_deform_attn_forward(v, sh, ls, lc, at, 64, slot)
        te, td = [], []
        for _ in range(a.rounds):
            te.append(wall(exact, a.calls))
            ke = lib.semidetr_msda_last_kernels().decode()
            td.append(wall(default, a.calls))
            kd = lib.semidetr_msda_last_kernels().decode()
        spread = max(max(te) - min(te), max(td) - min(td))
        Lq_ = sets[0][3].shape[1]
        entries = N * Lq_ * M * len(LEVELS) * P * 4 * 8
        lines.append(f"{shape:8s} N={N} Lq={Lq_:5d} backward   exact {min(te):9.1f} .. {max(te):9.1f}   default {min(td):8.1f} .. {max(td):8.1f}   "
                     f"exact / default {min(te) / min(td):6.2f}x   spread {spread:7.1f}   entry bytes (counted) {entries / 1e6:7.1f} MB   [{ke} | {kd}]")
        print(lines[-1], flush=True)
        try:
            st = stage_times(exact)
            total = sum(st.values())
            lines.append(f"{shape:8s} exact route, device time per call by kernel (us): " +
                         "  ".join(f"{k} {st.get(k, float('nan')):8.1f}" for k in STAGES) + f"   sum {total:8.1f}")
        except Exception as e:      # the profiler is an aid: the wall times above stand without it
            lines.append(f"{shape:8s} exact route, per-kernel times unavailable: {type(e).__name__}: {e}")
        print(lines[-1], flush=True)
        del sets
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

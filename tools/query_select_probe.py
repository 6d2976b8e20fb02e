#!/usr/bin/env python
"""Time the two-stage query selection at DINO's shapes on the GPU against the reference's op sequence restated with torch on
the same GPU in the same process (tests/query_select_torch_restated.py, checked against the reference's fixture by
tests/test_query_select_ref.py: the baseline is that sequence, never the new code itself).

    python tools/query_select_probe.py [--calls 200] [--out profiles/query_select_probe.txt]

B in {1, 4}, S = 22 223 (four levels), C = 80, k = 900, d_model = 256, mixed-size band masks.  Three segments, each timed on
both sides, alternating, wall time per call over ``--calls`` calls after warm-up (host clock around work that ends in a
synchronise); launches per call are counted with torch's profiler in a separate pass:
    proposals   gen_encoder_output_proposals forward
    select      max + top-k + the three gathers + the two sigmoids
    backward    both backwards (gradients of tgt_undetach and ref_enc down to the memory)
The copy in ``proposals`` is also set against its own bytes (one read of the unmasked rows + one write of the memory).
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

LEVELS = [(100, 167), (50, 84), (25, 42), (13, 21)]
FRACS = [(0.75, 0.9), (1.0, 1.0), (1.0, 0.62), (0.55, 1.0)]


def band_mask(shapes, fracs):
    rows = []
    for fh, fw in fracs:
        parts = []
        for H, W in shapes:
            m = np.ones((H, W), bool)
            m[:int(np.ceil(H * fh)), :int(np.ceil(W * fw))] = False
            parts.append(m.reshape(-1))
        rows.append(np.concatenate(parts))
    return np.stack(rows)


def segments(B, dev, k=900, C=80, D=256):
    import query_select_torch_restated as T
    import semi_detr_amd as s
    g = torch.Generator(device=dev).manual_seed(B)
    mask = torch.from_numpy(band_mask(LEVELS, FRACS[:B])).to(dev)
    S = mask.shape[1]
    shapes = torch.tensor(LEVELS, dtype=torch.long, device=dev)
    shapes_host = [tuple(r) for r in LEVELS]                     # the restatement iterates the levels on the host
    mem = torch.randn(B, S, D, device=dev, generator=g).requires_grad_(True)
    logits = torch.randn(B, S, C, device=dev, generator=g)
    reg = torch.randn(B, S, 4, device=dev, generator=g)
    with torch.no_grad():
        om0, prop0 = s.gen_encoder_output_proposals(mem, mask, shapes)
        coord0 = reg + prop0
    g_tgt = torch.randn(B, k, D, device=dev, generator=g)
    g_enc = torch.randn(B, k, 4, device=dev, generator=g)

    def fwd(side):
        if side == "hip":
            om, prop = s.gen_encoder_output_proposals(mem, mask, shapes)
            coord = (reg + prop).requires_grad_(True)
            out = s.select_queries(logits, coord, prop, om, k)
        else:
            om, prop = T.gen_proposals(mem, mask, shapes_host)
            coord = (reg + prop).requires_grad_(True)
            out = T.select(logits, coord, prop, om, k)
        return out[3], out[4], coord

    graphs = {side: fwd(side) for side in ("hip", "torch")}

    def backward(side):
        tgt, enc, coord = graphs[side]
        torch.autograd.grad([tgt, enc], [mem, coord], [g_tgt, g_enc], retain_graph=True)

    def nograd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run
    hip = {"proposals": nograd(lambda: s.gen_encoder_output_proposals(mem, mask, shapes)),
           "select": nograd(lambda: s.select_queries(logits, coord0, prop0, om0, k)), "backward": lambda: backward("hip")}
    base = {"proposals": nograd(lambda: T.gen_proposals(mem, mask, shapes_host)),
            "select": nograd(lambda: T.select(logits, coord0, prop0, om0, k)), "backward": lambda: backward("torch")}
    valid_rows = int(torch.isfinite(prop0[..., 0]).sum())
    return hip, base, dict(S=S, valid_rows=valid_rows, bytes=(valid_rows + B * S) * D * 4)


def wall(fn, calls, warmup=20, min_seconds=0.25):
    """us per call over at least ``calls`` calls AND at least ``min_seconds`` of work (a short segment gets more calls, so
    that the clock and the scheduler do not dominate the window)."""
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


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type.name != "CPU")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_select_probe: needs a GPU (no timing is taken on the CPU)")
    dev = torch.device("cuda:0")
    lines = [f"{torch.cuda.get_device_name(0)}; S = 22223 (4 levels), C = 80, k = 900, d_model = 256, mixed-size band masks; "
             f"wall time per call in us over at least {a.calls} calls and at least 0.25 s after 20 warm-up calls, incl. the final "
             f"synchronize; "
             f"{a.rounds} alternating rounds, min .. max"]
    for B in (1, 4):
        hip, base, info = segments(B, dev)
        for seg in ("proposals", "select", "backward"):
            th, tb = [], []
            for _ in range(a.rounds):
                th.append(wall(hip[seg], a.calls))
                tb.append(wall(base[seg], a.calls))
            try:
                nl = f"launches {launches(hip[seg]):3d} vs {launches(base[seg]):3d}"
            except Exception as e:                                  # the profiler is an aid, the timing is the result
                nl = f"launches not counted ({type(e).__name__})"
            verdict = "no slower" if min(th) <= min(tb) else "SLOWER"
            lines.append(f"B={B} {seg:10s} hip {min(th):8.1f} .. {max(th):8.1f}   torch restatement {min(tb):8.1f} .. {max(tb):8.1f}   "
                         f"ratio {min(tb) / min(th):5.2f}x   {nl}   {verdict}")
            if seg == "proposals":
                lines.append(f"B={B} proposals  moves {info['bytes'] / 1e6:.1f} MB ({info['valid_rows']} unmasked rows read, "
                             f"{B * info['S']} written): {info['bytes'] / min(th) / 1e6:.2f} TB/s over the wall time per call")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

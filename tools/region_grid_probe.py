#!/usr/bin/env python
"""Sweep the region grids of the three encoder window kernels (semidetr_msda_set_region_grid) on bench.py's inputs -- fused prologue,
padding masks of the mixed-size batch, window kernels -- and print one line per (batch size, kernel, pinned grid): the forward launch
for `forward`, the whole backward (window gather + region scatter, the other kernel left automatic) for `gather` / `scatter`.
`pin 0x0` is what the library chooses by itself.  profiles/region_grid_probe.txt is this tool's output.

    python tools/region_grid_probe.py [--bs 1 4] [--iters 20] [--passes 3] [--rows 4] [--cols 7]

A library without the pin (an older build loaded through the same Python tree) is measured at its defaults only."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

KERNELS = ("forward", "gather", "scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3, help="every grid is timed once per pass, the passes interleaved")
    ap.add_argument("--rows", type=int, default=4, help="region rows above the coarsest grid that are swept (the scatter: + 2)")
    ap.add_argument("--cols", type=int, default=7, help="region columns above the coarsest grid (the scatter: 4)")
    a = ap.parse_args()
    import semi_detr_amd as sda          # (registers the compiled front end under the reference's module name)
    import MultiScaleDeformableAttention as MSDA
    has_pin = "semidetr_msda_set_region_grid" in sda._lib.SIGNATURES
    sda._lib.set_forward_policy("window")
    dev = torch.device("cuda:0")
    wl = bench.Workload(dev, 1234, recipe="coco10", io="raw", input_sets=8, masked=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("device", torch.cuda.get_device_name(0), "compute units", cus, "pin available", has_pin, flush=True)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    def runner(n, forward):
        mask, turn = wl.mask[n], [0]

        def fn():
            turn[0] += 1
            r = turn[0]
            v, args = wl.t[("value", n)][r % wl.rot], wl._args("enc", n, wl.S, r)
            if forward:
                MSDA.ms_deform_attn_fused_forward(v, wl.shapes, wl.starts, *args, mask)
            else:
                MSDA.ms_deform_attn_fused_backward(v, wl.shapes, wl.starts, *args, wl.t[("enc_gout", n)][r % wl.rot], mask)
        return fn

    # the coarsest grids of the 800 x 1333 pyramid: 25 x 16 (forward), 15 x 16 (gather), 8 x 24 (scatter) pixel regions of the 100 x 167 level
    coarsest = {"forward": (4, 11), "gather": (7, 11), "scatter": (13, 7)}
    for n in a.bs:
        for kernel in KERNELS:
            fn = runner(n, kernel == "forward")
            for _ in range(6):          # (synchronised: the backward's gather follows what the slot's forward launches counted)
                fn()
                torch.cuda.synchronize()
            y0, x0 = coarsest[kernel]
            rows, cols = (a.rows + 2, 4) if kernel == "scatter" else (a.rows, a.cols)
            grids = [(0, 0)] + ([(y, x) for y in range(y0, y0 + rows) for x in range(x0, x0 + cols)] if has_pin else [])
            res = {g: [] for g in grids}
            for _ in range(a.passes):
                for g in grids:
                    if has_pin:
                        sda._lib.set_region_grid(kernel, *g)
                    res[g].append(timed(fn))
            base = statistics.median(res[(0, 0)])
            for g in grids:
                info = ""
                if has_pin:
                    sda._lib.set_region_grid(kernel, *g)
                    q = sda._lib.region_grid(kernel, bench.LEVELS, n, bench.M, cus)
                    info = "grid %dx%d regions %d workgroups %d tail split %d largest region %d queries" % (
                        q["nry"], q["nrx"], q["regions"], q["workgroups"], q["tail_split"], q["max_queries"])
                print("bs%d %-8s pin %2dx%-2d  median %7.1f us  min %7.1f  max %7.1f  vs automatic %+5.1f%%  %s" % (
                    n, kernel, g[0], g[1], statistics.median(res[g]), min(res[g]), max(res[g]),
                    100 * (statistics.median(res[g]) / base - 1), info), flush=True)
            if has_pin:
                sda._lib.set_region_grid(kernel, 0, 0)


if __name__ == "__main__":
    main()

// Every compile-time tuning knob of the MSDA unit (msda.hip and the headers it includes), each with its default and the measurements that
// chose it.  Preprocessor only: plain C++ includes it too (tests/host/msda_grid_host_check.cpp).  msda.hip includes it before any kernel
// header, so a tuning build overrides a knob on the command line (tools/ab_build.sh <name> -DSEMIDETR_X=..., tools/rw_regs.sh,
// tools/kernel_resources.py --extra) and every user sees the same value.  A knob is DEFINED here and nowhere else; what a window kernel is
// instantiated with is put together from them in exactly one place, its ...Product configuration (msda_dispatch.h).
// (Not here: SEMIDETR_BRFREE and SEMIDETR_NT_LOADS, switches inside the kernel bodies of msda_rw.h / msda_fast.h that no dispatch code reads.)
#pragma once

#ifndef SEMIDETR_SCATTER_SW      // 1 (tuning builds): the cell-sorted scatter (msda_sw.h, measured and rejected) instead of the region scatter
#define SEMIDETR_SCATTER_SW 0
#endif
#ifndef SEMIDETR_SW_NT
#define SEMIDETR_SW_NT 512
#define SEMIDETR_SW_Q 176
#define SEMIDETR_SW_RTH 8
#define SEMIDETR_SW_RTW 16
#define SEMIDETR_SW_WH 24
#define SEMIDETR_SW_WW 32
#define SEMIDETR_SW_WPE 4
#endif
#ifndef SEMIDETR_SW_DBG
#define SEMIDETR_SW_DBG 0      // timing aids (tuning builds, results wrong): 1 no entry loop, 2 no flush, 4 no misses, 8 no walk at all
#endif
// A/B knobs of tools/archive/r04_ab_multi.sh (same-box comparison of several builds inside the bench step).  Round 4, rotated inputs:
// encoder gather with 8 instead of 16 corner loads in flight at five waves per SIMD: backward 701 -> 695 us at bs 4 (with
// replayed inputs round 2 had measured it level); region scatter with 176 queries per pass at six waves per SIMD (three
// workgroups per CU): with 13 VGPRs spilled 702 vs 701 us at bs 4, 205 vs 196 us at bs 1; once the thread-derived constants were
// kept out of the kernel-long registers (msda_region.h: 102 -> 84 VGPRs at four waves, 2 spilled dwords at six) 700 -> 680 us at
// bs 4, 197 -> 194.5 us at bs 1, fused prologue 733 -> 712 us -- adopted.
#ifndef SEMIDETR_GATHER_WPE      // encoder gather: waves per SIMD the register budget is set for, corner loads in flight / 4
#define SEMIDETR_GATHER_WPE 5
#define SEMIDETR_GATHER_KB 2
#endif
#ifndef SEMIDETR_GATHER5_WPE     // ... the five-level (20-sample) instantiation
#define SEMIDETR_GATHER5_WPE 4      // (5 / 2 as for four levels: COCO-Full encoder backward 9.77 -> 9.69 ms per step, but the fused-prologue
#define SEMIDETR_GATHER5_KB 4       //  instantiation spills 4 registers there -- left as it is)
#endif
#ifndef SEMIDETR_SEPARATE_FILL
#define SEMIDETR_SEPARATE_FILL 0      // tuning builds: 1 = hipMemsetAsync before the gather instead of the gather's side job
#endif
#ifndef SEMIDETR_SCATTER_Q       // region scatter: queries per pass (LDS) and waves per SIMD
#define SEMIDETR_SCATTER_Q 256     // (an 8 x 24 region of a halving pyramid has 192 + 48 + 12 + 3 queries: one pass; more take several)
#define SEMIDETR_SCATTER_WPE 6
#endif
#ifndef SEMIDETR_SCATTER_WU
#define SEMIDETR_SCATTER_WU 8      // entries per stream and trip of the row walk (+ kWuPaired: paired corners, msda_region.h ScatterWu)
#endif
#ifndef SEMIDETR_SCATTER_NT
#define SEMIDETR_SCATTER_NT 512    // (704 threads = one sample per thread, no half-empty second sample slot, two workgroups per CU:
#endif                             //  encoder backward 726 against 678 us at bs 4 -- the third workgroup is worth more)
#ifndef SEMIDETR_SCATTER_TIGHT
#define SEMIDETR_SCATTER_TIGHT 1
#endif
#ifndef SEMIDETR_SCATTER_AID
#define SEMIDETR_SCATTER_AID 0      // tuning builds (tools/ab_build.sh -DSEMIDETR_SCATTER_AID=...): timing aids of the walk, results wrong
#endif
#ifndef SEMIDETR_SCATTER_RTH     // region scatter: region (pixels of the finest level) and window per sampling level
// Round 5, after the flush path lost its 64-bit arithmetic (the kernel then ran at the atomic unit's rate, compute 328 of 398 us): 8 x 24
// regions, 24 x 40 windows, 256 queries per pass, 74.5 KB of LDS = TWO workgroups per CU flush 10 % fewer rows -- 400 -> 365 us at bs 4,
// 118 -> 114 us at bs 1 (tools/r05_ab_kern.sh; 8 x 16 / 176 queries / three per CU was the optimum while compute was the co-limit).
// Others measured: 12 x 16 390, 10 x 16 385, 8 x 20 387, 8 x 22 383, 8 x 24 with 272 queries (three samples per thread) 375, 576 / 640
// threads 414 / 406, 16 x 16 at one workgroup per CU 457-514.
#define SEMIDETR_SCATTER_RTH 8
#define SEMIDETR_SCATTER_RTW 24
#define SEMIDETR_SCATTER_WH 24
#define SEMIDETR_SCATTER_WW 40
#endif
#ifndef SEMIDETR_GW_NT           // msda_gw_d32 (lane-per-sample gather of the encoder backward): threads, region, margins of level 0 / the coarse levels
#define SEMIDETR_GW_NT 1024      // (round 5, second half: 768 -> 1024 once nothing spilled there)
#define SEMIDETR_GW_RTH 15      // (round 6: 15, not 16 -- the grad_out rows of a round need 8 KB of LDS beside the windows; a 100-row level is 7 x 14.3 rows either way)
#define SEMIDETR_GW_RTW 16
#define SEMIDETR_GW_H0 4
#define SEMIDETR_GW_HC 4
#endif
#ifndef SEMIDETR_GW_RTH5
#define SEMIDETR_GW_RTH5 13      // ... five levels: the windows of all five at margin 4 fit beside the query list with regions of up to 13 x 16 pixels
#define SEMIDETR_GW_NT5 1024     //     (a 100-row level = 8 x 12.5 rows; 14 rows -- the same tiling -- would need 165 KB)
#define SEMIDETR_GW_NT5_RAW 1024 //     (with the grad_out rows in LDS the fused prologue fits 1024 threads too: 117 / 128 VGPRs, no spill)
#endif
#ifndef SEMIDETR_GW_FB
#define SEMIDETR_GW_FB 4         // msda_gw_d32: far samples whose loads are in flight together
#endif
#ifndef SEMIDETR_GW_SB
#define SEMIDETR_GW_SB 1            // dot-loop steps (five ds_read_b128 each) between scheduling barriers
#endif
#ifndef SEMIDETR_GW_DBG
#define SEMIDETR_GW_DBG 0        // timing aids of msda_gw_d32 (results wrong), tuning builds only
#endif
#ifndef SEMIDETR_RW_NT
#define SEMIDETR_RW_NT 768       // msda_rw_d32: threads per workgroup.  Its windows take most of the LDS, so a CU holds ONE workgroup and
                                 // the workgroup's size is the CU's occupancy: 12 instead of 8 waves 192.9 -> 176.7 us inside the step
                                 // (1024 threads: only with margin 5 and 25 spilled registers so far, 262 us)
#endif
#ifndef SEMIDETR_RW_TAIL
#define SEMIDETR_RW_TAIL 1       // msda_rw_d32 forward: tail split (helper workgroups for the last, partly filled wave of workgroups)
#endif
#ifndef SEMIDETR_RW_DBG
#define SEMIDETR_RW_DBG 0        // timing aids of the four-level msda_rw_d32 (results wrong), tuning builds only: see msda_rw.h
#endif
#ifndef SEMIDETR_RW_TUNE
#define SEMIDETR_RW_TUNE kRwProduct4        // msda_rw_d32's configuration: msda_rw.h's rw_tune(named flags, samples between scheduling barriers).  The product's
                                            // are defined, pinned to their historical numbers and explained at kRwProduct4 / kRwProduct5 in msda_dispatch.h; a tuning
                                            // build may pass an archived record's plain integer instead (tools/ab_build.sh -DSEMIDETR_RW_TUNE=1920)
#endif
#ifndef SEMIDETR_RW_SB_LOCATTN
#define SEMIDETR_RW_SB_LOCATTN rw_untune(SEMIDETR_RW_TUNE).samples_per_barrier
                                      // the reference contract's compute-loop samples between scheduling barriers (the fused prologue keeps SEMIDETR_RW_TUNE's).
                                      // Round 5: four (-1.3 ... -2 %); round 6, with the branch-free round loop (msda_rw.h SEMIDETR_BRFREE; 129 VGPRs at any spacing):
                                      // two / three / four samples 162.5-163.8 / 168.5-171.0 / 164.3-165.4 us (tools/r05_ab_kern.sh, same box) -> two, like RawIO
#endif
#ifndef SEMIDETR_RW_TUNE_MASK
#define SEMIDETR_RW_TUNE_MASK kRwProduct4   // the instantiation with the padding mask (166 VGPRs; with the table but without the compact records it spills)
#endif
#ifndef SEMIDETR_RW_RTH
#define SEMIDETR_RW_RTH 25       // msda_rw_d32, four levels: LARGEST region height (x 16 columns; the grid is tiled evenly, msda_rw.h) and coarse-level
                                 // margin.  24 x 16 regions hold 510 queries
#endif
#ifndef SEMIDETR_RW_HC
#define SEMIDETR_RW_HC 5         // (5.3 rounds of 96: better balanced than 16 x 16's 3.5) and stage 1.8 instead of 2.9 window rows per query; margin 5
                                 // is the widest that fits then.  In the step 167.2 -> 162.2 us (16 x 16 / margin 6 -> 24 x 16 / margin 5; 32 x 16 /
                                 // margin 4: 165.6); by spread (probe): -6 % at 1 px, -1..-4 % at 2 px, level at 2.5 - 4 px, +3 % at 5 px
#endif
#ifndef SEMIDETR_RW_RTH5
#define SEMIDETR_RW_RTH5 24      // ... five levels.  With the evenly tiled grid (a 100-row level = 4 x 25 or 5 x 20 rows instead of 4 x 24 + 4), in
#endif                           // the step: four levels 25 / 24 rows 162.2 / 166.7 us (fused prologue 172.7 / 179.1; uneven 24: 162.0 / 176.5),
                                 // five levels 254 / 249 us (uneven 24: 257) -- what decides is how evenly a region's queries fill its rounds
#ifndef SEMIDETR_RW_NT5
#define SEMIDETR_RW_NT5 960      // ... the five-level instantiation: margin 4 is what fits either way; 24 x 16 regions like the four-level one, and the
                                 //     largest workgroup that fits beside their windows: 15 waves (16 x 16 / 1024 threads: 202 / 209 / 243 us at sigma 1 /
                                 //     2 / 3 px, 24 x 16 / 960: 195 / 204 / 241, / 896: 190 / 204 / 242)
#define SEMIDETR_RW_TUNE5 kRwProduct5   // (the fused prologue kept round 4's configuration through round 5 -- with table + query list it spilled at 128
                                        //  registers: SEMIDETR_RW_TUNE5_RAW / _MASK)
#ifndef SEMIDETR_RW_TUNE5_RAW
#define SEMIDETR_RW_TUNE5_RAW kRwProduct5      // (round 6: with no branch around the round loop's loads -- msda_rw.h SEMIDETR_BRFREE -- the fused prologue's five-level
#define SEMIDETR_RW_TUNE5_MASK kRwProduct5     //  instantiations fit the table / list / compact-record configuration too: 112 / 113 VGPRs, no spill; rounds 4-5:
#endif                                         //  rw_tune(kRwRebuildTid | kRwLean | kRwOneFine, 1) = 1110)
#endif
#ifndef SEMIDETR_LVL_CHUNKQ
#define SEMIDETR_LVL_CHUNKQ 224      // queries per scatter workgroup of the levels too large to bucket.  Round 5 (tools/r05_ab_step.sh): the merged
                                     // launch takes one 1024-thread workgroup per CU, so what counts is how its workgroups fill waves of 256 --
                                     // Lq 1100 at bs 4: 192 -> 6 chunks -> 768 + 280 = 1048 workgroups = 4.09 waves; 224 / 256 -> 5 chunks -> 920 =
                                     // 3.6: decoder backward 0.901 -> 0.864 ms per step (bs 4), 0.306 -> 0.255 (bs 1: 262 -> 230 workgroups, one
                                     // wave); 208 (6 chunks) 0.902 / 0.306, 320 (4 chunks) 0.932 / 0.269
#endif

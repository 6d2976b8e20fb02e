// Product dispatch of the fp32 / channels == 32 MSDA fast path: the configurations of the three encoder window kernels (RwProduct,
// GwProduct, ScatterProduct -- a window kernel is instantiated in exactly one of them, from the knobs of msda_tuning.h), the grid-size
// hints, and launch_fast_forward / launch_fast_backward.  Included by msda.hip after the kernel headers, msda_grid.h and msda_policy.h;
// msda_experiments.h (the tuning dispatch of the experiments library) follows it and shares pick_split, allow_big_lds and the hints.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "msda_grid.h"
#include "msda_policy.h"

namespace {

// fast-path applicability: channels == 32, 16-byte aligned pointers, LDS budget
bool fast_ok(const void *a, const void *b, const void *c, int D, int L, int P)
{
    const uintptr_t al = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
    return D == kD && L <= kMaxLevels && (al & 15) == 0 && (int64_t)L * P <= 256;
}

// kOob + (head offset + lane offset) must stay out of range without wrapping: the in-row byte offset of a lane is
// < num_heads * 128, so num_heads <= 32 keeps it below the 4096-byte guard band of kOob.
bool heads_ok(int M) { return (int64_t)M * kD * 4 <= 4096; }

// the fast-path kernels address one image's value slice with 32-bit BYTE offsets (buffer instructions)
bool slice_ok(int S, int M) { return (int64_t)S * M * kD * 4 < (int64_t)0xFFFFF000u; }

using semidetr::pick_split;         // (common.h: the one rule of the fp32 and the 16-bit forward)
using semidetr::allow_big_lds;     // (kernels of one signature share the pointer TYPE; the grant is keyed on the pointer VALUE)

// ---- grid-size hints.  The level table lives in device memory, so a launch that has no host copy of it cannot know how many patches /
//      regions its pyramid has.  The kernels enumerate their units on the device: a workgroup takes units slot, slot + bound, slot + 2 x
//      bound, ... of its (image, head) until none is left, so ANY bound >= 1 computes the same result -- too small a bound serialises units in one
//      workgroup, too large a one launches workgroups that read the level table, find nothing and leave.  The hints aim a little above
//      the real count of a usual DETR pyramid.
// units of `patch_px` pixels each cut from EVERY level (the 4 x 8 query patches of the patch forward / gather): about the number of such
// patches of a usual pyramid, ragged edges included
inline int patch_grid_hint(int S, int L, int patch_px) { return (S + patch_px - 1) / patch_px * 5 / 4 + 4 * L; }
// regions of up to `region_px` pixels of the FINEST level, which holds ~3/4 of a DETR pyramid's pixels (the window kernels, the region scatter)
inline int finest_level_regions(int S, int region_px) { return (S * 3 / 4 + region_px - 1) / region_px; }
inline int region_grid_hint(int S, int L, int region_px) { return finest_level_regions(S, region_px) * 9 / 8 + 2 * L; }
// the region scatter's hint before round 5 (SEMIDETR_SCATTER_TIGHT=0), the patch formula on regions: S / region * 5 / 4 + 4 L = 161 for the 91
// regions of the 800 x 1333 pyramid launched 2240 workgroups per bs-4 launch that found no region -- each holds one of a CU's two slots
// until it has read the level table
inline int region_grid_hint_loose(int S, int L, int region_px) { return patch_grid_hint(S, L, region_px); }

// ---- the product configurations of the region-window forward (msda_rw.h; defaults of SEMIDETR_RW_TUNE... in msda_tuning.h).  The numbers they are
//      pinned to are what DESIGN.md, profiles/ and the archived A/B scripts quote (kernel names print them).
// Four levels.  Round 4 (1920): two compute-loop samples between scheduling barriers (with four samples' LDS reads in flight round 4's first
// version spilled; one: 2 us slower); kRwOneFine -33 VGPRs; kRwLean 256 -> 160 VGPRs: what lets 768 threads run; kRwSplitLoad: the fused
// prologue's location arithmetic at the start of the round that uses the loaded data, not where the loads are issued (a round early, waiting for
// them): fused-prologue forward 189.8 -> 188.0 us.  Round 5: kRwLevelTable, kRwQueryList, kRwCompact and kRwOneOowPerTrip -- the geometry of a
// round 284 -> ~130 VALU instructions, no publish step: probe (tools/r05_ab_fwd.sh, medians of 5) 169.1 -> 164.4 us at sigma 1 px, 179.4 ->
// 172.7 at 2 px, 202.3 -> 190.1 at 3 px; kRwWideOffsets: another -1 %.
constexpr int kRwProduct4 = rw_tune(kRwWideOffsets | kRwCompact | kRwQueryList | kRwLevelTable | kRwSplitLoad | kRwOneOowPerTrip | kRwLean | kRwOneFine, 2);
// Five levels.  Round 4 (1110; 16 waves per CU, 128 VGPRs): ONE sample between scheduling barriers (three passes of samples per lane) and
// kRwRebuildTid.  768 threads: 223 / 232 / 273 us at sigma 1 / 2 / 3 px, 1024: 208 / 225 / 255.  (Four levels at 1024 threads would have to
// give up margin 6 for 5: 206 against 205 us -- no gain.)  Round 5: as four levels -- split loads, level table, query list, compact records,
// one out-of-window sample per trip; the wide window offsets do not fit beside 120 octets' records.
constexpr int kRwProduct5 = rw_tune(kRwCompact | kRwQueryList | kRwLevelTable | kRwSplitLoad | kRwRebuildTid | kRwOneOowPerTrip | kRwLean | kRwOneFine, 1);
static_assert(kRwProduct4 == 98320 && kRwProduct5 == 47910, "the product configurations keep their historical numbers");
static_assert(rw_tune_or(kRwProduct4, kRwTailSplit) == 200720, "... and the tail-split variant its own (98320 + 100 x kRwTailSplit)");

// One product configuration of the window forward, keyed on (IO, levels, padding mask): kernel, tail-split kernel, LDS bytes, threads and
// region pixels all come from the ONE parameter set below, so what is launched and what it is given cannot disagree.
// Level 0 through global loads, windows of the coarse levels with the widest margin that fits beside the octet records: one workgroup per CU
// either way, and the workgroup as large as its registers allow (SEMIDETR_RW_NT).
//   four levels: 24 x 16 regions, margin FIVE, 113 KB of windows + 34.5 KB of records (16 x 16 regions at margin 4 / 5 / 6 and
//                sigma 2 px: 239 / 231 / 219-229 us, at 3 px: 290 / 265 / 252 us with 512 threads; SEMIDETR_RW_RTH in msda_tuning.h)
//   five levels: 24 x 16 regions, margin FOUR (102 + 53 KB; margin 5 fits only a 640-thread workgroup), 960 threads; patch
//                kernel 314 / 292 / 299 us at sigma 1 / 2 / 3 px, this one 195 / 204 / 241
template <typename IO, int KL, bool MASK>
struct RwProduct {
    static constexpr bool kRaw = std::is_same<IO, RawIO>::value;
    static_assert((KL == 4 || KL == 5) && (!MASK || kRaw), "four or five levels; the padding mask comes with the fused prologue");
    static constexpr int threads = KL == 4 ? SEMIDETR_RW_NT : SEMIDETR_RW_NT5, rth = KL == 4 ? SEMIDETR_RW_RTH : SEMIDETR_RW_RTH5, rtw = 16;
    static constexpr int hc = KL == 4 ? SEMIDETR_RW_HC : 4, dbg = KL == 4 ? SEMIDETR_RW_DBG : 0, region_px = rth * rtw;
    static constexpr int round = threads / 8;      // queries per round: eight lanes per query
    // (the reference contract's four-level instantiation has its own barrier spacing, SEMIDETR_RW_SB_LOCATTN; the tail split, a four-level
    //  instantiation of its own -- msda_rw.h kRwTailSplit --, keeps the configuration's)
    static constexpr int tune4 = MASK ? SEMIDETR_RW_TUNE_MASK : SEMIDETR_RW_TUNE;
    static constexpr int tune5 = MASK ? SEMIDETR_RW_TUNE5_MASK : (kRaw ? SEMIDETR_RW_TUNE5_RAW : SEMIDETR_RW_TUNE5);
    static constexpr int tune = KL == 5 ? tune5 : (kRaw ? tune4 : rw_tune_spaced(tune4, SEMIDETR_RW_SB_LOCATTN));
    static constexpr int tune_tail = rw_tune_or(tune4, kRwTailSplit);
    template <int TUNE> static constexpr auto kernel_of = &msda_rw_d32<IO, threads, rth, rtw, -1, hc, KL, false, dbg, TUNE, MASK>;
    template <int TUNE> static constexpr size_t lds_of = rw_lds_bytes<threads, rth, rtw, -1, hc, KL, TUNE>();
    // (functions, here and in the two configurations below: naming a configuration -- grid_geom does, for its geometry -- must not instantiate
    //  its kernel; the kernels are instantiated where the launch functions take them, in that order)
    static constexpr bool has_tail = KL == 4;
    static constexpr auto kernel() { return kernel_of<tune>; }
    static constexpr auto kernel_tail() { return kernel_of<has_tail ? tune_tail : tune>; }      // (no tail split: the plain kernel)
    static constexpr size_t lds_bytes = lds_of<tune>;
    static_assert(lds_bytes <= 160 * 1024, "region-window configuration does not fit the LDS");
    static_assert(!has_tail || lds_of<tune_tail> == lds_bytes, "the tail-split instantiation is launched with the same LDS size");
};

// One product configuration of the lane-per-sample window gather (msda_gw.h), keyed like RwProduct: 16 x 16 regions, margin 4 on every level,
// one 1024-thread workgroup per CU
// (round 5: 1024 threads = 16 waves per CU for the reference contract and the fused prologue without a mask -- 124 / 128 VGPRs
//  once the region grid's division reciprocals and the float copies of the level sizes are rebuilt per region: 232 -> 217 us
//  in the probe; the masked instantiation too since the thread index is rebuilt from the wave number where it is needed)
// Five levels (round 6, the COCO-Full pyramid): 20 lanes per (query, head) row, three rows per wave; the windows of five levels
// at margin 4 fit the LDS with regions of up to 13 x 16 pixels (SEMIDETR_GW_RTH5).
template <typename IO, int KL, bool MASK>
struct GwProduct {
    static constexpr bool kRaw = std::is_same<IO, RawIO>::value;
    static_assert((KL == 4 || KL == 5) && (!MASK || kRaw), "four or five levels; the padding mask comes with the fused prologue");
    static constexpr int threads = KL == 4 ? SEMIDETR_GW_NT : (kRaw ? SEMIDETR_GW_NT5_RAW : SEMIDETR_GW_NT5);
    static constexpr int rth = KL == 4 ? SEMIDETR_GW_RTH : SEMIDETR_GW_RTH5, rtw = SEMIDETR_GW_RTW, region_px = rth * rtw;
    static constexpr int round = (threads / 64) * (KL == 4 ? 4 : 3);      // queries per round: four / three (query, head) rows per wave
    static constexpr auto kernel() { return &msda_gw_d32<IO, threads, rth, rtw, SEMIDETR_GW_H0, SEMIDETR_GW_HC, KL, MASK, SEMIDETR_GW_DBG>; }
    static constexpr size_t lds_bytes = gw_lds_bytes<threads, rth, rtw, SEMIDETR_GW_H0, SEMIDETR_GW_HC, KL>();
};

// The product configuration of the region scatter (msda_region.h), keyed on the IO alone: one instantiation serves every pyramid.
template <typename IO>
struct ScatterProduct {
    static constexpr int threads = SEMIDETR_SCATTER_NT, queries_per_pass = SEMIDETR_SCATTER_Q;
    static constexpr int rth = SEMIDETR_SCATTER_RTH, rtw = SEMIDETR_SCATTER_RTW, region_px = rth * rtw;
    // (two workgroups per CU are four waves per SIMD: the fused prologue's instantiation takes that register budget -- at six it
    //  spills two registers; the reference contract's measured 1.5 % faster with the tighter one)
    static constexpr int wpe = std::is_same<IO, RawIO>::value ? 4 : SEMIDETR_SCATTER_WPE;
    static constexpr int wh = SEMIDETR_SCATTER_WH, ww = SEMIDETR_SCATTER_WW;
    static constexpr auto kernel() { return &msda_bwd_scatter_d32_reg<IO, threads, queries_per_pass, rth, rtw, wh, ww, 0, wpe, SEMIDETR_SCATTER_WU>; }
    static constexpr size_t lds_bytes = reg_lds_bytes<threads, queries_per_pass, wh, ww>();
    // workgroups a CU holds at once: what its 160 KB of LDS and its 2048 threads take (74.5 KB, 512 threads: two)
    static constexpr int per_cu = (int)std::min<size_t>(160 * 1024 / lds_bytes, 2048 / threads);
    static_assert(per_cu >= 1, "region-scatter configuration does not fit a CU");
};

// The chooser (msda_grid.h) has ONE geometry per (kernel, levels), whatever the IO policy of the launch.
template <int KL>
constexpr bool kGwSameGeometry = GwProduct<RawIO, KL, false>::round == GwProduct<LocAttnIO, KL, false>::round &&
                                 GwProduct<RawIO, KL, false>::rth == GwProduct<LocAttnIO, KL, false>::rth &&
                                 GwProduct<RawIO, KL, false>::rtw == GwProduct<LocAttnIO, KL, false>::rtw;
static_assert(kGwSameGeometry<4> && kGwSameGeometry<5>,
              "the region-grid chooser scores one geometry per (kernel, levels): the fused prologue's (RawIO) and the reference contract's "
              "(LocAttnIO) window-gather configurations must have the same round, rth and rtw (SEMIDETR_GW_NT5_RAW == SEMIDETR_GW_NT5)");
static_assert(ScatterProduct<RawIO>::per_cu == ScatterProduct<LocAttnIO>::per_cu, "... and the region scatter's one occupancy");

// what the chooser is told about kernel 0 forward / 1 gather / 2 scatter for a pyramid of L levels (the set-up shares: msda_grid.h grid_geom_of)
GridGeom grid_geom(int kernel, int L)
{
    using Rw4 = RwProduct<LocAttnIO, 4, false>; using Rw5 = RwProduct<LocAttnIO, 5, false>;
    using Gw4 = GwProduct<LocAttnIO, 4, false>; using Gw5 = GwProduct<LocAttnIO, 5, false>;
    using Sc = ScatterProduct<LocAttnIO>;
    // (the window kernels' windows take most of the LDS: one workgroup per CU)
    if (kernel == 0) return L == 5 ? grid_geom_of(0, Rw5::rth, Rw5::rtw, Rw5::round, 1) : grid_geom_of(0, Rw4::rth, Rw4::rtw, Rw4::round, 1);
    if (kernel == 1) return L == 5 ? grid_geom_of(1, Gw5::rth, Gw5::rtw, Gw5::round, 1) : grid_geom_of(1, Gw4::rth, Gw4::rtw, Gw4::round, 1);
    return grid_geom_of(2, Sc::rth, Sc::rtw, Sc::queries_per_pass, Sc::per_cu);
}

// ---- product dispatch of the fast path (fp32, channels == 32), shared by the reference contract (LocAttnIO) and the
//      fused prologue (RawIO).  Apart from the forward-kernel choice (msda_policy.h), what runs is a function of the arguments only.
template <typename IO>
int launch_fast_forward(hipStream_t st, const float *value, const int64_t *spatial_shapes,
                        const int64_t *level_start, const IO &io, int N, int S, int M, int L, int Lq, int P,
                        int flags, float *out, const int64_t *host_shapes = nullptr)
{
    SEMIDETR_REQUIRE(!(flags & SEMIDETR_MSDA_QUERIES_ARE_PIXELS) || Lq == S, SEMIDETR_E_BADARG,
                     "msda_forward: SEMIDETR_MSDA_QUERIES_ARE_PIXELS needs num_query == spatial_size");
    // (a patch's 32 x (L * P + 1) records have to fit 64 KB: pyramids of more than 15 levels x 4 points take the strips)
    const bool pixels = (flags & SEMIDETR_MSDA_QUERIES_ARE_PIXELS) != 0 && (size_t)32 * (L * P + 1) * 32 <= 63 * 1024;
#define LAUNCH_FWD(SP, PT, TILES, LDS)                                                                          \
    hipLaunchKernelGGL((msda_fwd_d32<SP, 4, PT, IO>), dim3((unsigned)((int64_t)N * (TILES) * M)), dim3(256), \
                       (LDS), st, value, spatial_shapes, level_start, io, S, M, L, Lq, P, (TILES), out)
    if (pixels) {
        // encoder self-attention.  The region-window kernel is built for num_point == 4 and four or five levels.  A padding mask
        // (fused prologue; the reference ALWAYS passes one: transformer.py:1309,1460 -> ops/modules/ms_deform_attn.py:95-96) has its
        // own instantiation: padded rows are staged as zeros, level 0 drops padded corners from its records (msda_rw.h).
        // SEMIDETR_MSDA_FIXED_FORWARD: the caller wants the kernel to be a function of the arguments alone (bitwise reproducible
        // forward: the two kernels sum in different orders) -- the patch kernel, whatever the policy says.
        // (an image's sampling data and output below 2^32 bytes: the window kernel indexes them with 32 bits inside the image)
        const bool window_ok = P == kPT && (L == 4 || L == 5) && !(flags & SEMIDETR_MSDA_FIXED_FORWARD) &&
                               (uint64_t)S * M * L * P * 8 < (1ull << 32) && (uint64_t)S * M * kD * 4 < (1ull << 32);
        FwdStats fs;
        bool use_window = false;
        if (int rc = fwd_adapt_next(st, window_ok, (flags >> 8) & 0xff, L, fs, use_window)) return rc;
        if (use_window) {
            bool fell_back = false;      // a device / runtime that does not grant the window kernel its ~150 KB of LDS gets the patch kernel, not an error
            // cfg: the RwProduct to run.  Its kernel_tail is the same configuration with the tail split compiled in (has_tail: whether it has one)
            auto launch_window = [&](auto cfg) -> int {
                using C = decltype(cfg);
                auto kern = C::kernel();
                const auto kern_tail = C::kernel_tail();
                constexpr size_t wlds = C::lds_bytes;
                constexpr int threads = C::threads, region_px = C::region_px;
                // grid size: region_grid_hint -- unless the caller handed over a host copy of the table: then the grid is chosen for this
                // launch (region_grid_choice) and exactly N x regions x M workgroups are launched
                const bool tail_kernel = SEMIDETR_RW_TAIL && C::has_tail;
                const int dev_cus = device_cus();
                const GridChoice gc = region_grid_choice(0, grid_geom(0, L), host_shapes, L, N, M, dev_cus, tail_kernel);
                const int wbound = gc.regions ? gc.regions : region_grid_hint(S, L, region_px);
                // + one helper workgroup per CU for the tail split (msda_rw.h: the units of the last, partly filled wave of workgroups are
                // cut into parts; one workgroup per CU is what the kernel's LDS allows).  SEMIDETR_RW_TAIL=0 builds do without.
                // Only launches of fewer than ~three waves of workgroups get them (the kernel's own rule, from the real region count): on a
                // bs-4 launch 256 idle helpers, each waiting for a whole CU to read the level table and leave, cost 7 us of 154.
                // (level table known: where the chooser's model says the split pays for the grid it picked)
                const int cus = tail_kernel ? dev_cus : 0;
                const int tail = gc.regions ? (gc.tail ? cus : 0)
                                            : ((int64_t)N * M * finest_level_regions(S, region_px) < (int64_t)3 * cus ? cus : 0);
                if (tail > 0) kern = kern_tail;
                if (int rc = allow_big_lds(kern, wlds, "msda_forward")) {      // refused for this instantiation: the patch kernel below
                    fell_back = true;
                    return rc;
                }
                SEMIDETR_REQUIRE((int64_t)N * wbound * M + tail < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_forward: grid too large");
                hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)N * wbound * M + tail)), dim3(threads), wlds, st, (const float *)nullptr,
                                   value, spatial_shapes, level_start, io, S, M, wbound, out, (float4 *)nullptr, (int64_t)0, fs, tail, gc.nry, gc.nrx);
                g_last_kernels = "msda_rw_d32";
                return semidetr::launch_status("msda_rw_d32<forward>");
            };
            auto pick_window = [&]() -> int {
                if constexpr (std::is_same<IO, RawIO>::value) {
                    if (io.has_mask()) return L == 4 ? launch_window(RwProduct<IO, 4, true>{}) : launch_window(RwProduct<IO, 5, true>{});
                }
                return L == 4 ? launch_window(RwProduct<IO, 4, false>{}) : launch_window(RwProduct<IO, 5, false>{});
            };
            const int wrc = pick_window();
            if (!fell_back) return wrc;
            (void)hipGetLastError();
            fs = FwdStats{nullptr, 0u};      // (this launch's counter parity was the window kernel's: count nothing)
        }
        // 4 x 8 query patches
        const int bound = patch_grid_hint(S, L, 32);
        SEMIDETR_REQUIRE((int64_t)N * bound * M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_forward: grid too large");
        hipLaunchKernelGGL((msda_fwd_d32<1, 4, patch_hw(4, 8), IO>), dim3((unsigned)((int64_t)N * bound * M)), dim3(256),
                           (size_t)32 * (L * P + 1) * 32, st, value, spatial_shapes, level_start, io, S, M, L, Lq, P, bound, out, fs);
        g_last_kernels = "msda_fwd_d32<1, 4, 408";
        return semidetr::launch_status("msda_fwd_d32<patch>");
    }
    int split = pick_split(0, N, Lq, M);
    // the records of a workgroup's rows have to fit the 64 KB every kernel may use without asking (L * P up to 256 is on this
    // path: 32 rows x 257 records x 32 bytes would be 263 KB): fewer rows per workgroup for the very wide cases
    while (split < 4 && (size_t)(32 / split) * (L * P + 1) * 32 > 64 * 1024) split *= 2;
    const int rpb = 32 / split;
    const int tiles = (Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)N * tiles * M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_forward: grid too large");
    const size_t lds = (size_t)rpb * (L * P + 1) * 32;
    if (int rc = allow_big_lds(&msda_fwd_d32<4, 4, 0, IO>, lds, "msda_forward")) return rc;      // only L * P > 255 at 8 rows
    if (split == 1) LAUNCH_FWD(1, 0, tiles, lds);
    else if (split == 2) LAUNCH_FWD(2, 0, tiles, lds);
    else LAUNCH_FWD(4, 0, tiles, lds);
#undef LAUNCH_FWD
    g_last_kernels = split == 1 ? "msda_fwd_d32<1, 4, 0" : (split == 2 ? "msda_fwd_d32<2, 4, 0" : "msda_fwd_d32<4, 4, 0");
    return semidetr::launch_status("msda_fwd_d32");
}

// ---- backward, encoder self-attention: patch gather (the two small gradients; it clears grad_value as a side job, the
//      scatter that accumulates into it is the NEXT launch) + region-owned scatter (msda_region.h).  fill: bytes of grad_value
template <typename IO>
int launch_encoder_backward(hipStream_t st, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                            const int64_t *level_start, const IO &io, int N, int S, int M, int L, int Lq, int P,
                            int flags, float *grad_value, const int64_t *host_shapes, size_t fill)
{
    const bool fill_in_gather = !SEMIDETR_SEPARATE_FILL && (L * P == 16 || L * P == 20) && (reinterpret_cast<uintptr_t>(grad_value) & 15) == 0;
    if (!fill_in_gather) {
        const hipError_t e = hipMemsetAsync(grad_value, 0, fill, st);
        if (e != hipSuccess) return semidetr::fail((int)e, "msda_backward memset: %s", hipGetErrorString(e));
    }
    const size_t glds = (size_t)32 * (L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float);
    const int gbound = patch_grid_hint(S, L, 32);
    const int gt = (Lq + 31) / 32;
    SEMIDETR_REQUIRE((int64_t)N * std::max(gbound, gt) * M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward: grid too large");
    float4 *zero = fill_in_gather ? reinterpret_cast<float4 *>(grad_value) : nullptr;
    bool window_gather = false;
    // (SEMIDETR_MSDA_FIXED_FORWARD: which gather runs must not depend on earlier launches either -- the patch gather)
    // (Lq * M * L * P * 8 bytes per image < 2^32: msda_gw_d32 indexes the sampling data inside an image with 32 bits)
    // (SEMIDETR_MSDA_GATHER_WINDOW / _PATCH: the caller's record of what the slot said when the matching forward ran; neither: its state now)
    const bool near = (flags & SEMIDETR_MSDA_GATHER_WINDOW) ? true : ((flags & SEMIDETR_MSDA_GATHER_PATCH) ? false : slot_samples_are_near((flags >> 8) & 0xff));
    if ((L == 4 || L == 5) && P == kPT && (fill_in_gather || SEMIDETR_SEPARATE_FILL) && !(flags & SEMIDETR_MSDA_FIXED_FORWARD) && near &&
        (uint64_t)Lq * M * L * P * 8 < (1ull << 32)) {
        // lane-per-sample gather on region windows (msda_gw.h).  cfg: the GwProduct to run
        auto launch_gw = [&](auto cfg) -> bool {
            using C = decltype(cfg);
            const auto kern = C::kernel();
            if (allow_big_lds(kern, C::lds_bytes, "msda_backward") != SEMIDETR_OK) {      // refused: the patch gather below
                (void)hipGetLastError();
                return false;
            }
            // (the region grid and, with the level table on the host, the exact grid size: region_grid_choice)
            const GridChoice gc = region_grid_choice(1, grid_geom(1, L), host_shapes, L, N, M, device_cus(), false);
            const int wbound = gc.regions ? gc.regions : region_grid_hint(S, L, C::region_px);
            if ((int64_t)N * wbound * M >= INT32_MAX) return false;
            hipLaunchKernelGGL(kern, dim3((unsigned)((int64_t)N * wbound * M)), dim3(C::threads), C::lds_bytes, st, grad_out, value, spatial_shapes,
                               level_start, io, S, M, wbound, zero, (int64_t)(fill / 16), gc.nry, gc.nrx);
            return true;
        };
        if constexpr (std::is_same<IO, RawIO>::value) {
            if (io.has_mask()) window_gather = L == 4 ? launch_gw(GwProduct<IO, 4, true>{}) : launch_gw(GwProduct<IO, 5, true>{});
        }
        if (!window_gather && !io.has_mask()) window_gather = L == 4 ? launch_gw(GwProduct<IO, 4, false>{}) : launch_gw(GwProduct<IO, 5, false>{});
    }
    if (!window_gather) {
        if (L * P == 16)             // DINO: sample loop unrolled, results in registers
            hipLaunchKernelGGL((msda_bwd_gather_d32<IO, 16, patch_hw(4, 8), SEMIDETR_GATHER_WPE, SEMIDETR_GATHER_KB>), dim3((unsigned)((int64_t)N * gbound * M)), dim3(256), glds, st,
                               grad_out, value, spatial_shapes, level_start, io, S, M, L, Lq, P, gbound, zero, (int64_t)(fill / 16));
        else if (L * P == 20)        // five levels (COCO-Full recipe)
        {
            // (the fused prologue's instantiation holds its softmax / location arithmetic besides: with 16 corner loads in flight it
            //  spills at four waves per SIMD since it also carries the padding mask's summary -- 8 in flight: 98 registers)
            constexpr int kb5 = std::is_same<IO, RawIO>::value ? 2 : SEMIDETR_GATHER5_KB;
            hipLaunchKernelGGL((msda_bwd_gather_d32<IO, 20, patch_hw(4, 8), SEMIDETR_GATHER5_WPE, kb5>), dim3((unsigned)((int64_t)N * gbound * M)), dim3(256), glds, st,
                               grad_out, value, spatial_shapes, level_start, io, S, M, L, Lq, P, gbound, zero, (int64_t)(fill / 16));
        }
        else
            hipLaunchKernelGGL((msda_bwd_gather_d32<IO, 0>), dim3((unsigned)((int64_t)N * gt * M)), dim3(256), glds, st,
                               grad_out, value, spatial_shapes, level_start, io, S, M, L, Lq, P, gt);
    }
    if (int rc = semidetr::launch_status(window_gather ? "msda_gw_d32" : "msda_bwd_gather_d32")) return rc;
#if SEMIDETR_SCATTER_SW
    {
        auto kern = &msda_sw_d32<IO, SEMIDETR_SW_NT, SEMIDETR_SW_Q, SEMIDETR_SW_RTH, SEMIDETR_SW_RTW, SEMIDETR_SW_WH, SEMIDETR_SW_WW, SEMIDETR_SW_WPE>;
        constexpr size_t rlds = sw_lds_bytes<SEMIDETR_SW_NT, SEMIDETR_SW_Q, SEMIDETR_SW_WH, SEMIDETR_SW_WW>();
        if (int rc = allow_big_lds(kern, rlds, "msda_backward")) return rc;
        const int rbound = (S * 3 / 4 + SEMIDETR_SW_RTH * SEMIDETR_SW_RTW - 1) / (SEMIDETR_SW_RTH * SEMIDETR_SW_RTW) * 9 / 8 + 4 * L;
        const int64_t rgrid = (int64_t)N * rbound * M;
        SEMIDETR_REQUIRE(rgrid < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward: grid too large");
        hipLaunchKernelGGL(kern, dim3((unsigned)rgrid), dim3(SEMIDETR_SW_NT), rlds, st, grad_out, spatial_shapes, level_start, io, S, M, L,
                           rbound, grad_value);
        g_last_kernels = window_gather ? "msda_gw_d32+msda_sw_d32" : "msda_bwd_gather_d32+msda_sw_d32";
        return semidetr::launch_status("msda_sw_d32");
    }
#endif
    using Sc = ScatterProduct<IO>;
    const auto kern = Sc::kernel();
    if (int rc = allow_big_lds(kern, Sc::lds_bytes, "msda_backward")) return rc;
    // grid size: region_grid_hint as for the window kernels; with the level table on the host the region grid is chosen for this launch
    // and the grid size is exact (region_grid_choice)
    const GridChoice gc = region_grid_choice(2, grid_geom(2, L), host_shapes, L, N, M, device_cus(), false);
    const int rbound = gc.regions ? gc.regions
                       : (SEMIDETR_SCATTER_TIGHT ? region_grid_hint(S, L, Sc::region_px) : region_grid_hint_loose(S, L, Sc::region_px));
    const int64_t rgrid = (int64_t)N * rbound * M;
    SEMIDETR_REQUIRE(rgrid < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward: grid too large");
    hipLaunchKernelGGL(kern, dim3((unsigned)rgrid), dim3(Sc::threads), Sc::lds_bytes, st, grad_out, spatial_shapes, level_start, io, S, M, L,
                       rbound, grad_value, gc.nry, gc.nrx);
    g_last_kernels = window_gather ? "msda_gw_d32+msda_bwd_scatter_d32_reg"
                     : (fill_in_gather ? "msda_bwd_gather_d32+msda_bwd_scatter_d32_reg"
                                       : "fillBufferAligned+msda_bwd_gather_d32+msda_bwd_scatter_d32_reg");
    return semidetr::launch_status("msda_bwd_scatter_d32_reg");
}

// ---- backward, any query set: the merged level kernel, or one small fused kernel after the fill.  fill: bytes of grad_value
template <typename IO>
int launch_query_set_backward(hipStream_t st, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                              const int64_t *level_start, const IO &io, int N, int S, int M, int L, int Lq, int P,
                              float *grad_value, size_t fill)
{
    hipError_t e = hipMemsetAsync(grad_value, 0, fill, st);
    if (e != hipSuccess) return semidetr::fail((int)e, "msda_backward memset: %s", hipGetErrorString(e));
    // (four gather blocks of 2 * 32 * (L * P + 1) records share a merged workgroup's LDS: beyond L * P = 36 the launch takes
    //  the strips kernel below)
    const size_t merged_gather_lds = (size_t)(kLvlThreadsWide / 256) * ((size_t)2 * 32 * (L * P + 1) + 2 * kMaxLevels / 4 + 4) * 16;
    // (S < 2^20: lvl_scatter_body packs a level-local row index into 20 bits of its entry word -- ADVICE r03; larger maps take
    //  the strips kernel below)
    if ((int64_t)N * Lq >= 512 && P <= 8 && merged_gather_lds <= 159 * 1024 && S < (1 << 20)) {
        // level-aggregated scatter workgroups + gather workgroups side by side in ONE launch (msda_bwd_lvl_merged_wide).
        // bucketed levels: as many queries per workgroup as its LDS takes (fewest flushed rows); levels too large to bucket:
        // <= 192 queries per workgroup (parallelism), and enough workgroups for small launches
        const int qcap = P <= 4 ? kLvlQWide : kLvlQWide / 2;             // the entry list is chunk * P * 4 * 8 bytes
        const int want = (128 + N * L * M - 1) / (N * L * M);            // small launches: >= ~128 scatter workgroups
        const int fine = std::min(want, (Lq + 63) / 64);
        // ONE chunk for the bucketed levels whenever the queries fit (Lq <= 384, the two-stage Deformable-DETR / BASELINE shape):
        // the workgroup then owns the level's rows of its (image, head) and STORES their sums instead of adding them atomically
        // (lvl_scatter_body, "exclusive") -- micro-benchmark backward 36.3 -> 30.7 us, bs 4 / Lq 300 63 -> 53 us
        const int chunks_b = Lq <= qcap ? 1 : std::max((Lq + qcap - 1) / qcap, fine), chunk_q_b = (Lq + chunks_b - 1) / chunks_b;
        const int chunks = std::max(std::max(chunks_b, fine), (Lq + SEMIDETR_LVL_CHUNKQ - 1) / SEMIDETR_LVL_CHUNKQ);
        const int chunk_q = (Lq + chunks - 1) / chunks;
        const int gt = (Lq + 31) / 32;                                   // gather: 32 query rows per 256-thread block
        const int64_t gblocks = (int64_t)N * gt * M, sblocks = (int64_t)N * chunks * L * M;
        const size_t half_f4 = (size_t)2 * 32 * (L * P + 1) + 2 * kMaxLevels / 4 + 4;
        constexpr int kParts = kLvlThreadsWide / 256;                    // gather blocks per workgroup
        const size_t slds = std::max((size_t)kLvlQWide * kD * 4 + ((size_t)chunk_q_b * P * 4 + 8) * 8 + (size_t)2 * kLvlRows * 4,
                                     kParts * half_f4 * 16);
        const int64_t grid = sblocks + (gblocks + kParts - 1) / kParts;
        SEMIDETR_REQUIRE(grid < INT32_MAX && slds <= 159 * 1024, SEMIDETR_E_TOOLARGE, "msda_backward: merged launch too large");
#define LAUNCH_MERGED(KLP_)                                                                                          \
        do {                                                                                                             \
            auto kern = &msda_bwd_lvl_merged_wide<IO, KLP_>;                                                             \
            if (int rc = allow_big_lds(kern, slds, "msda_backward")) return rc;                                          \
            hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kLvlThreadsWide), slds, st, grad_out, value, spatial_shapes, \
                               level_start, io, S, M, L, Lq, P, chunks, chunk_q, chunks_b, chunk_q_b, (int)sblocks, gt, (int)gblocks,      \
                               grad_value);                                                                              \
        } while (0)
        if (L * P == 16) LAUNCH_MERGED(16);
        else LAUNCH_MERGED(0);
#undef LAUNCH_MERGED
        g_last_kernels = "fillBufferAligned+msda_bwd_lvl_merged_wide";
        return semidetr::launch_status("msda_bwd_lvl_merged_wide");
    }
    // small launches: one fused kernel after the fill; 32 query rows per workgroup, 8 when that would not fill 256 CUs
    // (and 8 when 32 rows of records would not fit 64 KB of LDS: L * P > 62)
    const int rpb = ((int64_t)N * M * ((Lq + 31) / 32) >= 1024 && (size_t)32 * (L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float) <= 64 * 1024) ? 32 : 8;
    const int tiles = (Lq + rpb - 1) / rpb;
    const int64_t grid = (int64_t)N * tiles * M;
    SEMIDETR_REQUIRE(grid < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward: grid too large");
    const size_t lds = (size_t)rpb * (L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float);
    if (int rc = allow_big_lds(&msda_bwd_d32<8, IO>, lds, "msda_backward")) return rc;      // only L * P > 254 at 8 rows
    if (rpb == 32)
        hipLaunchKernelGGL((msda_bwd_d32<32, IO>), dim3((unsigned)grid), dim3(256), lds, st, grad_out, value, spatial_shapes,
                           level_start, io, S, M, L, Lq, P, tiles, grad_value);
    else
        hipLaunchKernelGGL((msda_bwd_d32<8, IO>), dim3((unsigned)grid), dim3(256), lds, st, grad_out, value, spatial_shapes,
                           level_start, io, S, M, L, Lq, P, tiles, grad_value);
    g_last_kernels = rpb == 32 ? "fillBufferAligned+msda_bwd_d32<32" : "fillBufferAligned+msda_bwd_d32<8";
    return semidetr::launch_status("msda_bwd_d32");
}

template <typename IO>
int launch_fast_backward(hipStream_t st, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const IO &io, int N, int S, int M, int L, int Lq, int P,
                         int flags, float *grad_value, const int64_t *host_shapes = nullptr)
{
    SEMIDETR_REQUIRE(!(flags & SEMIDETR_MSDA_QUERIES_ARE_PIXELS) || Lq == S, SEMIDETR_E_BADARG,
                     "msda_backward: SEMIDETR_MSDA_QUERIES_ARE_PIXELS needs num_query == spatial_size");
    const bool pixels = (flags & SEMIDETR_MSDA_QUERIES_ARE_PIXELS) != 0 && (size_t)32 * (L * P + 1) * 32 <= 63 * 1024;
    const size_t fill = sizeof(float) * (size_t)N * S * M * kD;
    // (S * M * 128 < 2^32: the region scatter addresses grad_value rows by 32-bit byte offsets from the image's first row)
    // (... and its sampling data inside the image's view with 32-bit indices: S * M * L * P * 8 < 2^32)
    // (M * 128 <= 0xffff: the region scatter's flush multiplies a 16-bit pixel key by the row pitch into 32 bits -- implied by heads_ok,
    //  stated here because the kernel's inline assembly depends on it)
    if (pixels && P == kPT && S < (1 << 23) && (uint64_t)S * M * kD * 4 < (1ull << 32) && (uint64_t)S * M * L * P * 8 < (1ull << 32) &&
        (int64_t)M * kD * 4 <= 0xffff)
        return launch_encoder_backward(st, grad_out, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, flags, grad_value, host_shapes, fill);
    return launch_query_set_backward(st, grad_out, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, grad_value, fill);
}

}  // namespace

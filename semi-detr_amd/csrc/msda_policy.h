// The data-driven kernel choice of the encoder self-attention: which forward kernel a call site's launches take (fwd_adapt_next) and
// which gather its backward takes (slot_samples_are_near), from what the forward kernels counted about their samples.  Per-device host
// state behind a mutex + mapped pinned memory.  Included by msda.hip after the kernel headers (FwdStats: msda_fast.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"

namespace {

// ---- which kernel runs the encoder self-attention forward: the patch kernel (msda_fwd_d32<1,4,408>) or the region-window
//      kernel (msda_rw_d32, LDS windows +- 5 px around a region, five levels +- 4 px).  The second is ~30 % faster while the learned
//      offsets keep most samples within a few pixels of their queries (sigma <= 2 px: 162 against 234 us at bs 4 inside the step) and slower
//      once ~70 % of them are further than 4 px away (sigma ~5.5 px; profiles/r04_region_window_dispatch.txt), so the choice
//      follows the DATA: both kernels count how far their samples reach (FwdStats, msda_fast.h), the count of launch k is
//      handed to the host by the first thread of launch k + 1 through mapped pinned memory, and the dispatcher -- whenever it
//      next gets here, it never waits -- moves between the kernels with hysteresis.  Per (device, call-site slot); a mutex serialises
//      the few host words.  semidetr_msda_set_forward_policy pins the choice (tests, A/B timing).
// Thresholds re-measured with the 768 / 1024-thread window kernels (tools/archive/r04_rw_cross2.sh, rotated inputs, bs 4): four levels 233 /
// 243 / 251 / 261 / 283 us against the patch kernel's 270-273 us at sigma 3.5 / 4 / 4.5 / 5 / 6 px -- level at ~5.5 px = a far share of
// ~0.71; five levels level at ~5 px = ~0.67.  One image alone (616 regions x heads for 256 CUs) used to need its own, lower bound;
// the larger workgroups removed the difference (57 / 63 / 65.5 / 68.5 against 68 / 70.5 / 71.5 / 72 us at 2 / 3 / 3.5 / 4 px).
// Round 5 (the window kernel's geometry halved, tools/r05_crossover.sh): four levels, bs 4: 193 / 213 / 232 / 246 / 255 / 260 us against the patch
// kernel's 263-270 at sigma 3 / 4 / 5 / 6 / 7 / 8 px -- level beyond 8 px (far share 0.85); one image: 56 / 63 / 68 / 70.5 / 74.5 against 70-71 --
// level at ~6 px (0.76).  The band moves from 0.60 / 0.70 to 0.72 / 0.80.
// Round 6 (tools/r06_spread.sh, profiles/r06_sample_patterns.txt; Gaussian spreads AND the reference's own initial offset star,
// ops/modules/ms_deform_attn.py:62-70): four levels, bs 4 -- window 197 / 215 / 229 / 246 us against the patch kernel's 250 / 253 / 253 / 249 at sigma
// 4 / 5 / 6 / 8 px (far share 0.53 / 0.67 / 0.76 / 0.85): level at ~0.85; star 140 against 222, star x 2 (far share 0.57) 200 against 220.  Five levels:
// window 233 / 252 / 261 / 274 against 299 / 301 / 301 / 298 -- ahead at every spread measured (round 5's band 0.56 / 0.66 predates the level table and
// the compact records in the five-level kernel and sent sigma >= 5 px to the patch kernel: 301 instead of 252 us).
constexpr float kFarToWindow = 0.78f;      // patch -> window when fewer than this share of the samples are far ...
constexpr float kFarToPatch = 0.86f;       // ... window -> patch above this one
constexpr float kFarToWindow5 = 0.82f, kFarToPatch5 = 0.90f;      // five levels (COCO-Full pyramid)
// Per CALL SITE (round 5): the reference builds twelve MSDeformAttn instances per model (transformer.py:609,760) whose learned offsets
// reach differently far, so the state is kept per (device, slot): the caller names the slot in bits 8..15 of `flags`
// (SEMIDETR_MSDA_POLICY_SLOT; the Python module gives every instance its own), slot 0 is the state every caller that names none shares.
// A slot's counts come from its own launches only and are judged by the thresholds of its own pyramid.
constexpr int kPolicySlots = 256;
struct FwdSlot {
    unsigned launches = 0, seen_seq = 0, updates = 0;
    int mode = 0;                          // 0 = patch kernel, 1 = region-window kernel
    float last_frac = -1.f;
};
struct FwdAdapt {
    unsigned *dev_cnt = nullptr;           // device words per slot: {far, total, kind, -} x launch parity, [8] = publications so far
    unsigned *pub_host = nullptr;          // mapped pinned memory per slot: {sequence, far, total, kind}
    unsigned *pub_dev = nullptr;           // the same memory as the device sees it
    bool failed = false;                   // allocation failed once: stay with the patch kernel, silently
    FwdSlot slot[kPolicySlots];
};
constexpr int kMaxDevices = 64;
std::mutex g_adapt_mu;
FwdAdapt *g_adapt[kMaxDevices];            // allocated at a device's first adaptive dispatch
std::atomic<int> g_fwd_policy{0};          // 0 adaptive, 1 always the patch kernel, 2 the window kernel whenever it applies

// compute units of the current device (cached per device index; 0 if the runtime will not say: the callers then do without)
int device_cus()
{
    static std::atomic<int> cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int c = cus[dev].load(std::memory_order_relaxed);
    if (c == 0) {
        int v = 0;
        c = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : -1;
        cus[dev].store(c, std::memory_order_relaxed);
    }
    return c > 0 ? c : 0;
}

// the launch's FwdStats and the kernel to use; called with the stream the launch goes to
int fwd_adapt_next(hipStream_t st, bool allow_window, int slot_id, int levels, FwdStats &fs, bool &use_window)
{
    fs = FwdStats{nullptr, 0u};
    const int policy = g_fwd_policy.load(std::memory_order_relaxed);
    use_window = allow_window && policy == 2;
    if (policy != 0 || !allow_window) return SEMIDETR_OK;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return SEMIDETR_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lock(g_adapt_mu);
    if (!g_adapt[dev]) g_adapt[dev] = new (std::nothrow) FwdAdapt();
    if (!g_adapt[dev]) return SEMIDETR_OK;
    FwdAdapt &a = *g_adapt[dev];
    if (!a.dev_cnt && !a.failed && !capturing) {       // first use on this device (never inside a stream capture): two small
        // allocations and a SYNCHRONOUS clear (ONCE per process and device; the allocations may synchronise anyway).  The counter block
        // is shared by every slot and every stream of the device: a clear merely queued on the first launch's stream could run after
        // another stream's first counting launch had started adding.
        void *h = nullptr, *d = nullptr, *c = nullptr;
        // (the device block of a slot: counters zero, words [10..11] = where the slot's record lives in the mapped host memory -- FwdStats)
        std::vector<unsigned> init((size_t)kPolicySlots * 16, 0u);
        if (hipHostMalloc(&h, kPolicySlots * 16, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess &&
            hipMalloc(&c, kPolicySlots * 64) == hipSuccess) {
            for (int sid = 0; sid < kPolicySlots; ++sid) {
                const unsigned *pp = static_cast<unsigned *>(d) + 4 * sid;
                std::memcpy(&init[(size_t)sid * 16 + 10], &pp, sizeof(pp));
            }
        }
        if (h && d && c && hipMemcpy(c, init.data(), init.size() * sizeof(unsigned), hipMemcpyHostToDevice) == hipSuccess) {
            std::fill_n(static_cast<unsigned *>(h), kPolicySlots * 4, 0u);
            a.pub_host = static_cast<unsigned *>(h);
            a.pub_dev = static_cast<unsigned *>(d);
            a.dev_cnt = static_cast<unsigned *>(c);
        } else {
            (void)hipGetLastError();
            a.failed = true;
        }
    }
    FwdSlot &sl = a.slot[slot_id & (kPolicySlots - 1)];
    if (a.dev_cnt) {
        const int sid = slot_id & (kPolicySlots - 1);
        volatile unsigned *pub = a.pub_host + 4 * sid;
        const unsigned seq = pub[0];
        if (seq != sl.seen_seq) {                      // a finished launch's counts have arrived since the last look
            const unsigned far = pub[1], total = pub[2];
            if (pub[0] != seq || far > total) {        // caught between two records (the device writes 16 bytes at once,
                                                       // so this is paranoia): look again at the next dispatch
            } else if (total) {
                sl.seen_seq = seq;
                sl.last_frac = (float)far / (float)total;
                ++sl.updates;
                if (sl.mode == 0 && sl.last_frac < (levels == 5 ? kFarToWindow5 : kFarToWindow)) sl.mode = 1;
                else if (sl.mode == 1 && sl.last_frac > (levels == 5 ? kFarToPatch5 : kFarToPatch)) sl.mode = 0;
            }
        }
        if (!capturing) {                              // a captured launch keeps the kernel of the moment and counts nothing
            const unsigned par = sl.launches++ & 1u;
            unsigned *base = a.dev_cnt + 16 * sid;
            fs = FwdStats{base, par};
        }
    }
    use_window = sl.mode == 1;
    return SEMIDETR_OK;
}

// What the slot's forward launches counted about its samples, for the BACKWARD's gather (same data, one forward earlier): true = few enough
// of them are far from their queries for the lane-per-sample window gather (msda_gw.h) to pay.  It crosses the patch gather earlier
// than the window forward crosses the patch forward (tools/r05_gw_sigma.sh, bs 4, whole backward: 572 / 635 / 796 / 976 / 1157 us
// against 659 / 707 / 834 / 986 / 1111 us at sigma 1 / 2 / 3 / 4 / 5 px; bs 1 level at 3 px): below a far share of ~0.45
// (sigma ~3.5 px).  Reads the state, counts nothing; no count received yet = the patch gather.
// Round 6, with a round's grad_out rows in LDS (same script): whole backward, four levels, window gather 644 / 794 / 933 / 1091 us against the patch
// gather's 715 / 830 / 933 / 1062 at sigma 3 / 4 / 5 / 6 px (far share 0.33 / 0.53 / 0.67 / 0.76); the reference's star 490 against 577, but the star
// twice as far (far share 0.57: half the samples 6 and 8 px out, all of them on the cooperative path) 620 against 574 -- the patch gather profits from
// the star's regularity.  Five levels: 761 / 910 / 1072 against 856 / 965 / 1088 at sigma 3 / 4 / 5 px, star x 2 794 against 770.  0.45 -> 0.55.
constexpr float kFarToWindowGather = 0.55f;
bool slot_samples_are_near(int slot_id)
{
    const int policy = g_fwd_policy.load(std::memory_order_relaxed);
    if (policy != 0) return policy == 2;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
    std::lock_guard<std::mutex> lock(g_adapt_mu);
    if (!g_adapt[dev]) return false;
    const FwdSlot &sl = g_adapt[dev]->slot[slot_id & (kPolicySlots - 1)];
    return sl.updates > 0 && sl.last_frac >= 0.f && sl.last_frac < kFarToWindowGather;
}

}  // namespace

// Multi-scale deformable attention for gfx950 (MI355X, CDNA4): forward + backward, C-ABI entry points.
//
// Behavioural spec = the reference CUDA op (detr_od/models/utils/ops/src/cuda/ms_deform_im2col_cuda.cuh:
// forward :237-299 with bilinear fetch :33-84; backward :301-403 with scatter :87-159), re-designed for
// 64-wide wavefronts and the measured behaviour of this chip's atomic units -- not a translation.
//
// This file: the include order of the kernel headers, the generic path (any D, fp32 / fp64: one wavefront per (n, q, m) row,
// lanes stride the channels), the padding-mask summary kernel and the C-ABI entry points.  The host side of the fast path has one
// header per concern: msda_tuning.h (every SEMIDETR_* knob), msda_grid.h (region-grid chooser), msda_policy.h (data-driven kernel
// choice), msda_dispatch.h (the window kernels' product configurations and the two launch functions).  msda_fast.h: the fp32 /
// D == 32 kernels (the DINO-DETR shape):
//  * forward: a 256-thread workgroup owns 32 queries of ONE (image, head) -- an 8 x 4 pixel patch for encoder
//    self-attention, 32 consecutive queries otherwise.  Workgroups are numbered head-fastest, so with the
//    observed block -> XCD round-robin every XCD's private 4 MiB L2 only sees value rows of "its" heads
//    (one head of one image = S * 128 B = 2.8 MB at 800x1333).  Phase 1 turns the tile's sampling locations /
//    attention weights into per-sample records {4 corner offsets, 4 weights} in LDS (the reference recomputes
//    them in all 32 channel threads and re-reads the int64 level table per sample); phase 2 covers one
//    128-byte value row with 8 lanes x float4, so every global_load_dwordx4 moves 8 complete cache lines.
//  * backward, any query set: 32 lanes per value row (lane = channel) so each global_atomic_add_f32
//    wave-instruction updates two COMPLETE lines (the L2 atomic unit charges per 64-byte half-line touched:
//    tools/atomic_probe.hip); channel sums for grad_attn / grad_loc by DPP inside the half-wave; small
//    gradients staged in LDS and written back coalesced.
//  * backward, encoder self-attention: a streaming gather kernel for the small gradients + an owner-computes
//    scatter kernel that buckets (sample, corner) pairs by target row in LDS with integer atomics only
//    (ds_add_f32 is lane-serial on gfx950: tools/lds_atomic_probe.hip) and issues one atomic per row run.
//  * every fast-path kernel is a template over an IO policy: the reference op contract (locations +
//    softmaxed weights) or the fused MSDeformAttn prologue (reference points + raw offsets + raw logits).
//
// Coordinates are computed WITHOUT fma contraction so cell selection (floor) is bit-identical to the
// CPU oracle; everything downstream may contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#if SEMIDETR_EXPERIMENTS
#include "semidetr_hip_experiments.h"
#endif
#include "msda_tuning.h" // every SEMIDETR_* knob of this unit, before anything reads one

namespace {

constexpr int kMaxLevels = 32;

#include "msda_geom.h"   // sample geometry (mul_rn / sub_rn, sample_setup[_oob], kOob) + raw-buffer loads, shared with msda_h16.hip

__device__ __forceinline__ void fp_atomic_add(float *p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void fp_atomic_add(double *p, double v) { unsafeAtomicAdd(p, v); }

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
// generic path: one wavefront per (n, q, m) row
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void msda_fwd_generic(
    const T *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
    const T *__restrict__ loc, const T *__restrict__ attn, int N, int S, int M, int D, int L, int Lq,
    int P, T *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)N * Lq * M) return;
    const int m = (int)(row % M);
    const int n = (int)(row / ((int64_t)M * Lq));
    const T *vb = value + ((int64_t)n * S * M + m) * D;
    const T *lrow = loc + row * L * P * 2;
    const T *arow = attn + row * L * P;
    const int rs = M * D;
    for (int c0 = 0; c0 < D; c0 += 64) {
        const int c = c0 + lane;
        const bool act = c < D;
        T acc = 0;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
            for (int p = 0; p < P; ++p) {
                int off[4];
                T lw, lh;
                const T x = lrow[(l * P + p) * 2], y = lrow[(l * P + p) * 2 + 1];
                if (!sample_setup(x, y, H, W, st, rs, off, lw, lh)) continue;
                const T a = arow[l * P + p];
                const T hh = 1 - lh, hw = 1 - lw;
                if (act) {
                    const T v1 = off[0] >= 0 ? vb[off[0] + c] : (T)0;
                    const T v2 = off[1] >= 0 ? vb[off[1] + c] : (T)0;
                    const T v3 = off[2] >= 0 ? vb[off[2] + c] : (T)0;
                    const T v4 = off[3] >= 0 ? vb[off[3] + c] : (T)0;
                    acc += a * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4);
                }
            }
        }
        if (act) out[row * D + c] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void msda_bwd_generic(
    const T *__restrict__ gout, const T *__restrict__ value, const int64_t *__restrict__ shapes,
    const int64_t *__restrict__ starts, const T *__restrict__ loc, const T *__restrict__ attn, int N,
    int S, int M, int D, int L, int Lq, int P, T *__restrict__ gvalue, T *__restrict__ gloc,
    T *__restrict__ gattn)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)N * Lq * M) return;
    const int m = (int)(row % M);
    const int n = (int)(row / ((int64_t)M * Lq));
    const int64_t vo = ((int64_t)n * S * M + m) * D;
    const T *vb = value + vo;
    T *gvb = gvalue + vo;
    const T *lrow = loc + row * L * P * 2;
    const T *arow = attn + row * L * P;
    const T *grow = gout + row * D;
    const int rs = M * D;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
        for (int p = 0; p < P; ++p) {
            int off[4];
            T lw, lh;
            const T x = lrow[(l * P + p) * 2], y = lrow[(l * P + p) * 2 + 1];
            const bool inside = sample_setup(x, y, H, W, st, rs, off, lw, lh);
            T s_attn = 0, s_x = 0, s_y = 0;
            if (inside) {
                const T a = arow[l * P + p];
                const T hh = 1 - lh, hw = 1 - lw;
                const T w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
                for (int c = lane; c < D; c += 64) {
                    const T g = grow[c], ga = g * a;
                    T v1 = 0, v2 = 0, v3 = 0, v4 = 0;
                    if (off[0] >= 0) { v1 = vb[off[0] + c]; fp_atomic_add(gvb + off[0] + c, w1 * ga); }
                    if (off[1] >= 0) { v2 = vb[off[1] + c]; fp_atomic_add(gvb + off[1] + c, w2 * ga); }
                    if (off[2] >= 0) { v3 = vb[off[2] + c]; fp_atomic_add(gvb + off[2] + c, w3 * ga); }
                    if (off[3] >= 0) { v4 = vb[off[3] + c]; fp_atomic_add(gvb + off[3] + c, w4 * ga); }
                    s_attn += g * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
                    s_x += ga * (hh * (v2 - v1) + lh * (v4 - v3));
                    s_y += ga * (hw * (v3 - v1) + lw * (v4 - v2));
                }
                s_attn = wave_sum(s_attn);
                s_x = wave_sum(s_x);
                s_y = wave_sum(s_y);
            }
            if (lane == 0) {
                const int64_t k = row * L * P + l * P + p;
                gattn[k] = s_attn;
                gloc[2 * k] = (T)W * s_x;
                gloc[2 * k + 1] = (T)H * s_y;
            }
        }
    }
}

#include "msda_lanes.h"  // DPP lane reductions + the workgroup -> tile mapping, shared with msda_h16.hip
#include "msda_fast.h"   // IO policies + the D == 32 fp32 kernels
#if SEMIDETR_EXPERIMENTS
#include "msda_fast_experiments.h"   // windowed scatter, resident-level forward, 512-thread merged / cooperative-fill backward
#endif
#include "msda_region.h" // region-owned windowed scatter for encoder self-attention
#include "msda_rw.h"     // region-window forward (product since round 4) / gather (experiments) for encoder self-attention
#include "msda_gw.h"     // lane-per-sample region-window gather for the encoder backward (round 5)
#if SEMIDETR_SCATTER_SW
#include "msda_sw.h"     // cell-sorted region scatter (round 5): measured and rejected, tuning builds only (-DSEMIDETR_SCATTER_SW=1, tools/ab_build.sh)
#endif
#if SEMIDETR_EXPERIMENTS    // negative results kept as evidence: only in libsemidetr_hip_exp.so
#include "msda_dest.h"   // destination-owned grad_value kernel for encoder self-attention
#include "msda_lw.h"     // LDS-window forward for encoder self-attention
#include "msda_own.h"    // owner-computes grad_value for arbitrary query sets
#endif

thread_local const char *g_last_kernels = "";

int check_common(const void *value, const void *shapes, const void *starts, const void *loc,
                 const void *attn, int N, int S, int M, int D, int L, int Lq, int P, size_t elem)
{
    SEMIDETR_REQUIRE(value && shapes && starts && loc && attn, SEMIDETR_E_BADARG, "msda: null pointer argument");
    SEMIDETR_REQUIRE(N > 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq > 0 && P > 0, SEMIDETR_E_BADARG,
                     "msda: sizes must be positive (N=%d S=%d M=%d D=%d L=%d Lq=%d P=%d)", N, S, M, D, L, Lq, P);
    // device index arithmetic inside one image is 32-bit (as in the reference, .cuh:255-269)
    SEMIDETR_REQUIRE((int64_t)(S + 1) * M * D < INT32_MAX, SEMIDETR_E_TOOLARGE,
                     "msda: spatial_size*num_heads*channels = %lld exceeds 32-bit indexing", (long long)S * M * D);
    SEMIDETR_REQUIRE((int64_t)N * Lq * M < INT32_MAX / 4, SEMIDETR_E_TOOLARGE, "msda: too many (n,q,m) rows");
    (void)elem;
    return SEMIDETR_OK;
}

template <typename T>
int forward_impl(void *stream, const T *value, const int64_t *shapes, const int64_t *starts, const T *loc,
                 const T *attn, int N, int S, int M, int D, int L, int Lq, int P, T *out)
{
    if (int rc = check_common(value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, sizeof(T))) return rc;
    SEMIDETR_REQUIRE(out, SEMIDETR_E_BADARG, "msda_forward: null output");
    const int64_t rows = (int64_t)N * Lq * M;
    const int blocks = (int)((rows + 3) / 4);
    hipLaunchKernelGGL(msda_fwd_generic<T>, dim3(blocks), dim3(256), 0, semidetr::as_stream(stream), value,
                       shapes, starts, loc, attn, N, S, M, D, L, Lq, P, out);
    g_last_kernels = "msda_fwd_generic";
    return semidetr::launch_status("msda_fwd_generic");
}

template <typename T>
int backward_impl(void *stream, const T *gout, const T *value, const int64_t *shapes, const int64_t *starts,
                  const T *loc, const T *attn, int N, int S, int M, int D, int L, int Lq, int P, T *gvalue,
                  T *gloc, T *gattn)
{
    if (int rc = check_common(value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, sizeof(T))) return rc;
    SEMIDETR_REQUIRE(gout && gvalue && gloc && gattn, SEMIDETR_E_BADARG, "msda_backward: null pointer argument");
    hipError_t e = hipMemsetAsync(gvalue, 0, sizeof(T) * (size_t)N * S * M * D, semidetr::as_stream(stream));
    if (e != hipSuccess) return semidetr::fail((int)e, "msda_backward memset: %s", hipGetErrorString(e));
    const int64_t rows = (int64_t)N * Lq * M;
    const int blocks = (int)((rows + 3) / 4);
    hipLaunchKernelGGL(msda_bwd_generic<T>, dim3(blocks), dim3(256), 0, semidetr::as_stream(stream), gout,
                       value, shapes, starts, loc, attn, N, S, M, D, L, Lq, P, gvalue, gloc, gattn);
    g_last_kernels = "fillBufferAligned+msda_bwd_generic";
    return semidetr::launch_status("msda_bwd_generic");
}

}  // namespace

// the host side of the fast path, one header per concern (each opens the anonymous namespace itself)
#include "msda_grid.h"       // region-grid chooser of the encoder window kernels: plain C++, also built alone by tests/host/msda_grid_host_check.cpp
#include "msda_policy.h"     // data-driven choice between the patch and the window kernels, per (device, call-site slot)
#include "msda_dispatch.h"   // RwProduct / GwProduct / ScatterProduct, the grid hints, launch_fast_forward / launch_fast_backward
#include "msda_exact.h"      // namespace semidetr_exact: the exact (order-independent) grad_value pipeline of semidetr_msda_backward_exact_f32
#if SEMIDETR_EXPERIMENTS
namespace {
#include "msda_experiments.h"
}  // namespace
#endif

extern "C" const char *semidetr_msda_last_kernels(void) { return g_last_kernels; }

extern "C" int semidetr_msda_set_forward_policy(int policy)
{
    SEMIDETR_REQUIRE(policy >= 0 && policy <= 2, SEMIDETR_E_BADARG, "msda_set_forward_policy: 0 adaptive, 1 patch kernel, 2 window kernel");
    g_fwd_policy.store(policy, std::memory_order_relaxed);
    return SEMIDETR_OK;
}

extern "C" int semidetr_msda_set_region_grid(int kernel, int nry, int nrx)
{
    SEMIDETR_REQUIRE(kernel >= 0 && kernel < kGridKernels, SEMIDETR_E_BADARG, "msda_set_region_grid: kernel 0 forward, 1 gather, 2 scatter");
    SEMIDETR_REQUIRE(nry >= 0 && nrx >= 0 && nry <= kGridMaxAxis && nrx <= kGridMaxAxis && (nry > 0) == (nrx > 0), SEMIDETR_E_BADARG,
                     "msda_set_region_grid: nry and nrx both 0 (automatic) or both in 1..%d", kGridMaxAxis);
    SEMIDETR_REQUIRE((int64_t)nry * nrx <= (1 << 22), SEMIDETR_E_TOOLARGE, "msda_set_region_grid: more than %d regions", 1 << 22);
    g_grid_pin[kernel].store(nry << 16 | nrx, std::memory_order_relaxed);
    return SEMIDETR_OK;
}

extern "C" int semidetr_msda_region_grid_query(int kernel, const int64_t *host_spatial_shapes, int num_levels, int batch, int num_heads,
                                               int num_cus, int *grid6)
{
    SEMIDETR_REQUIRE(kernel >= 0 && kernel < kGridKernels, SEMIDETR_E_BADARG, "msda_region_grid_query: kernel 0 forward, 1 gather, 2 scatter");
    SEMIDETR_REQUIRE(grid6 && num_levels > 0 && batch > 0 && num_heads > 0 && num_cus >= 0, SEMIDETR_E_BADARG,
                     "msda_region_grid_query: null result or non-positive size (num_levels=%d batch=%d num_heads=%d)", num_levels, batch,
                     num_heads);
    const GridChoice c = region_grid_choice(kernel, grid_geom(kernel, num_levels), host_spatial_shapes, num_levels, batch, num_heads, num_cus,
                                            kernel == 0 && num_levels == 4 && SEMIDETR_RW_TAIL);
    const int64_t wgs = (int64_t)batch * c.regions * num_heads;
    SEMIDETR_REQUIRE(wgs + num_cus < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_region_grid_query: grid too large");
    grid6[0] = c.nry;
    grid6[1] = c.nrx;
    grid6[2] = c.regions;
    grid6[3] = (int)wgs;
    grid6[4] = c.regions && c.tail ? 1 : 0;
    grid6[5] = c.max_queries;
    return SEMIDETR_OK;
}

extern "C" int semidetr_msda_forward_policy_state_slot(int slot, int *policy, int *mode, float *far_fraction, unsigned *updates)
{
    SEMIDETR_REQUIRE(slot >= 0 && slot < kPolicySlots, SEMIDETR_E_BADARG, "msda_forward_policy_state: slot must be 0..%d", kPolicySlots - 1);
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return semidetr::fail((int)e, "msda_forward_policy_state: %s", hipGetErrorString(e));
    std::lock_guard<std::mutex> lock(g_adapt_mu);
    const FwdAdapt *a = g_adapt[dev >= 0 && dev < kMaxDevices ? dev : 0];
    const FwdSlot none;
    const FwdSlot &sl = a ? a->slot[slot] : none;
    if (policy) *policy = g_fwd_policy.load(std::memory_order_relaxed);
    if (mode) *mode = sl.mode;
    if (far_fraction) *far_fraction = sl.last_frac;
    if (updates) *updates = sl.updates;
    return SEMIDETR_OK;
}

extern "C" int semidetr_msda_gather_choice(int slot)
{
    return (slot >= 0 && slot < kPolicySlots && slot_samples_are_near(slot)) ? SEMIDETR_MSDA_GATHER_WINDOW : SEMIDETR_MSDA_GATHER_PATCH;
}

extern "C" int semidetr_msda_forward_policy_state(int *policy, int *mode, float *far_fraction, unsigned *updates)
{
    return semidetr_msda_forward_policy_state_slot(0, policy, mode, far_fraction, updates);
}

#if SEMIDETR_EXPERIMENTS
// tuning aid: per-phase cycle counters of the instrumented kernels; reset = 1 zeroes them
extern "C" int semidetr_debug_counters(unsigned long long *out16, int reset)
{
    hipError_t e = hipSuccess;
    if (out16) e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_dest_dbg), sizeof(unsigned long long) * 16);
    if (e == hipSuccess && reset) {
        const unsigned long long z[16] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_dest_dbg), z, sizeof(z));
    }
    return e == hipSuccess ? SEMIDETR_OK : semidetr::fail((int)e, "debug_counters: %s", hipGetErrorString(e));
}

extern "C" void semidetr_msda_set_variant(int fwd_variant, int bwd_variant)
{
    g_fwd_variant_a.store(fwd_variant, std::memory_order_relaxed);
    g_bwd_variant_a.store(bwd_variant, std::memory_order_relaxed);
}
#define SEMIDETR_FWD_VARIANT (g_fwd_variant_a.load(std::memory_order_relaxed))
#define SEMIDETR_BWD_VARIANT (g_bwd_variant_a.load(std::memory_order_relaxed))
#else
#define SEMIDETR_FWD_VARIANT 0
#define SEMIDETR_BWD_VARIANT 0
#endif

// fast path of the f32 entry points: the product dispatch, or (experiments library, a variant forced) the tuning dispatch
template <typename IO>
static int dispatch_fast_forward(hipStream_t st, const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                 const IO &io, int N, int S, int M, int L, int Lq, int P, int flags, float *out,
                                 const int64_t *host_shapes)
{
#if SEMIDETR_EXPERIMENTS
    if (SEMIDETR_FWD_VARIANT != 0) return exp_launch_fast_forward(st, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, flags, out);
#endif
    return launch_fast_forward(st, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, flags, out, host_shapes);
}
template <typename IO>
static int dispatch_fast_backward(hipStream_t st, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start, const IO &io, int N, int S, int M, int L, int Lq, int P, int flags,
                                  float *grad_value, const int64_t *host_shapes)
{
#if SEMIDETR_EXPERIMENTS
    if (SEMIDETR_BWD_VARIANT != 0)
        return exp_launch_fast_backward(st, grad_out, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, flags, grad_value);
#endif
    return launch_fast_backward(st, grad_out, value, spatial_shapes, level_start, io, N, S, M, L, Lq, P, flags, grad_value, host_shapes);
}

extern "C" int semidetr_msda_forward_f32_v2(void *stream, const float *value, const int64_t *spatial_shapes,
                                            const int64_t *level_start, const float *sampling_loc,
                                            const float *attn_weight, int batch, int spatial_size,
                                            int num_heads, int channels, int num_levels, int num_query,
                                            int num_point, int flags, float *out, const int64_t *host_spatial_shapes)
{
    const int N = batch, S = spatial_size, M = num_heads, D = channels, L = num_levels, Lq = num_query,
              P = num_point;
    if (SEMIDETR_FWD_VARIANT == 99 || !fast_ok(value, sampling_loc, out, D, L, P) || !slice_ok(S, M) || !heads_ok(M))
        return forward_impl<float>(stream, value, spatial_shapes, level_start, sampling_loc, attn_weight, N,
                                   S, M, D, L, Lq, P, out);
    if (int rc = check_common(value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L,
                              Lq, P, 4))
        return rc;
    SEMIDETR_REQUIRE(out, SEMIDETR_E_BADARG, "msda_forward: null output");
    const LocAttnIO io = {sampling_loc, attn_weight, nullptr, nullptr};
    return dispatch_fast_forward(semidetr::as_stream(stream), value, spatial_shapes, level_start, io, N, S, M, L, Lq,
                                 P, flags, out, host_spatial_shapes);
}

extern "C" int semidetr_msda_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                         const int64_t *level_start, const float *sampling_loc,
                                         const float *attn_weight, int batch, int spatial_size,
                                         int num_heads, int channels, int num_levels, int num_query,
                                         int num_point, int flags, float *out)
{
    return semidetr_msda_forward_f32_v2(stream, value, spatial_shapes, level_start, sampling_loc, attn_weight, batch, spatial_size,
                                        num_heads, channels, num_levels, num_query, num_point, flags, out, nullptr);
}

extern "C" int semidetr_msda_backward_f32_v2(void *stream, const float *grad_out, const float *value,
                                             const int64_t *spatial_shapes, const int64_t *level_start,
                                             const float *sampling_loc, const float *attn_weight, int batch,
                                             int spatial_size, int num_heads, int channels, int num_levels,
                                             int num_query, int num_point, int flags, float *grad_value,
                                             float *grad_sampling_loc, float *grad_attn_weight, const int64_t *host_spatial_shapes)
{
    const int N = batch, S = spatial_size, M = num_heads, D = channels, L = num_levels, Lq = num_query,
              P = num_point;
    if (SEMIDETR_BWD_VARIANT == 99 || !fast_ok(value, sampling_loc, grad_out, D, L, P) || !slice_ok(S, M) || !heads_ok(M) ||
        !fast_ok(grad_value, grad_sampling_loc, grad_attn_weight, D, L, P))
        return backward_impl<float>(stream, grad_out, value, spatial_shapes, level_start, sampling_loc,
                                    attn_weight, N, S, M, D, L, Lq, P, grad_value, grad_sampling_loc,
                                    grad_attn_weight);
    if (int rc = check_common(value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L,
                              Lq, P, 4))
        return rc;
    SEMIDETR_REQUIRE(grad_out && grad_value && grad_sampling_loc && grad_attn_weight, SEMIDETR_E_BADARG,
                     "msda_backward: null pointer argument");
    const LocAttnIO io = {sampling_loc, attn_weight, grad_sampling_loc, grad_attn_weight};
    return dispatch_fast_backward(semidetr::as_stream(stream), grad_out, value, spatial_shapes, level_start, io, N, S,
                                  M, L, Lq, P, flags, grad_value, host_spatial_shapes);
}

extern "C" int semidetr_msda_backward_f32(void *stream, const float *grad_out, const float *value,
                                          const int64_t *spatial_shapes, const int64_t *level_start,
                                          const float *sampling_loc, const float *attn_weight, int batch,
                                          int spatial_size, int num_heads, int channels, int num_levels,
                                          int num_query, int num_point, int flags, float *grad_value,
                                          float *grad_sampling_loc, float *grad_attn_weight)
{
    return semidetr_msda_backward_f32_v2(stream, grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                         spatial_size, num_heads, channels, num_levels, num_query, num_point, flags, grad_value,
                                         grad_sampling_loc, grad_attn_weight, nullptr);
}

// ---- exact backward (opt-in): grad_value as the exact sum of its contributions, rounded once (msda_exact.h) ------------
// entries per (image, head) = num_query * num_levels * num_point * 4, or 0 when that is not below 2^32
static uint64_t exact_slice_entries(int L, int Lq, int P)
{
    uint64_t e = (uint64_t)Lq * (uint64_t)L;
    if (e >= (1ull << 32)) return 0;
    e *= (uint64_t)P;
    if (e >= (1ull << 30)) return 0;
    return e * 4;
}

extern "C" size_t semidetr_msda_exact_workspace_bytes(int batch, int spatial_size, int num_heads, int num_levels, int num_query,
                                                      int num_point)
{
    if (batch <= 0 || spatial_size <= 0 || num_heads <= 0 || num_levels <= 0 || num_query <= 0 || num_point <= 0) return 0;
    if (!exact_slice_entries(num_levels, num_query, num_point)) return 0;
    return semidetr_exact::workspace_layout(batch, spatial_size, num_heads, num_levels, num_query, num_point).total_bytes;
}

extern "C" int semidetr_msda_backward_exact_f32(void *stream, const float *grad_out, const float *value, const int64_t *spatial_shapes,
                                                const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                                                int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                                int num_query, int num_point, int flags, void *workspace, size_t workspace_bytes,
                                                float *grad_value, float *grad_sampling_loc, float *grad_attn_weight)
{
    namespace ex = semidetr_exact;
    const int N = batch, S = spatial_size, M = num_heads, D = channels, L = num_levels, Lq = num_query, P = num_point;
    if (int rc = check_common(value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L, Lq, P, 4)) return rc;
    SEMIDETR_REQUIRE(grad_out && grad_value && grad_sampling_loc && grad_attn_weight && workspace, SEMIDETR_E_BADARG,
                     "msda_backward_exact: null pointer argument");
    SEMIDETR_REQUIRE(D == kD, SEMIDETR_E_BADARG, "msda_backward_exact: channels must be 32 (got %d)", D);
    // (the small gradients come from the strips / patch gather: 32 rows of L * P + 1 records and the level table in 64 KB of LDS)
    const size_t glds = (size_t)32 * ((size_t)L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float);
    SEMIDETR_REQUIRE(L <= kMaxLevels && (int64_t)L * P <= 256 && glds <= 64 * 1024, SEMIDETR_E_BADARG,
                     "msda_backward_exact: num_levels * num_point = %lld does not fit the gather kernel's LDS (at most 62, <= %d levels)",
                     (long long)L * P, kMaxLevels);
    SEMIDETR_REQUIRE(heads_ok(M) && slice_ok(S, M), SEMIDETR_E_BADARG, "msda_backward_exact: <= 32 heads, image slice < 4 GB");
    SEMIDETR_REQUIRE(fast_ok(value, sampling_loc, grad_out, D, L, P) && fast_ok(grad_value, grad_sampling_loc, grad_attn_weight, D, L, P) &&
                         (reinterpret_cast<uintptr_t>(attn_weight) & 15) == 0,
                     SEMIDETR_E_BADARG, "msda_backward_exact: pointers must be 16-byte aligned");
    const uint64_t slice = exact_slice_entries(L, Lq, P);
    SEMIDETR_REQUIRE(slice != 0, SEMIDETR_E_BADARG,
                     "msda_backward_exact: num_query * num_levels * num_point * 4 must be below 2^32 (num_query=%d num_levels=%d num_point=%d)",
                     Lq, L, P);
    const ex::Workspace ws = ex::workspace_layout(N, S, M, L, Lq, P);
    SEMIDETR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, SEMIDETR_E_BADARG,
                     "msda_backward_exact: workspace must be 16-byte aligned");
    SEMIDETR_REQUIRE(workspace_bytes >= ws.total_bytes, SEMIDETR_E_BADARG,
                     "msda_backward_exact: workspace too small (%zu bytes, semidetr_msda_exact_workspace_bytes says %zu)", workspace_bytes,
                     ws.total_bytes);
    const bool pixels = (flags & SEMIDETR_MSDA_QUERIES_ARE_PIXELS) != 0;
    SEMIDETR_REQUIRE(!pixels || Lq == S, SEMIDETR_E_BADARG,
                     "msda_backward_exact: SEMIDETR_MSDA_QUERIES_ARE_PIXELS needs num_query == spatial_size");
    const int64_t samples = (int64_t)N * Lq * M * L * P, sample_blocks = (samples + 255) / 256;
    const int tiles = (S + ex::kReduceGroups - 1) / ex::kReduceGroups;
    const int gbound = patch_grid_hint(S, L, 32), gt = (Lq + 31) / 32;
    SEMIDETR_REQUIRE(sample_blocks < INT32_MAX && (int64_t)N * M * tiles < INT32_MAX && (int64_t)N * std::max(gbound, gt) * M < INT32_MAX,
                     SEMIDETR_E_TOOLARGE, "msda_backward_exact: grid too large");
    hipStream_t st = semidetr::as_stream(stream);
    // grad_sampling_loc / grad_attn_weight: the gather of the default route (no atomics, bitwise reproducible), zero = nullptr:
    // the patch instantiations for encoder self-attention as launch_encoder_backward takes them, else the strips one
    const LocAttnIO io = {sampling_loc, attn_weight, grad_sampling_loc, grad_attn_weight};
    const bool patch = pixels && P == kPT && (L * P == 16 || L * P == 20);
    if (patch && L * P == 16)
        hipLaunchKernelGGL((msda_bwd_gather_d32<LocAttnIO, 16, patch_hw(4, 8), SEMIDETR_GATHER_WPE, SEMIDETR_GATHER_KB>),
                           dim3((unsigned)((int64_t)N * gbound * M)), dim3(256), glds, st, grad_out, value, spatial_shapes, level_start, io, S, M,
                           L, Lq, P, gbound, (float4 *)nullptr, (int64_t)0);
    else if (patch)
        hipLaunchKernelGGL((msda_bwd_gather_d32<LocAttnIO, 20, patch_hw(4, 8), SEMIDETR_GATHER5_WPE, SEMIDETR_GATHER5_KB>),
                           dim3((unsigned)((int64_t)N * gbound * M)), dim3(256), glds, st, grad_out, value, spatial_shapes, level_start, io, S, M,
                           L, Lq, P, gbound, (float4 *)nullptr, (int64_t)0);
    else
        hipLaunchKernelGGL((msda_bwd_gather_d32<LocAttnIO, 0>), dim3((unsigned)((int64_t)N * gt * M)), dim3(256), glds, st, grad_out, value,
                           spatial_shapes, level_start, io, S, M, L, Lq, P, gt);
    if (int rc = semidetr::launch_status("msda_bwd_gather_d32")) return rc;
    unsigned *count = static_cast<unsigned *>(workspace);
    unsigned *start = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + ws.counts_bytes);
    ex::Entry *entries = reinterpret_cast<ex::Entry *>(static_cast<char *>(workspace) + 2 * ws.counts_bytes);
    const int64_t n16 = (int64_t)(ws.counts_bytes / 16);
    hipLaunchKernelGGL(ex::exact_clear, dim3((unsigned)std::min<int64_t>((n16 + 255) / 256, 2048)), dim3(256), 0, st,
                       reinterpret_cast<uint4 *>(count), n16);
    hipLaunchKernelGGL(ex::exact_count, dim3((unsigned)sample_blocks), dim3(256), 0, st, spatial_shapes, level_start, sampling_loc, S, M, L,
                       Lq, P, samples, count);
    hipLaunchKernelGGL(ex::exact_scan, dim3((unsigned)(N * M)), dim3(ex::kScanThreads), 0, st, count, start, S);
    hipLaunchKernelGGL(ex::exact_fill, dim3((unsigned)sample_blocks), dim3(256), 0, st, spatial_shapes, level_start, sampling_loc,
                       attn_weight, S, M, L, Lq, P, samples, start, count, entries, (unsigned)slice);
    hipLaunchKernelGGL(ex::exact_reduce, dim3((unsigned)((int64_t)N * M * tiles)), dim3(ex::kReduceThreads), 0, st, grad_out, start, count,
                       entries, (unsigned)slice, S, M, tiles, grad_value);
    g_last_kernels = ex::kLaunchedKernels;
    return semidetr::launch_status("msda_backward_exact");
}

// ---- fused MSDeformAttn prologue / epilogue (fp32, channels == 32) --------------------------------------
static int check_fused(const void *value, const void *shapes, const void *starts, const void *ref, int ref_dim,
                       const void *off, const void *logit, int N, int S, int M, int D, int L, int Lq, int P)
{
    if (int rc = check_common(value, shapes, starts, off, logit, N, S, M, D, L, Lq, P, 4)) return rc;
    SEMIDETR_REQUIRE(ref, SEMIDETR_E_BADARG, "msda_fused: null reference_points");
    SEMIDETR_REQUIRE(ref_dim == 2 || ref_dim == 4, SEMIDETR_E_BADARG,
                     "Last dim of reference_points must be 2 or 4, but get %d instead.", ref_dim);
    SEMIDETR_REQUIRE(D == kD && L <= kMaxLevels && (int64_t)L * P <= 256 && slice_ok(S, M) && heads_ok(M), SEMIDETR_E_BADARG,
                     "msda_fused: only channels == 32 (got %d), <= %d levels, L*P <= 256, <= 32 heads, image slice < 4 GB", D, kMaxLevels);
    SEMIDETR_REQUIRE((((uintptr_t)value | (uintptr_t)off | (uintptr_t)ref) & 15) == 0, SEMIDETR_E_BADARG,
                     "msda_fused: value / sampling_offsets / reference_points must be 16-byte aligned");
    SEMIDETR_REQUIRE((int64_t)N * Lq * L * ref_dim * 4 < (int64_t)0xFFFFFFF0u, SEMIDETR_E_TOOLARGE,
                     "msda_fused: reference_points must be smaller than 4 GB");
    return SEMIDETR_OK;
}

extern "C" int semidetr_msda_fused_forward_f32_v2(void *stream, const float *value, const int64_t *spatial_shapes,
                                                  const int64_t *level_start, const float *reference_points,
                                                  int ref_dim, const float *sampling_offsets,
                                                  const float *attn_logits, const unsigned char *padding_mask,
                                                  const int *mask_extents, int batch,
                                                  int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                                  int num_point, int flags, float *out, const int64_t *host_spatial_shapes)
{
    if (int rc = check_fused(value, spatial_shapes, level_start, reference_points, ref_dim, sampling_offsets,
                             attn_logits, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point))
        return rc;
    SEMIDETR_REQUIRE(out && ((uintptr_t)out & 15) == 0, SEMIDETR_E_BADARG, "msda_fused_forward: bad output pointer");
    const unsigned ref_bytes = (unsigned)((int64_t)batch * num_query * num_levels * ref_dim * 4);
    const RawIO io = {reference_points, sampling_offsets, attn_logits, nullptr, nullptr, ref_dim, num_heads,
                      num_levels, padding_mask, spatial_size, ref_bytes, padding_mask ? mask_extents : nullptr};
    SEMIDETR_REQUIRE(!padding_mask || SEMIDETR_FWD_VARIANT == 0, SEMIDETR_E_BADARG,
                     "msda_fused_forward: the experimental kernel variants do not take a padding mask");
    return dispatch_fast_forward(semidetr::as_stream(stream), value, spatial_shapes, level_start, io, batch,
                                 spatial_size, num_heads, num_levels, num_query, num_point, flags, out, host_spatial_shapes);
}

extern "C" int semidetr_msda_fused_forward_f32(void *stream, const float *value, const int64_t *spatial_shapes,
                                               const int64_t *level_start, const float *reference_points,
                                               int ref_dim, const float *sampling_offsets,
                                               const float *attn_logits, const unsigned char *padding_mask,
                                               const int *mask_extents, int batch,
                                               int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                               int num_point, int flags, float *out)
{
    return semidetr_msda_fused_forward_f32_v2(stream, value, spatial_shapes, level_start, reference_points, ref_dim, sampling_offsets,
                                              attn_logits, padding_mask, mask_extents, batch, spatial_size, num_heads, channels,
                                              num_levels, num_query, num_point, flags, out, nullptr);
}

extern "C" int semidetr_msda_fused_backward_f32_v2(void *stream, const float *grad_out, const float *value,
                                                   const int64_t *spatial_shapes, const int64_t *level_start,
                                                   const float *reference_points, int ref_dim,
                                                   const float *sampling_offsets, const float *attn_logits,
                                                   const unsigned char *padding_mask, const int *mask_extents, int batch,
                                                   int spatial_size, int num_heads, int channels, int num_levels,
                                                   int num_query, int num_point, int flags, float *grad_value,
                                                   float *grad_sampling_offsets, float *grad_attn_logits,
                                                   const int64_t *host_spatial_shapes)
{
    if (int rc = check_fused(value, spatial_shapes, level_start, reference_points, ref_dim, sampling_offsets,
                             attn_logits, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point))
        return rc;
    SEMIDETR_REQUIRE(grad_out && grad_value && grad_sampling_offsets && grad_attn_logits, SEMIDETR_E_BADARG,
                     "msda_fused_backward: null pointer argument");
    SEMIDETR_REQUIRE((((uintptr_t)grad_out | (uintptr_t)grad_value | (uintptr_t)grad_sampling_offsets) & 15) == 0,
                     SEMIDETR_E_BADARG, "msda_fused_backward: pointers must be 16-byte aligned");
    const unsigned ref_bytes = (unsigned)((int64_t)batch * num_query * num_levels * ref_dim * 4);
    const RawIO io = {reference_points, sampling_offsets, attn_logits, grad_sampling_offsets, grad_attn_logits,
                      ref_dim, num_heads, num_levels, padding_mask, spatial_size, ref_bytes, padding_mask ? mask_extents : nullptr};
    SEMIDETR_REQUIRE(!padding_mask || SEMIDETR_BWD_VARIANT == 0, SEMIDETR_E_BADARG,
                     "msda_fused_backward: the experimental kernel variants do not take a padding mask");
    return dispatch_fast_backward(semidetr::as_stream(stream), grad_out, value, spatial_shapes, level_start, io, batch,
                                  spatial_size, num_heads, num_levels, num_query, num_point, flags, grad_value, host_spatial_shapes);
}

extern "C" int semidetr_msda_fused_backward_f32(void *stream, const float *grad_out, const float *value,
                                                const int64_t *spatial_shapes, const int64_t *level_start,
                                                const float *reference_points, int ref_dim,
                                                const float *sampling_offsets, const float *attn_logits,
                                                const unsigned char *padding_mask, const int *mask_extents, int batch,
                                                int spatial_size, int num_heads, int channels, int num_levels,
                                                int num_query, int num_point, int flags, float *grad_value,
                                                float *grad_sampling_offsets, float *grad_attn_logits)
{
    return semidetr_msda_fused_backward_f32_v2(stream, grad_out, value, spatial_shapes, level_start, reference_points, ref_dim,
                                               sampling_offsets, attn_logits, padding_mask, mask_extents, batch, spatial_size, num_heads,
                                               channels, num_levels, num_query, num_point, flags, grad_value, grad_sampling_offsets,
                                               grad_attn_logits, nullptr);
}

// ---- padding mask -> one word per (image, level): vh | vw << 16 or -1 (MaskExt, msda_fast.h).  One workgroup per (image, level): the first
//      padded pixel of row 0 / column 0 gives the candidate (vw, vh); every pixel is then checked against "padding iff y >= vh or
//      x >= vw" -- exactly what F.interpolate of an image-sized padding band produces (dense_heads/dino_detr_head.py:305-318).
// Round 6: 1024 threads, 16 mask bytes per thread and trip (one division per trip instead of one per pixel; the level's 16.7 k bytes of the
// 100 x 167 level are ONE trip): 24 -> ~4 us per launch.  It runs once per mask tensor -- in training: per batch, i.e. a few times per step.
__global__ __launch_bounds__(1024) void msda_mask_extents_kernel(const unsigned char *__restrict__ mask, const int64_t *__restrict__ shapes,
                                                                 const int64_t *__restrict__ starts, int S, int L, int *__restrict__ ext)
{
    const int n = (int)blockIdx.x / L, l = (int)blockIdx.x % L;
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
    const unsigned char *mk = mask + (int64_t)n * S + st;
    __shared__ int s_vh, s_vw, s_bad;
    if (threadIdx.x == 0) { s_vh = H; s_vw = W; s_bad = 0; }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 1024)
        if (mk[x]) atomicMin(&s_vw, x);
    for (int y = threadIdx.x; y < H; y += 1024)
        if (mk[(int64_t)y * W]) atomicMin(&s_vh, y);
    __syncthreads();
    int vh = s_vh, vw = s_vw;
    if (vh == 0 || vw == 0) vh = vw = 0;      // pixel (0, 0) is padding: only "everything is" has the form
    bool bad = false;
    const int HW = H * W;
    // 16 consecutive pixels per thread: aligned 16-byte loads where the level's first byte allows it (it need not be aligned: st is any sum of H*W)
    const int head = (int)((16 - ((uintptr_t)mk & 15)) & 15);       // bytes before the first aligned 16
    for (int i = threadIdx.x; i < min(head, HW); i += 1024) {
        const int y = i / W, x = i - y * W;
        bad = bad || ((mk[i] != 0) != (y >= vh || x >= vw));
    }
    for (int i0 = head + 16 * (int)threadIdx.x; i0 < HW; i0 += 16 * 1024) {
        int y = i0 / W, x = i0 - y * W;
        if (i0 + 16 <= HW) {
            const uint4 q = *reinterpret_cast<const uint4 *>(mk + i0);
            const unsigned w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const bool m = ((w4[b >> 2] >> (8 * (b & 3))) & 0xffu) != 0;
                bad = bad || (m != (y >= vh || x >= vw));
                if (++x == W) { x = 0; ++y; }
            }
        } else {
            for (int i = i0; i < HW; ++i) {
                bad = bad || ((mk[i] != 0) != (y >= vh || x >= vw));
                if (++x == W) { x = 0; ++y; }
            }
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) ext[blockIdx.x] = (s_bad || H > 0x7fff || W > 0x7fff) ? -1 : (vh | (vw << 16));
}

extern "C" int semidetr_msda_mask_extents(void *stream, const unsigned char *padding_mask, const int64_t *spatial_shapes,
                                          const int64_t *level_start, int batch, int spatial_size, int num_levels, int *extents)
{
    SEMIDETR_REQUIRE(padding_mask && spatial_shapes && level_start && extents, SEMIDETR_E_BADARG, "msda_mask_extents: null pointer argument");
    SEMIDETR_REQUIRE(batch > 0 && spatial_size > 0 && num_levels > 0 && num_levels <= kMaxLevels && (int64_t)batch * num_levels < INT32_MAX,
                     SEMIDETR_E_BADARG, "msda_mask_extents: sizes must be positive (batch=%d spatial_size=%d num_levels=%d)", batch,
                     spatial_size, num_levels);
    hipLaunchKernelGGL(msda_mask_extents_kernel, dim3((unsigned)(batch * num_levels)), dim3(1024), 0, semidetr::as_stream(stream),
                       padding_mask, spatial_shapes, level_start, spatial_size, num_levels, extents);
    return semidetr::launch_status("msda_mask_extents");
}

extern "C" int semidetr_msda_forward_f64(void *stream, const double *value, const int64_t *spatial_shapes,
                                         const int64_t *level_start, const double *sampling_loc,
                                         const double *attn_weight, int batch, int spatial_size,
                                         int num_heads, int channels, int num_levels, int num_query,
                                         int num_point, double *out)
{
    return forward_impl<double>(stream, value, spatial_shapes, level_start, sampling_loc, attn_weight, batch,
                                spatial_size, num_heads, channels, num_levels, num_query, num_point, out);
}

extern "C" int semidetr_msda_backward_f64(void *stream, const double *grad_out, const double *value,
                                          const int64_t *spatial_shapes, const int64_t *level_start,
                                          const double *sampling_loc, const double *attn_weight, int batch,
                                          int spatial_size, int num_heads, int channels, int num_levels,
                                          int num_query, int num_point, double *grad_value,
                                          double *grad_sampling_loc, double *grad_attn_weight)
{
    return backward_impl<double>(stream, grad_out, value, spatial_shapes, level_start, sampling_loc,
                                 attn_weight, batch, spatial_size, num_heads, channels, num_levels, num_query,
                                 num_point, grad_value, grad_sampling_loc, grad_attn_weight);
}

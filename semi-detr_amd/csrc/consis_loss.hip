// Cross-view query consistency loss of Semi-DETR for gfx950 (DinoDetrSSOD.unsup_loss, detr_ssod/models/dino_detr_ssod.py:463-481),
// every decoder layer in one launch:
//   loss_l = scale * mean_{k, d} ( w_k * (normalize(hs_v1[l][bid_k, idx_k])_d - normalize(hs_v2[l][bid_k, idx_k])_d)^2 )
// with normalize(x) = x / max(||x||_2, eps) (F.normalize) and hs_v2 detached.
//
//   consis_fwd_kernel       one wave per work item (l, k), four per workgroup: the two rows straight from the callers' tensors
//                           (per layer and view a base pointer, a batch stride and a query stride), ||x1||^2 and ||x2||^2 by a
//                           wave tree, then sum_d (y1 - y2)^2 times w_k; the workgroup's rows in fp64 -> one partial slot
//   consis_finalize_kernel  ONE workgroup: per layer the slots in index order (lanes stride them, then a shuffle tree, fp64)
//                           -> loss_l = (float)(sum_l * (double)(scale / (K * D))); and the inverse map (b, q) -> k or -1 over
//                           the pad that the backward reads
//   consis_bwd_kernel       one wave per row (l, b, q) of the dense gradient of hs_v1[l]: a selected row is recomputed from the
//                           two rows and gets its gradient, every other row is written as zeros (no memset, no atomics)
// No float atomics: every sum is taken in a fixed order, so a launch sequence is bitwise reproducible.  The (bid, idx) pairs are
// distinct by construction (idx = i + single_pad * g); that is the contract, and with it the inverse map has one writer per slot.
//
// Arithmetic (tests/consis_ref64.py states it in float64 with error bounds; IEEE divide and sqrtf, no rsq / rcp, no fma):
//   row sum of t_0 .. t_{D-1}:  lane j takes the float4 chunks j, j + 64, ... in that order, acc += (t0 + t1) + (t2 + t3) from
//     acc = 0 (D = 256: one chunk, the row stays in registers), then the xor tree over 32, 16, 8, 4, 2, 1 lanes
//   n = sqrtf(row sum of x^2), y = x / fmaxf(n, eps), e = y1 - y2, term_k = (row sum of e^2) * w_k
//   backward: coef_l = inv * upstream_l (inv = scale / (K * D) in fp32), c = w_k * coef_l, g = (2 c) * e
//     n1 >= eps:  grad = g / n1 - x1 * (((dot / n1) / n1) / n1), dot = row sum of x1 * g
//     n1 <  eps:  grad = g / eps                     (clamp_min's gate, >= passes; a zero row has no norm gradient)
// A pair with bid outside [0, B) or idx outside [0, pad_size) is not dereferenced: its workgroup's partial is NaN, so the loss of
// every layer is NaN (the reference raises a device-side index error there), and it gets no slot in the inverse map.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxL = SEMIDETR_CONSIS_MAX_LAYERS;
constexpr int kBwdRows = 16;                 // rows of the dense gradient per workgroup (four per wave)

struct Launch {
    semidetr_consis_loss p;
    int blocks_per_layer;      // ceil(K / kWaves)
    float inv;                 // scale / (K * D)
};

__device__ __forceinline__ float wave_sum(float v)
{
    #pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
    #pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__device__ __forceinline__ float4 ld4(const float *row, int chunk)
{
    return *reinterpret_cast<const float4 *>(row + 4 * chunk);
}

__device__ __forceinline__ float sum4(float a, float b, float c, float d) { return (a + b) + (c + d); }

// (bid, idx) of pair k, or false when it must not be dereferenced
__device__ __forceinline__ bool pair_of(const semidetr_consis_loss &p, int k, int &b, int &q)
{
    int64_t bb;
    if (p.bid_is_int64) {
        bb = static_cast<const int64_t *>(p.known_bid)[k];
    } else {
        const float f = static_cast<const float *>(p.known_bid)[k];
        if (!(f >= 0.f && f < (float)p.batch)) return false;       // NaN fails here too
        bb = (int64_t)f;
    }
    const int64_t qq = p.map_known_indice[k];
    if (bb < 0 || bb >= p.batch || qq < 0 || qq >= p.pad_size) return false;
    b = (int)bb;
    q = (int)qq;
    return true;
}

// One row of each view, D == 256 (FIXED: one float4 per lane, held in registers) or any D % 4 == 0 (re-read per pass).
template <bool FIXED>
struct Rows {
    const float *r1, *r2;
    int chunks, lane;
    float4 a, b;
    __device__ __forceinline__ Rows(const float *r1_, const float *r2_, int D, int lane_)
        : r1(r1_), r2(r2_), chunks(D >> 2), lane(lane_)
    {
        if (FIXED) { a = ld4(r1, lane); b = ld4(r2, lane); }
    }
    // row sum of f(x1 chunk, x2 chunk) in the order of the header
    template <typename F>
    __device__ __forceinline__ float sum(F f) const
    {
        float acc = 0.f;
        if (FIXED) {
            acc += f(a, b);
        } else {
            for (int c = lane; c < chunks; c += 64) acc += f(ld4(r1, c), ld4(r2, c));
        }
        return wave_sum(acc);
    }
    template <typename F>
    __device__ __forceinline__ void each(F f) const
    {
        if (FIXED) {
            f(lane, a, b);
        } else {
            for (int c = lane; c < chunks; c += 64) f(c, ld4(r1, c), ld4(r2, c));
        }
    }
};

struct Norms { float n1, d1, d2; };

template <bool FIXED>
__device__ __forceinline__ Norms norms_of(const Rows<FIXED> &r, float eps)
{
    const float s1 = r.sum([](float4 x, float4) { return sum4(x.x * x.x, x.y * x.y, x.z * x.z, x.w * x.w); });
    const float s2 = r.sum([](float4, float4 x) { return sum4(x.x * x.x, x.y * x.y, x.z * x.z, x.w * x.w); });
    Norms n;
    n.n1 = sqrtf(s1);
    n.d1 = fmaxf(n.n1, eps);
    n.d2 = fmaxf(sqrtf(s2), eps);
    return n;
}

__device__ __forceinline__ float4 diff_of(float4 x1, float4 x2, float d1, float d2)
{
    return make_float4(x1.x / d1 - x2.x / d2, x1.y / d1 - x2.y / d2, x1.z / d1 - x2.z / d2, x1.w / d1 - x2.w / d2);
}

template <bool FIXED>
__global__ __launch_bounds__(kThreads) void consis_fwd_kernel(const Launch L, double *__restrict__ partial)
{
    __shared__ double red[kWaves];
    const semidetr_consis_loss &p = L.p;
    const int layer = blockIdx.x / L.blocks_per_layer, blk = blockIdx.x - layer * L.blocks_per_layer;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blk * kWaves + wv;
    double term = 0.0;
    if (k < p.num_known) {
        int b, q;
        if (pair_of(p, k, b, q)) {
            const semidetr_consis_layer &ly = p.layer[layer];
            const Rows<FIXED> r(ly.v1 + b * ly.v1_stride[0] + q * ly.v1_stride[1],
                                ly.v2 + b * ly.v2_stride[0] + q * ly.v2_stride[1], p.dim, lane);
            const Norms n = norms_of(r, p.eps);
            const float d1 = n.d1, d2 = n.d2;
            const float s = r.sum([d1, d2](float4 x1, float4 x2) {
                const float4 e = diff_of(x1, x2, d1, d2);
                return sum4(e.x * e.x, e.y * e.y, e.z * e.z, e.w * e.w);
            });
            term = (double)(s * (p.loss_weights ? p.loss_weights[k] : 0.f));
        } else {
            term = __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    if (lane == 0) red[wv] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void consis_finalize_kernel(const Launch L, const double *__restrict__ partial,
                                                                   float *__restrict__ losses, int32_t *__restrict__ inverse)
{
    const semidetr_consis_loss &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int l = wv; l < p.num_layers; l += kWaves) {
        double acc = 0.0;
        for (int i = lane; i < L.blocks_per_layer; i += 64) acc += partial[l * L.blocks_per_layer + i];
        acc = wave_sum(acc);
        if (lane == 0) losses[l] = (float)(acc * (double)L.inv);
    }
    const int slots = p.batch * p.pad_size;
    for (int i = threadIdx.x; i < slots; i += kThreads) inverse[i] = -1;
    __syncthreads();
    for (int k = threadIdx.x; k < p.num_known; k += kThreads) {
        int b, q;
        if (pair_of(p, k, b, q)) inverse[b * p.pad_size + q] = k;
    }
}

template <bool FIXED>
__global__ __launch_bounds__(kThreads) void consis_bwd_kernel(const Launch L, const int32_t *__restrict__ inverse,
                                                              const float *__restrict__ grad_losses)
{
    const semidetr_consis_loss &p = L.p;
    const int rows = p.batch * p.num_query, blocks_per_layer = (rows + kBwdRows - 1) / kBwdRows;
    const int layer = blockIdx.x / blocks_per_layer, blk = blockIdx.x - layer * blocks_per_layer;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const semidetr_consis_layer &ly = p.layer[layer];
    const int D = p.dim, chunks = D >> 2;
    const float coef = L.inv * grad_losses[layer];
    for (int i = 0; i < kBwdRows / kWaves; ++i) {
        const int row = blk * kBwdRows + i * kWaves + wv;
        if (row >= rows) break;
        const int b = row / p.num_query, q = row - b * p.num_query;
        float *out = ly.grad_v1 + (int64_t)row * D;
        const int k = q < p.pad_size ? inverse[b * p.pad_size + q] : -1;
        if (k < 0) {
            for (int c = lane; c < chunks; c += 64) *reinterpret_cast<float4 *>(out + 4 * c) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const Rows<FIXED> r(ly.v1 + b * ly.v1_stride[0] + q * ly.v1_stride[1], ly.v2 + b * ly.v2_stride[0] + q * ly.v2_stride[1],
                            D, lane);
        const Norms n = norms_of(r, p.eps);
        const float d1 = n.d1, d2 = n.d2, n1 = n.n1, eps = p.eps;
        const float c2 = 2.f * ((p.loss_weights ? p.loss_weights[k] : 0.f) * coef);
        if (n1 >= eps) {
            const float dot = r.sum([d1, d2, c2](float4 x1, float4 x2) {
                const float4 e = diff_of(x1, x2, d1, d2);
                return sum4(x1.x * (c2 * e.x), x1.y * (c2 * e.y), x1.z * (c2 * e.z), x1.w * (c2 * e.w));
            });
            const float t = ((dot / n1) / n1) / n1;
            r.each([=](int c, float4 x1, float4 x2) {
                const float4 e = diff_of(x1, x2, d1, d2);
                *reinterpret_cast<float4 *>(out + 4 * c) =
                    make_float4((c2 * e.x) / n1 - x1.x * t, (c2 * e.y) / n1 - x1.y * t, (c2 * e.z) / n1 - x1.z * t,
                                (c2 * e.w) / n1 - x1.w * t);
            });
        } else {
            r.each([=](int c, float4 x1, float4 x2) {
                const float4 e = diff_of(x1, x2, d1, d2);
                *reinterpret_cast<float4 *>(out + 4 * c) =
                    make_float4((c2 * e.x) / eps, (c2 * e.y) / eps, (c2 * e.z) / eps, (c2 * e.w) / eps);
            });
        }
    }
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

// Host-side check of the parameter block + launch geometry.  Returns SEMIDETR_OK or an error (message set).
int plan(const semidetr_consis_loss *params, Launch &L, int for_backward)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "consis_loss: null pointer (parameter block)");
    const semidetr_consis_loss &p = params[0];
    SEMIDETR_REQUIRE(p.num_layers >= 1 && p.num_layers <= kMaxL, SEMIDETR_E_BADARG, "consis_loss: %d layers (1..%d)",
                     p.num_layers, kMaxL);
    SEMIDETR_REQUIRE(p.batch > 0 && p.num_query > 0 && p.dim > 0 && p.num_known > 0, SEMIDETR_E_BADARG,
                     "consis_loss: bad sizes (B=%d Q=%d D=%d K=%d)", p.batch, p.num_query, p.dim, p.num_known);
    SEMIDETR_REQUIRE(p.dim % 4 == 0, SEMIDETR_E_BADARG, "consis_loss: D = %d is not a multiple of 4", p.dim);
    SEMIDETR_REQUIRE(p.pad_size >= 0 && p.pad_size <= p.num_query, SEMIDETR_E_BADARG,
                     "consis_loss: pad_size %d outside [0, Q = %d]", p.pad_size, p.num_query);
    SEMIDETR_REQUIRE(p.known_bid && p.map_known_indice, SEMIDETR_E_BADARG,
                     "consis_loss: null pointer (known_bid / map_known_indice)");
    SEMIDETR_REQUIRE(p.eps > 0.f && p.scale == p.scale, SEMIDETR_E_BADARG, "consis_loss: eps <= 0 or scale NaN");
    SEMIDETR_REQUIRE((int64_t)p.batch * p.num_query < ((int64_t)1 << 27) && (int64_t)p.num_known < ((int64_t)1 << 24) &&
                         (int64_t)p.batch * p.num_query * p.dim < ((int64_t)1 << 40),
                     SEMIDETR_E_TOOLARGE, "consis_loss: too large (B * Q < 2^27, K < 2^24)");
    for (int l = 0; l < p.num_layers; ++l) {
        const semidetr_consis_layer &ly = p.layer[l];
        SEMIDETR_REQUIRE(ly.v1 && ly.v2, SEMIDETR_E_BADARG, "consis_loss: layer %d: null pointer (hs_v1 / hs_v2)", l);
        SEMIDETR_REQUIRE(aligned16(ly.v1) && aligned16(ly.v2) && ly.v1_stride[0] % 4 == 0 && ly.v1_stride[1] % 4 == 0 &&
                             ly.v2_stride[0] % 4 == 0 && ly.v2_stride[1] % 4 == 0,
                         SEMIDETR_E_BADARG, "consis_loss: layer %d: rows must be 16-byte aligned (base and strides)", l);
        SEMIDETR_REQUIRE(ly.v1_stride[0] >= 0 && ly.v1_stride[1] >= 0 && ly.v2_stride[0] >= 0 && ly.v2_stride[1] >= 0,
                         SEMIDETR_E_BADARG, "consis_loss: layer %d: negative stride", l);
        if (for_backward)
            SEMIDETR_REQUIRE(ly.grad_v1 && aligned16(ly.grad_v1), SEMIDETR_E_BADARG,
                             "consis_loss: layer %d: null pointer or misaligned grad_v1", l);
    }
    L.p = p;
    L.blocks_per_layer = (p.num_known + kWaves - 1) / kWaves;
    L.inv = p.scale / (float)((int64_t)p.num_known * p.dim);
    return SEMIDETR_OK;
}

size_t partial_bytes(int num_layers, int num_known)
{
    return (size_t)num_layers * (size_t)((num_known + kWaves - 1) / kWaves) * sizeof(double);
}

}  // namespace

extern "C" size_t semidetr_consis_loss_workspace_bytes(int num_layers, int num_known, int batch, int pad_size)
{
    if (num_layers < 1 || num_layers > kMaxL || num_known < 1 || batch < 1 || pad_size < 0) return 0;
    return partial_bytes(num_layers, num_known) + (size_t)batch * (size_t)pad_size * sizeof(int32_t);
}

extern "C" int semidetr_consis_loss_forward_f32(void *stream, const semidetr_consis_loss *params, void *workspace,
                                                size_t workspace_bytes, float *losses)
{
    Launch L;
    if (int rc = plan(params, L, 0)) return rc;
    const semidetr_consis_loss &p = L.p;
    SEMIDETR_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 &&
                         workspace_bytes >= semidetr_consis_loss_workspace_bytes(p.num_layers, p.num_known, p.batch, p.pad_size),
                     SEMIDETR_E_BADARG, "consis_loss: workspace null, misaligned or smaller than "
                     "semidetr_consis_loss_workspace_bytes()");
    SEMIDETR_REQUIRE(losses, SEMIDETR_E_BADARG, "consis_loss: null pointer (losses)");
    hipStream_t st = semidetr::as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    int32_t *inverse = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + partial_bytes(p.num_layers, p.num_known));
    const dim3 grid(p.num_layers * L.blocks_per_layer);
    if (p.dim == 256) hipLaunchKernelGGL(consis_fwd_kernel<true>, grid, dim3(kThreads), 0, st, L, partial);
    else hipLaunchKernelGGL(consis_fwd_kernel<false>, grid, dim3(kThreads), 0, st, L, partial);
    if (int rc = semidetr::launch_status("consis_fwd_kernel")) return rc;
    hipLaunchKernelGGL(consis_finalize_kernel, dim3(1), dim3(kThreads), 0, st, L, partial, losses, inverse);
    return semidetr::launch_status("consis_finalize_kernel");
}

extern "C" int semidetr_consis_loss_backward_f32(void *stream, const semidetr_consis_loss *params, const void *workspace,
                                                 size_t workspace_bytes, const float *grad_losses)
{
    Launch L;
    if (int rc = plan(params, L, 1)) return rc;
    const semidetr_consis_loss &p = L.p;
    SEMIDETR_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 &&
                         workspace_bytes >= semidetr_consis_loss_workspace_bytes(p.num_layers, p.num_known, p.batch, p.pad_size),
                     SEMIDETR_E_BADARG, "consis_loss backward: workspace null, misaligned or smaller than "
                     "semidetr_consis_loss_workspace_bytes()");
    SEMIDETR_REQUIRE(grad_losses, SEMIDETR_E_BADARG, "consis_loss backward: null pointer (grad_losses)");
    const int32_t *inverse =
        reinterpret_cast<const int32_t *>(static_cast<const char *>(workspace) + partial_bytes(p.num_layers, p.num_known));
    const int rows = p.batch * p.num_query;
    const dim3 grid(p.num_layers * ((rows + kBwdRows - 1) / kBwdRows));
    hipStream_t st = semidetr::as_stream(stream);
    if (p.dim == 256) hipLaunchKernelGGL(consis_bwd_kernel<true>, grid, dim3(kThreads), 0, st, L, inverse, grad_losses);
    else hipLaunchKernelGGL(consis_bwd_kernel<false>, grid, dim3(kThreads), 0, st, L, inverse, grad_losses);
    return semidetr::launch_status("consis_bwd_kernel");
}

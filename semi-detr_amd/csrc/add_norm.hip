// Residual add + LayerNorm + positional add for gfx950, row width 256 (the model's d_model), forward and backward: the epilogue
// of every transformer sub-block (detr_od/models/utils/transformer.py:628-629, 636-637, 789-790, 811-812, 838-839) and the
// with_pos_embed that opens the next one.  fp32 arithmetic; the *_f32 entry points are fp32 in and out, the *_mixed entry points
// read and write rows of fp32, fp16 or bf16 elements, each operand and each result in its own type.
//
//   add_norm_fwd_kernel          workgroup = 4 waves, wave = 4 rows in flight, lane = 4 columns (one 16-byte load per operand);
//                                no LDS, no barrier.  Reads x, residual, pos once; writes y, q = y + pos, mean, rstd.
//   add_norm_bwd_kernel<sums>    workgroup = 4 waves, wave = 16 consecutive rows in 4 batches of 4 rows in flight.  Reads x,
//                                residual, gy, gq, mean, rstd; writes dx once.  <true>: every lane also adds g * xhat and g of
//                                its four columns over its wave's rows in row order; the four waves combine through LDS in wave
//                                order into slot blockIdx.x of the workspace (512 floats: dweight | dbias).
//   add_norm_param_kernel        8 workgroups x 64 columns x 16 parts: part k adds slots [k * chunk, (k + 1) * chunk) in index
//                                order in fp64, the 16 parts are added in part order, one rounding to fp32.
//   add_norm_fwd_mixed_kernel, add_norm_bwd_mixed_kernel<sums>
//                                the same grids, row -> wave map, batches and slots; a 16-bit operand is one 8-byte load per lane,
//                                up-cast exactly; a 16-bit result is rounded once, to nearest even, from the unrounded fp32 value
//                                (q from the unrounded y + pos; fp16 overflows to inf).  The backward stores its one fp32 dx as
//                                grad_x and / or grad_residual, each in its type, and gq as grad_pos in pos's type.
// The grid, the row -> wave map, the slot count and the chunks are functions of `rows` alone: no float atomics, no memset, two
// runs are bitwise equal.
//
// Arithmetic per row, in this order (tests/add_norm_ref64.py bounds it; the compiler may contract a * b + c into an fma):
//   s = x + residual; mu = (sum_lanes ((s0 + s1) + (s2 + s3))) / 256 by a xor butterfly (every lane holds the same bits);
//   d = s - mu; var = (sum d^2) / 256 the same way; rstd = 1 / sqrt(var + eps); y = (d * rstd) * w + b; q = y + pos.
//   backward: g = gy + gq; xhat = (x + residual - mu) * rstd; gw = g * w; c1 = (sum gw) / 256; c2 = (sum gw * xhat) / 256;
//   dx = rstd * ((gw - c1) - xhat * c2).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"                   // Cvt<T16>, unpack4, pack2: shared with msda_h16.hip

constexpr int kDim = 256;                    // row width: 64 lanes x one float4
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kFlight = 4;                   // rows a wave has in flight
constexpr int kBwdBatches = 4;               // the backward's wave owns kBwdBatches * kFlight consecutive rows
constexpr int kBwdWaveRows = kBwdBatches * kFlight, kBwdGroupRows = kBwdWaveRows * kWaves;
constexpr int kSlot = 2 * kDim;              // floats of one partial slot: dweight | dbias
constexpr int kParts = 16;                   // chunks of slots added side by side by add_norm_param_kernel
constexpr float kInvDim = 1.0f / kDim;

__device__ __forceinline__ float wave_sum(float v)
{
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float sum4(const float4 &a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// element offset of row r of an operand read through the strides of the two leading dimensions
__device__ __forceinline__ int64_t row_offset(const int64_t *stride, int i0, int i1) { return i0 * stride[0] + i1 * stride[1]; }

__device__ __forceinline__ float4 load4(const float *base, int64_t off, int lane)
{
    return reinterpret_cast<const float4 *>(base + off)[lane];
}

__global__ __launch_bounds__(kThreads) void add_norm_fwd_kernel(const semidetr_add_norm p, const int rows)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * kWaves + wave) * kFlight;
    if (row0 >= rows) return;
    const float4 w = reinterpret_cast<const float4 *>(p.weight)[lane], b = reinterpret_cast<const float4 *>(p.bias)[lane];
    float4 s[kFlight], t[kFlight], ps[kFlight];
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {      // every load of the batch before the first use; a row past the end re-reads the last
        const int r = min(row0 + i, rows - 1), i0 = r / p.rows1, i1 = r - i0 * p.rows1;
        s[i] = load4(p.x, row_offset(p.x_stride, i0, i1), lane);
        if (p.residual) t[i] = load4(p.residual, row_offset(p.residual_stride, i0, i1), lane);
        if (p.q) ps[i] = load4(p.pos, row_offset(p.pos_stride, i0, i1), lane);
    }
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {
        const int r = row0 + i;
        if (r >= rows) break;
        float4 v = s[i];
        if (p.residual) v = add4(v, t[i]);
        const float mu = wave_sum(sum4(v)) * kInvDim;
        const float4 d = make_float4(v.x - mu, v.y - mu, v.z - mu, v.w - mu);
        const float var = wave_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * kInvDim;
        const float rstd = 1.0f / sqrtf(var + p.eps);
        const float4 y = make_float4((d.x * rstd) * w.x + b.x, (d.y * rstd) * w.y + b.y, (d.z * rstd) * w.z + b.z,
                                     (d.w * rstd) * w.w + b.w);
        reinterpret_cast<float4 *>(p.y + (int64_t)r * kDim)[lane] = y;
        if (p.q) reinterpret_cast<float4 *>(p.q + (int64_t)r * kDim)[lane] = add4(y, ps[i]);
        if (lane == 0) {
            p.mean[r] = mu;
            p.rstd[r] = rstd;
        }
    }
}

template <bool kSums>
__global__ __launch_bounds__(kThreads) void add_norm_bwd_kernel(const semidetr_add_norm p, const int rows, float *slots)
{
    __shared__ float part[kSums ? kWaves * kSlot : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_row0 = (blockIdx.x * kWaves + wave) * kBwdWaveRows;
    const float4 w = reinterpret_cast<const float4 *>(p.weight)[lane];
    float4 dw = make_float4(0.f, 0.f, 0.f, 0.f), db = dw;
    for (int batch = 0; batch < kBwdBatches; ++batch) {
        const int row0 = wave_row0 + batch * kFlight;
        if (row0 >= rows) break;             // the same for every lane of the wave
        float4 s[kFlight], t[kFlight], g[kFlight], h[kFlight];
        float mu[kFlight], rs[kFlight];
        #pragma unroll
        for (int i = 0; i < kFlight; ++i) {
            const int r = min(row0 + i, rows - 1), i0 = r / p.rows1, i1 = r - i0 * p.rows1;
            s[i] = load4(p.x, row_offset(p.x_stride, i0, i1), lane);
            if (p.residual) t[i] = load4(p.residual, row_offset(p.residual_stride, i0, i1), lane);
            if (p.gy) g[i] = load4(p.gy, row_offset(p.gy_stride, i0, i1), lane);
            if (p.gq) h[i] = load4(p.gq, row_offset(p.gq_stride, i0, i1), lane);
            mu[i] = p.mean[r];
            rs[i] = p.rstd[r];
        }
        #pragma unroll
        for (int i = 0; i < kFlight; ++i) {
            const int r = row0 + i;
            if (r >= rows) break;
            float4 v = s[i];
            if (p.residual) v = add4(v, t[i]);
            const float4 gg = p.gy ? (p.gq ? add4(g[i], h[i]) : g[i]) : h[i];
            const float m = mu[i], rstd = rs[i];
            const float4 xh = make_float4((v.x - m) * rstd, (v.y - m) * rstd, (v.z - m) * rstd, (v.w - m) * rstd);
            const float4 gw = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
            const float c1 = wave_sum(sum4(gw)) * kInvDim;
            const float c2 = wave_sum((gw.x * xh.x + gw.y * xh.y) + (gw.z * xh.z + gw.w * xh.w)) * kInvDim;
            const float4 dx = make_float4(rstd * ((gw.x - c1) - xh.x * c2), rstd * ((gw.y - c1) - xh.y * c2),
                                          rstd * ((gw.z - c1) - xh.z * c2), rstd * ((gw.w - c1) - xh.w * c2));
            reinterpret_cast<float4 *>(p.grad_x + (int64_t)r * kDim)[lane] = dx;
            if (kSums) {
                dw = make_float4(dw.x + gg.x * xh.x, dw.y + gg.y * xh.y, dw.z + gg.z * xh.z, dw.w + gg.w * xh.w);
                db = add4(db, gg);
            }
        }
    }
    if (kSums) {                             // a wave without rows adds its zeros: every wave reaches the barrier
        reinterpret_cast<float4 *>(part + wave * kSlot)[lane] = dw;
        reinterpret_cast<float4 *>(part + wave * kSlot + kDim)[lane] = db;
        __syncthreads();
        #pragma unroll
        for (int c = threadIdx.x; c < kSlot; c += kThreads) {
            float acc = part[c];
            #pragma unroll
            for (int k = 1; k < kWaves; ++k) acc += part[k * kSlot + c];
            slots[(int64_t)blockIdx.x * kSlot + c] = acc;
        }
    }
}

// ---- rows of mixed element types (SEMIDETR_ROW_*) ------------------------------------------------------------------------
// The arithmetic of one row between the loads and the stores, ONE source for every combination of types: the expressions of
// the fp32 kernels above in their order, so that the same contractions give the same bits (tests/test_gpu_add_norm_mixed.py).
// s = x + residual of the lane's four columns -> y of those columns, mean and rstd of the row
__device__ __forceinline__ float4 fwd_row(const float4 &v, const float4 &w, const float4 &b, const float eps, float &mu, float &rstd)
{
    mu = wave_sum(sum4(v)) * kInvDim;
    const float4 d = make_float4(v.x - mu, v.y - mu, v.z - mu, v.w - mu);
    const float var = wave_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * kInvDim;
    rstd = 1.0f / sqrtf(var + eps);
    return make_float4((d.x * rstd) * w.x + b.x, (d.y * rstd) * w.y + b.y, (d.z * rstd) * w.z + b.z, (d.w * rstd) * w.w + b.w);
}

// s and g = gy + gq of the lane's four columns, mean and rstd of the row -> dx and xhat
__device__ __forceinline__ float4 bwd_row(const float4 &v, const float4 &gg, const float m, const float rstd, const float4 &w, float4 &xh)
{
    xh = make_float4((v.x - m) * rstd, (v.y - m) * rstd, (v.z - m) * rstd, (v.w - m) * rstd);
    const float4 gw = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
    // The fp32 kernel adds the ROUNDED products here.  Where no result leaves as a float4 the compiler may contract them into
    // the sum instead (seen with the types fixed at compile time and 16-bit gradients only): the copy below is out of its reach.
    float4 rounded = gw;
    asm("" : "+v"(rounded.x), "+v"(rounded.y), "+v"(rounded.z), "+v"(rounded.w));
    const float c1 = wave_sum(sum4(rounded)) * kInvDim;
    const float c2 = wave_sum((gw.x * xh.x + gw.y * xh.y) + (gw.z * xh.z + gw.w * xh.w)) * kInvDim;
    return make_float4(rstd * ((gw.x - c1) - xh.x * c2), rstd * ((gw.y - c1) - xh.y * c2), rstd * ((gw.z - c1) - xh.z * c2),
                       rstd * ((gw.w - c1) - xh.w * c2));
}

// the lane's sums over its wave's rows, in row order: dw += g * xhat, db += g
__device__ __forceinline__ void add_sums(float4 &dw, float4 &db, const float4 &gg, const float4 &xh)
{
    dw = make_float4(dw.x + gg.x * xh.x, dw.y + gg.y * xh.y, dw.z + gg.z * xh.z, dw.w + gg.w * xh.w);
    db = add4(db, gg);
}

// The four waves' sums -> slot blockIdx.x, in wave order.  A wave without rows adds its zeros: every wave reaches the barrier.
__device__ __forceinline__ void store_slot(float *part, const float4 &dw, const float4 &db, float *slots, int lane, int wave)
{
    reinterpret_cast<float4 *>(part + wave * kSlot)[lane] = dw;
    reinterpret_cast<float4 *>(part + wave * kSlot + kDim)[lane] = db;
    __syncthreads();
    #pragma unroll
    for (int c = threadIdx.x; c < kSlot; c += kThreads) {
        float acc = part[c];
        #pragma unroll
        for (int k = 1; k < kWaves; ++k) acc += part[k * kSlot + c];
        slots[(int64_t)blockIdx.x * kSlot + c] = acc;
    }
}

// The kernels above with each operand loaded and each result stored in its own type.  The type codes are kernel arguments, so
// every choice below is one scalar branch of the whole wave and any mixture runs in one launch.  A 16-bit row is one 8-byte
// load / store per lane; the load phase keeps the raw bits (the first two dwords of a float4) and the up-cast happens in the
// arithmetic phase, so no branch of the load phase waits for memory.  (Instances with the codes fixed at compile time for the
// combinations autocast and .half() modules produce were built and measured: no faster)
__device__ __forceinline__ float4 load_raw(const void *base, int64_t off, int lane, int type)
{
    if (type == SEMIDETR_ROW_F32) return load4(static_cast<const float *>(base), off, lane);
    const float2 r = reinterpret_cast<const float2 *>(static_cast<const unsigned short *>(base) + off)[lane];
    return make_float4(r.x, r.y, 0.f, 0.f);
}

__device__ __forceinline__ float4 up4(const float4 &raw, int type)
{
    if (type == SEMIDETR_ROW_F32) return raw;
    const float2 r = make_float2(raw.x, raw.y);
    return type == SEMIDETR_ROW_FP16 ? unpack4<__half>(r) : unpack4<__hip_bfloat16>(r);
}

// row r of a contiguous (rows, 256) result: the unrounded fp32 values, rounded once where the result is 16-bit
__device__ __forceinline__ void store_row(void *base, int r, int lane, int type, const float4 &v)
{
    if (type == SEMIDETR_ROW_F32) {
        reinterpret_cast<float4 *>(static_cast<float *>(base) + (int64_t)r * kDim)[lane] = v;
        return;
    }
    uint2 bits;
    if (type == SEMIDETR_ROW_FP16) bits = make_uint2(pack2<__half>(v.x, v.y), pack2<__half>(v.z, v.w));
    else bits = make_uint2(pack2<__hip_bfloat16>(v.x, v.y), pack2<__hip_bfloat16>(v.z, v.w));
    reinterpret_cast<uint2 *>(static_cast<unsigned short *>(base) + (int64_t)r * kDim)[lane] = bits;
}

__global__ __launch_bounds__(kThreads) void add_norm_fwd_mixed_kernel(const semidetr_add_norm_mixed p, const int rows)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * kWaves + wave) * kFlight;
    if (row0 >= rows) return;
    const float4 w = reinterpret_cast<const float4 *>(p.weight)[lane], b = reinterpret_cast<const float4 *>(p.bias)[lane];
    float4 s[kFlight], t[kFlight], ps[kFlight];
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {
        const int r = min(row0 + i, rows - 1), i0 = r / p.rows1, i1 = r - i0 * p.rows1;
        s[i] = load_raw(p.x, row_offset(p.x_stride, i0, i1), lane, p.x_type);
        if (p.residual) t[i] = load_raw(p.residual, row_offset(p.residual_stride, i0, i1), lane, p.residual_type);
        if (p.q) ps[i] = load_raw(p.pos, row_offset(p.pos_stride, i0, i1), lane, p.pos_type);
    }
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {
        const int r = row0 + i;
        if (r >= rows) break;
        float4 v = up4(s[i], p.x_type);
        if (p.residual) v = add4(v, up4(t[i], p.residual_type));
        float mu, rstd;
        const float4 y = fwd_row(v, w, b, p.eps, mu, rstd);
        store_row(p.y, r, lane, p.y_type, y);
        if (p.q) store_row(p.q, r, lane, p.q_type, add4(y, up4(ps[i], p.pos_type)));
        if (lane == 0) {
            p.mean[r] = mu;
            p.rstd[r] = rstd;
        }
    }
}

template <bool kSums>
__global__ __launch_bounds__(kThreads) void add_norm_bwd_mixed_kernel(const semidetr_add_norm_mixed p, const int rows, float *slots)
{
    __shared__ float part[kSums ? kWaves * kSlot : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_row0 = (blockIdx.x * kWaves + wave) * kBwdWaveRows;
    const float4 w = reinterpret_cast<const float4 *>(p.weight)[lane];
    float4 dw = make_float4(0.f, 0.f, 0.f, 0.f), db = dw;
    for (int batch = 0; batch < kBwdBatches; ++batch) {
        const int row0 = wave_row0 + batch * kFlight;
        if (row0 >= rows) break;             // the same for every lane of the wave
        float4 s[kFlight], t[kFlight], g[kFlight], h[kFlight];
        float mu[kFlight], rs[kFlight];
        #pragma unroll
        for (int i = 0; i < kFlight; ++i) {
            const int r = min(row0 + i, rows - 1), i0 = r / p.rows1, i1 = r - i0 * p.rows1;
            s[i] = load_raw(p.x, row_offset(p.x_stride, i0, i1), lane, p.x_type);
            if (p.residual) t[i] = load_raw(p.residual, row_offset(p.residual_stride, i0, i1), lane, p.residual_type);
            if (p.gy) g[i] = load_raw(p.gy, row_offset(p.gy_stride, i0, i1), lane, p.gy_type);
            if (p.gq) h[i] = load_raw(p.gq, row_offset(p.gq_stride, i0, i1), lane, p.gq_type);
            mu[i] = p.mean[r];
            rs[i] = p.rstd[r];
        }
        #pragma unroll
        for (int i = 0; i < kFlight; ++i) {
            const int r = row0 + i;
            if (r >= rows) break;
            float4 v = up4(s[i], p.x_type);
            if (p.residual) v = add4(v, up4(t[i], p.residual_type));
            const float4 hq = p.gq ? up4(h[i], p.gq_type) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 gg = p.gy ? (p.gq ? add4(up4(g[i], p.gy_type), hq) : up4(g[i], p.gy_type)) : hq;
            float4 xh;
            const float4 dx = bwd_row(v, gg, mu[i], rs[i], w, xh);
            if (p.grad_x) store_row(p.grad_x, r, lane, p.grad_x_type, dx);
            if (p.grad_residual) store_row(p.grad_residual, r, lane, p.grad_residual_type, dx);
            if (p.grad_pos) store_row(p.grad_pos, r, lane, p.grad_pos_type, hq);
            if (kSums) add_sums(dw, db, gg, xh);
        }
    }
    if (kSums) store_slot(part, dw, db, slots, lane, wave);
}

__global__ __launch_bounds__(64 * kParts) void add_norm_param_kernel(const float *slots, const int num_slots, float *grad_weight,
                                                                      float *grad_bias)
{
    __shared__ double part[kParts][64];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;                      // 0 .. 511: dweight | dbias
    float *out = col < kDim ? grad_weight : grad_bias;           // the same for the whole workgroup (64 divides 256)
    if (!out) return;
    const int chunk = (num_slots + kParts - 1) / kParts;
    const int first = k * chunk, last = min(first + chunk, num_slots);
    double acc = 0.0;
    #pragma unroll 8
    for (int sl = first; sl < last; ++sl) acc += (double)slots[(int64_t)sl * kSlot + col];
    part[k][lane] = acc;
    __syncthreads();
    if (k == 0) {
        #pragma unroll
        for (int j = 1; j < kParts; ++j) acc += part[j][lane];
        out[col & (kDim - 1)] = (float)acc;
    }
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }
bool rows_ok(const void *ptr, const int64_t *stride)
{
    return aligned16(ptr) && stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0;
}

int64_t num_slots(int64_t rows) { return (rows + kBwdGroupRows - 1) / kBwdGroupRows; }

// Host-side check of the parameter block.  Returns SEMIDETR_OK or an error (message set); `rows` is rows0 * rows1.
int plan(const semidetr_add_norm *params, int for_backward, int &rows)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "add_norm: null pointer (parameter block)");
    const semidetr_add_norm &p = params[0];
    SEMIDETR_REQUIRE(p.dim == kDim, SEMIDETR_E_BADARG, "add_norm: row width %d (only %d is built)", p.dim, kDim);
    SEMIDETR_REQUIRE(p.rows0 > 0 && p.rows1 > 0, SEMIDETR_E_BADARG, "add_norm: bad sizes (rows0=%d rows1=%d)", p.rows0, p.rows1);
    SEMIDETR_REQUIRE((int64_t)p.rows0 * p.rows1 < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                     "add_norm: too large (rows0 * rows1 < 2^31)");
    SEMIDETR_REQUIRE(p.eps == p.eps, SEMIDETR_E_BADARG, "add_norm: eps is NaN");
    SEMIDETR_REQUIRE(p.x && p.weight && p.mean && p.rstd, SEMIDETR_E_BADARG, "add_norm: null pointer (x / weight / mean / rstd)");
    SEMIDETR_REQUIRE(rows_ok(p.x, p.x_stride) && (!p.residual || rows_ok(p.residual, p.residual_stride)) && aligned16(p.weight),
                     SEMIDETR_E_BADARG, "add_norm: rows must be 16-byte aligned (base and strides) with non-negative strides");
    if (!for_backward) {
        SEMIDETR_REQUIRE(p.bias && p.y, SEMIDETR_E_BADARG, "add_norm forward: null pointer (bias / y)");
        SEMIDETR_REQUIRE(!p.q == !p.pos, SEMIDETR_E_BADARG, "add_norm forward: q and pos come together");
        SEMIDETR_REQUIRE(aligned16(p.bias) && aligned16(p.y) && aligned16(p.q) && (!p.pos || rows_ok(p.pos, p.pos_stride)),
                         SEMIDETR_E_BADARG, "add_norm forward: bias, y, q and the rows of pos must be 16-byte aligned");
    } else {
        SEMIDETR_REQUIRE(p.gy || p.gq, SEMIDETR_E_BADARG, "add_norm backward: null pointer (gy and gq)");
        SEMIDETR_REQUIRE(p.grad_x && aligned16(p.grad_x), SEMIDETR_E_BADARG, "add_norm backward: null or misaligned grad_x");
        SEMIDETR_REQUIRE((!p.gy || rows_ok(p.gy, p.gy_stride)) && (!p.gq || rows_ok(p.gq, p.gq_stride)), SEMIDETR_E_BADARG,
                         "add_norm backward: the rows of gy and gq must be 16-byte aligned (base and strides)");
    }
    rows = (int)((int64_t)p.rows0 * p.rows1);
    return SEMIDETR_OK;
}

// ---- the mixed entry points: alignment per element type -----------------------------------------------------------
bool type_ok(int type) { return type == SEMIDETR_ROW_F32 || type == SEMIDETR_ROW_FP16 || type == SEMIDETR_ROW_BF16; }
// the alignment of a row of `type`: 16 bytes (one float4 per lane) or 8 bytes (four 16-bit elements per lane)
bool aligned_for(const void *ptr, int type) { return ((uintptr_t)ptr & (type == SEMIDETR_ROW_F32 ? 15 : 7)) == 0; }

// One row operand (`result` = 0: read through its strides) or contiguous row result (`result` = 1); NULL passes.
int row_check(const char *what, const void *ptr, int type, const int64_t *stride, int result)
{
    if (!ptr) return SEMIDETR_OK;
    SEMIDETR_REQUIRE(type_ok(type), SEMIDETR_E_BADARG, "add_norm mixed: unknown type code %d of %s (SEMIDETR_ROW_F32 / _FP16 / _BF16)",
                     type, what);
    SEMIDETR_REQUIRE(aligned_for(ptr, type) && (result || (stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0)),
                     SEMIDETR_E_BADARG, "add_norm mixed: the rows of %s must be %d-byte aligned (base%s)", what,
                     type == SEMIDETR_ROW_F32 ? 16 : 8, result ? "" : "; strides non-negative multiples of 4 elements");
    return SEMIDETR_OK;
}

int plan_mixed(const semidetr_add_norm_mixed *params, int for_backward, int &rows)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "add_norm mixed: null pointer (parameter block)");
    const semidetr_add_norm_mixed &p = params[0];
    SEMIDETR_REQUIRE(p.dim == kDim, SEMIDETR_E_BADARG, "add_norm mixed: row width %d (only %d is built)", p.dim, kDim);
    SEMIDETR_REQUIRE(p.rows0 > 0 && p.rows1 > 0, SEMIDETR_E_BADARG, "add_norm mixed: bad sizes (rows0=%d rows1=%d)", p.rows0, p.rows1);
    SEMIDETR_REQUIRE((int64_t)p.rows0 * p.rows1 < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                     "add_norm mixed: too large (rows0 * rows1 < 2^31)");
    SEMIDETR_REQUIRE(p.eps == p.eps, SEMIDETR_E_BADARG, "add_norm mixed: eps is NaN");
    SEMIDETR_REQUIRE(p.x && p.weight && p.mean && p.rstd, SEMIDETR_E_BADARG, "add_norm mixed: null pointer (x / weight / mean / rstd)");
    SEMIDETR_REQUIRE(aligned16(p.weight), SEMIDETR_E_BADARG, "add_norm mixed: weight must be 16-byte aligned");
    if (int rc = row_check("x", p.x, p.x_type, p.x_stride, 0)) return rc;
    if (int rc = row_check("residual", p.residual, p.residual_type, p.residual_stride, 0)) return rc;
    if (!for_backward) {
        SEMIDETR_REQUIRE(p.bias && p.y, SEMIDETR_E_BADARG, "add_norm mixed forward: null pointer (bias / y)");
        SEMIDETR_REQUIRE(!p.q == !p.pos, SEMIDETR_E_BADARG, "add_norm mixed forward: q and pos come together");
        SEMIDETR_REQUIRE(aligned16(p.bias), SEMIDETR_E_BADARG, "add_norm mixed forward: bias must be 16-byte aligned");
        if (int rc = row_check("pos", p.pos, p.pos_type, p.pos_stride, 0)) return rc;
        if (int rc = row_check("y", p.y, p.y_type, nullptr, 1)) return rc;
        if (int rc = row_check("q", p.q, p.q_type, nullptr, 1)) return rc;
    } else {
        SEMIDETR_REQUIRE(p.gy || p.gq, SEMIDETR_E_BADARG, "add_norm mixed backward: null pointer (gy and gq)");
        SEMIDETR_REQUIRE(p.grad_x || p.grad_residual, SEMIDETR_E_BADARG, "add_norm mixed backward: null pointer (grad_x and grad_residual)");
        SEMIDETR_REQUIRE(!p.grad_residual || p.residual, SEMIDETR_E_BADARG, "add_norm mixed backward: grad_residual without residual");
        SEMIDETR_REQUIRE(!p.grad_pos || p.gq, SEMIDETR_E_BADARG, "add_norm mixed backward: grad_pos without gq");
        if (int rc = row_check("gy", p.gy, p.gy_type, p.gy_stride, 0)) return rc;
        if (int rc = row_check("gq", p.gq, p.gq_type, p.gq_stride, 0)) return rc;
        if (int rc = row_check("grad_x", p.grad_x, p.grad_x_type, nullptr, 1)) return rc;
        if (int rc = row_check("grad_residual", p.grad_residual, p.grad_residual_type, nullptr, 1)) return rc;
        if (int rc = row_check("grad_pos", p.grad_pos, p.grad_pos_type, nullptr, 1)) return rc;
    }
    rows = (int)((int64_t)p.rows0 * p.rows1);
    return SEMIDETR_OK;
}


}  // namespace

extern "C" size_t semidetr_add_norm_workspace_bytes(int64_t rows)
{
    if (rows < 1 || rows >= ((int64_t)1 << 31)) return 0;
    return (size_t)num_slots(rows) * kSlot * sizeof(float);
}

extern "C" int semidetr_add_norm_forward_f32(void *stream, const semidetr_add_norm *params, void *workspace, size_t workspace_bytes)
{
    int rows = 0;
    if (int rc = plan(params, 0, rows)) return rc;
    (void)workspace;
    (void)workspace_bytes;                   // the forward needs none
    const int per_group = kWaves * kFlight;
    hipLaunchKernelGGL(add_norm_fwd_kernel, dim3((rows + per_group - 1) / per_group), dim3(kThreads), 0,
                       semidetr::as_stream(stream), params[0], rows);
    return semidetr::launch_status("add_norm_fwd_kernel");
}

extern "C" int semidetr_add_norm_backward_f32(void *stream, const semidetr_add_norm *params, void *workspace, size_t workspace_bytes)
{
    int rows = 0;
    if (int rc = plan(params, 1, rows)) return rc;
    const semidetr_add_norm &p = params[0];
    const bool sums = p.grad_weight || p.grad_bias;
    const int groups = (int)num_slots(rows);
    hipStream_t st = semidetr::as_stream(stream);
    if (!sums) {
        hipLaunchKernelGGL(add_norm_bwd_kernel<false>, dim3(groups), dim3(kThreads), 0, st, p, rows, nullptr);
        return semidetr::launch_status("add_norm_bwd_kernel");
    }
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= semidetr_add_norm_workspace_bytes(rows),
                     SEMIDETR_E_BADARG, "add_norm backward: workspace null, misaligned or smaller than semidetr_add_norm_workspace_bytes()");
    float *slots = static_cast<float *>(workspace);
    hipLaunchKernelGGL(add_norm_bwd_kernel<true>, dim3(groups), dim3(kThreads), 0, st, p, rows, slots);
    if (int rc = semidetr::launch_status("add_norm_bwd_kernel")) return rc;
    hipLaunchKernelGGL(add_norm_param_kernel, dim3(kSlot / 64), dim3(64 * kParts), 0, st, slots, groups, p.grad_weight, p.grad_bias);
    return semidetr::launch_status("add_norm_param_kernel");
}

extern "C" int semidetr_add_norm_forward_mixed(void *stream, const semidetr_add_norm_mixed *params, void *workspace,
                                               size_t workspace_bytes)
{
    int rows = 0;
    if (int rc = plan_mixed(params, 0, rows)) return rc;
    (void)workspace;
    (void)workspace_bytes;                   // the forward needs none
    const int per_group = kWaves * kFlight;
    hipLaunchKernelGGL(add_norm_fwd_mixed_kernel, dim3((rows + per_group - 1) / per_group), dim3(kThreads), 0,
                       semidetr::as_stream(stream), params[0], rows);
    return semidetr::launch_status("add_norm_fwd_mixed_kernel");
}

extern "C" int semidetr_add_norm_backward_mixed(void *stream, const semidetr_add_norm_mixed *params, void *workspace,
                                                size_t workspace_bytes)
{
    int rows = 0;
    if (int rc = plan_mixed(params, 1, rows)) return rc;
    const semidetr_add_norm_mixed &p = params[0];
    const bool sums = p.grad_weight || p.grad_bias;
    const int groups = (int)num_slots(rows);
    hipStream_t st = semidetr::as_stream(stream);
    if (!sums) {
        hipLaunchKernelGGL(add_norm_bwd_mixed_kernel<false>, dim3(groups), dim3(kThreads), 0, st, p, rows, nullptr);
        return semidetr::launch_status("add_norm_bwd_mixed_kernel");
    }
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= semidetr_add_norm_workspace_bytes(rows),
                     SEMIDETR_E_BADARG,
                     "add_norm mixed backward: workspace null, misaligned or smaller than semidetr_add_norm_workspace_bytes()");
    float *slots = static_cast<float *>(workspace);
    hipLaunchKernelGGL(add_norm_bwd_mixed_kernel<true>, dim3(groups), dim3(kThreads), 0, st, p, rows, slots);
    if (int rc = semidetr::launch_status("add_norm_bwd_mixed_kernel")) return rc;
    hipLaunchKernelGGL(add_norm_param_kernel, dim3(kSlot / 64), dim3(64 * kParts), 0, st, slots, groups, p.grad_weight, p.grad_bias);
    return semidetr::launch_status("add_norm_param_kernel");
}

// Residual add + LayerNorm + positional add for gfx950, row width 256 (the model's d_model), forward and backward: the epilogue
// of every transformer sub-block (detr_od/models/utils/transformer.py:628-629, 636-637, 789-790, 811-812, 838-839) and the
// with_pos_embed that opens the next one.  fp32 arithmetic; the *_f32 entry points are fp32 in and out, the *_mixed entry points
// read and write rows of fp32, fp16 or bf16 elements, each operand and each result in its own type.
//
//   add_norm_fwd_kernel<typed>        workgroup = 4 waves, wave = 4 rows in flight, lane = 4 columns; no LDS, no barrier.  Reads x,
//                                     residual, pos once; writes y, q = y + pos, mean, rstd.
//   add_norm_bwd_kernel<typed, sums>  workgroup = 4 waves, wave = 16 consecutive rows in 4 batches of 4 rows in flight.  Reads x,
//                                     residual, gy, gq, mean, rstd; stores its one fp32 dx as grad_x and / or grad_residual and gq
//                                     as grad_pos.  <., true>: every lane also adds g * xhat and g of its four columns over its
//                                     wave's rows in row order; the four waves combine through LDS in wave order into slot
//                                     blockIdx.x of the workspace (512 floats: dweight | dbias).
//   add_norm_param_kernel             8 workgroups x 64 columns x 16 parts: part k adds slots [k * chunk, (k + 1) * chunk) in index
//                                     order in fp64, the 16 parts are added in part order, one rounding to fp32.
// Both templates take the semidetr_add_norm_mixed block; the grid, the row -> wave map, the batches and the slots do not depend
// on <typed>, only how a row is loaded and stored does:
//   <false>  the *_f32 entry points (the host widens their block: every type fp32, grad_residual and grad_pos NULL).  The type
//            fields are not read: every row is one 16-byte load / store per lane, straight-line code.
//   <true>   the *_mixed entry points.  The type codes are kernel arguments; a 16-bit operand is one 8-byte load per lane, up-cast
//            exactly; a 16-bit result is rounded once, to nearest even, from the unrounded fp32 value (q from the unrounded
//            y + pos; fp16 overflows to inf); grad_x and grad_residual each in its type, grad_pos in pos's.
// The grid, the row -> wave map, the slot count and the chunks are functions of `rows` alone: no float atomics, no memset, two
// runs are bitwise equal.
//
// Arithmetic per row, in this order (tests/add_norm_ref64.py bounds it; the compiler may contract a * b + c into an fma):
//   s = x + residual; mu = (sum_lanes ((s0 + s1) + (s2 + s3))) / 256 by a xor butterfly (every lane holds the same bits);
//   d = s - mu; var = (sum d^2) / 256 the same way; rstd = 1 / sqrt(var + eps); y = (d * rstd) * w + b; q = y + pos.
//   backward: g = gy + gq; xhat = (x + residual - mu) * rstd; gw = g * w; c1 = (sum gw) / 256; c2 = (sum gw * xhat) / 256;
//   dx = rstd * ((gw - c1) - xhat * c2).  The lane's part of c2 has its contraction written out (dot4): it differs between
//   the instances with and without the parameter sums, so grad_x of the two differs in its last bits.
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

// ---- the arithmetic of one row between the loads and the stores: the only statement of it, for both instances ----------------
// Except in dot4, which products become fmas is the compiler's choice per basic block, so the bits also depend on the branches
// the kernels put around these functions (hence the fp32 instance's grad_x store outside every branch); the tests that compare
// the two instances with each other and the typed one with the fp32 one on up-cast operands bit for bit hold that choice still.
// s = x + residual of the lane's four columns -> y of those columns, mean and rstd of the row
__device__ __forceinline__ float4 fwd_row(const float4 &v, const float4 &w, const float4 &b, const float eps, float &mu, float &rstd)
{
    mu = wave_sum(sum4(v)) * kInvDim;
    const float4 d = make_float4(v.x - mu, v.y - mu, v.z - mu, v.w - mu);
    const float var = wave_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) * kInvDim;
    rstd = 1.0f / sqrtf(var + eps);
    return make_float4((d.x * rstd) * w.x + b.x, (d.y * rstd) * w.y + b.y, (d.z * rstd) * w.z + b.z, (d.w * rstd) * w.w + b.w);
}

// The lane's part of the sum for c2.  One product of each pair is rounded and the other goes into an fma, and which one was the
// compiler's choice per kernel when the fp32 backward kernels were two bodies: with the parameter sums it rounded x and z, without
// them y and w, so grad_x of the two launches differs in its last bits.  Those bits are the entry points' behaviour by now, so
// the choice is written out here, with contraction off, where it no longer moves with the code around it.
template <bool kSums>
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b)
{
    #pragma clang fp contract(off)
    if (kSums) return __builtin_fmaf(a.y, b.y, a.x * b.x) + __builtin_fmaf(a.w, b.w, a.z * b.z);
    return __builtin_fmaf(a.x, b.x, a.y * b.y) + __builtin_fmaf(a.z, b.z, a.w * b.w);
}

// s and g = gy + gq of the lane's four columns, mean and rstd of the row -> dx and xhat
template <bool kFence, bool kSums>
__device__ __forceinline__ float4 bwd_row(const float4 &v, const float4 &gg, const float m, const float rstd, const float4 &w, float4 &xh)
{
    xh = make_float4((v.x - m) * rstd, (v.y - m) * rstd, (v.z - m) * rstd, (v.w - m) * rstd);
    const float4 gw = make_float4(gg.x * w.x, gg.y * w.y, gg.z * w.z, gg.w * w.w);
    // c1 is the sum of the ROUNDED products: that is what the fp32 instance compiles to, and its bits are the contract.  Where no
    // result leaves as a float4 the compiler may contract the products into the sum instead (seen with the types fixed at compile
    // time and 16-bit gradients only), so the typed instance hands the sum a copy that is out of the compiler's reach.  The fp32
    // instance goes without the fence: there it buys nothing and costs 16 v_mov per batch and 2 VGPRs with the sums.
    float4 rounded = gw;
    if (kFence) asm("" : "+v"(rounded.x), "+v"(rounded.y), "+v"(rounded.z), "+v"(rounded.w));
    const float c1 = wave_sum(sum4(rounded)) * kInvDim;
    const float c2 = wave_sum(dot4<kSums>(gw, xh)) * kInvDim;
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

// ---- rows in their element type (SEMIDETR_ROW_*) ---------------------------------------------------------------------------------
// The code of a row: the block's field in the typed instance, where every choice below is one scalar branch of the whole wave and
// any mixture runs in one launch; the constant fp32 in the other, where the field is not read and the three functions below are
// the plain float4 access.  (Instances with the codes fixed at compile time for the combinations autocast and .half() modules
// produce were built and measured: no faster)
template <bool kTyped>
__device__ __forceinline__ int code(const int &field) { return kTyped ? field : SEMIDETR_ROW_F32; }

// A 16-bit row is one 8-byte load / store per lane; the load phase keeps the raw bits (the first two dwords of a float4) and the
// up-cast happens in the arithmetic phase, so no branch of the load phase waits for memory.
__device__ __forceinline__ float4 load_raw(const void *base, int64_t off, int lane, int type)
{
    if (type == SEMIDETR_ROW_F32) return reinterpret_cast<const float4 *>(static_cast<const float *>(base) + off)[lane];
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

template <bool kTyped>
__global__ __launch_bounds__(kThreads) void add_norm_fwd_kernel(const semidetr_add_norm_mixed p, const int rows)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * kWaves + wave) * kFlight;
    if (row0 >= rows) return;
    const int x_type = code<kTyped>(p.x_type), residual_type = code<kTyped>(p.residual_type), pos_type = code<kTyped>(p.pos_type);
    const float4 w = reinterpret_cast<const float4 *>(p.weight)[lane], b = reinterpret_cast<const float4 *>(p.bias)[lane];
    float4 s[kFlight], t[kFlight], ps[kFlight];
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {      // every load of the batch before the first use; a row past the end re-reads the last
        const int r = min(row0 + i, rows - 1), i0 = r / p.rows1, i1 = r - i0 * p.rows1;
        s[i] = load_raw(p.x, row_offset(p.x_stride, i0, i1), lane, x_type);
        if (p.residual) t[i] = load_raw(p.residual, row_offset(p.residual_stride, i0, i1), lane, residual_type);
        if (p.q) ps[i] = load_raw(p.pos, row_offset(p.pos_stride, i0, i1), lane, pos_type);
    }
    #pragma unroll
    for (int i = 0; i < kFlight; ++i) {
        const int r = row0 + i;
        if (r >= rows) break;
        float4 v = up4(s[i], x_type);
        if (p.residual) v = add4(v, up4(t[i], residual_type));
        float mu, rstd;
        const float4 y = fwd_row(v, w, b, p.eps, mu, rstd);
        store_row(p.y, r, lane, code<kTyped>(p.y_type), y);
        if (p.q) store_row(p.q, r, lane, code<kTyped>(p.q_type), add4(y, up4(ps[i], pos_type)));
        if (lane == 0) {
            p.mean[r] = mu;
            p.rstd[r] = rstd;
        }
    }
}

template <bool kTyped, bool kSums>
__global__ __launch_bounds__(kThreads) void add_norm_bwd_kernel(const semidetr_add_norm_mixed p, const int rows, float *slots)
{
    __shared__ float part[kSums ? kWaves * kSlot : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_row0 = (blockIdx.x * kWaves + wave) * kBwdWaveRows;
    const int x_type = code<kTyped>(p.x_type), residual_type = code<kTyped>(p.residual_type);
    const int gy_type = code<kTyped>(p.gy_type), gq_type = code<kTyped>(p.gq_type);
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
            s[i] = load_raw(p.x, row_offset(p.x_stride, i0, i1), lane, x_type);
            if (p.residual) t[i] = load_raw(p.residual, row_offset(p.residual_stride, i0, i1), lane, residual_type);
            if (p.gy) g[i] = load_raw(p.gy, row_offset(p.gy_stride, i0, i1), lane, gy_type);
            if (p.gq) h[i] = load_raw(p.gq, row_offset(p.gq_stride, i0, i1), lane, gq_type);
            mu[i] = p.mean[r];
            rs[i] = p.rstd[r];
        }
        #pragma unroll
        for (int i = 0; i < kFlight; ++i) {
            const int r = row0 + i;
            if (r >= rows) break;
            float4 v = up4(s[i], x_type);
            if (p.residual) v = add4(v, up4(t[i], residual_type));
            const float4 gg = p.gy ? (p.gq ? add4(up4(g[i], gy_type), up4(h[i], gq_type)) : up4(g[i], gy_type)) : up4(h[i], gq_type);
            float4 xh;
            const float4 dx = bwd_row<kTyped, kSums>(v, gg, mu[i], rs[i], w, xh);
            // the fp32 instance writes grad_x, which plan() has seen set, and nothing else: one store outside every branch
            if (!kTyped || p.grad_x) store_row(p.grad_x, r, lane, code<kTyped>(p.grad_x_type), dx);
            if (kTyped && p.grad_residual) store_row(p.grad_residual, r, lane, code<kTyped>(p.grad_residual_type), dx);
            if (kTyped && p.grad_pos) store_row(p.grad_pos, r, lane, code<kTyped>(p.grad_pos_type), up4(h[i], gq_type));
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

// ---- host side: one check and one launch helper per direction, on the semidetr_add_norm_mixed block -----------------------------
bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }
int64_t num_slots(int64_t rows) { return (rows + kBwdGroupRows - 1) / kBwdGroupRows; }

// One row operand (`result` = 0: read through its strides) or contiguous row result (`result` = 1); NULL passes.  A row starts
// 16-byte aligned (fp32: one float4 per lane) or 8-byte aligned (four 16-bit elements per lane).
int row_check(const char *what, const void *ptr, int type, const int64_t *stride, int result)
{
    if (!ptr) return SEMIDETR_OK;
    SEMIDETR_REQUIRE(type == SEMIDETR_ROW_F32 || type == SEMIDETR_ROW_FP16 || type == SEMIDETR_ROW_BF16, SEMIDETR_E_BADARG,
                     "add_norm: unknown type code %d of %s (SEMIDETR_ROW_F32 / _FP16 / _BF16)", type, what);
    const int bytes = type == SEMIDETR_ROW_F32 ? 16 : 8;
    SEMIDETR_REQUIRE(((uintptr_t)ptr & (bytes - 1)) == 0 &&
                         (result || (stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0)),
                     SEMIDETR_E_BADARG, "add_norm: the rows of %s must be %d-byte aligned (base%s)", what, bytes,
                     result ? "" : "; strides non-negative multiples of 4 elements");
    return SEMIDETR_OK;
}

// Host-side check of the parameter block.  Returns SEMIDETR_OK or an error (message set); `rows` is rows0 * rows1.
int plan(const semidetr_add_norm_mixed *params, int for_backward, int &rows)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "add_norm: null pointer (parameter block)");
    const semidetr_add_norm_mixed &p = params[0];
    SEMIDETR_REQUIRE(p.dim == kDim, SEMIDETR_E_BADARG, "add_norm: row width %d (only %d is built)", p.dim, kDim);
    SEMIDETR_REQUIRE(p.rows0 > 0 && p.rows1 > 0, SEMIDETR_E_BADARG, "add_norm: bad sizes (rows0=%d rows1=%d)", p.rows0, p.rows1);
    SEMIDETR_REQUIRE((int64_t)p.rows0 * p.rows1 < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                     "add_norm: too large (rows0 * rows1 < 2^31)");
    SEMIDETR_REQUIRE(p.eps == p.eps, SEMIDETR_E_BADARG, "add_norm: eps is NaN");
    SEMIDETR_REQUIRE(p.x && p.weight && p.mean && p.rstd, SEMIDETR_E_BADARG, "add_norm: null pointer (x / weight / mean / rstd)");
    SEMIDETR_REQUIRE(aligned16(p.weight), SEMIDETR_E_BADARG, "add_norm: weight must be 16-byte aligned");
    if (int rc = row_check("x", p.x, p.x_type, p.x_stride, 0)) return rc;
    if (int rc = row_check("residual", p.residual, p.residual_type, p.residual_stride, 0)) return rc;
    if (!for_backward) {
        SEMIDETR_REQUIRE(p.bias && p.y, SEMIDETR_E_BADARG, "add_norm forward: null pointer (bias / y)");
        SEMIDETR_REQUIRE(!p.q == !p.pos, SEMIDETR_E_BADARG, "add_norm forward: q and pos come together");
        SEMIDETR_REQUIRE(aligned16(p.bias), SEMIDETR_E_BADARG, "add_norm forward: bias must be 16-byte aligned");
        if (int rc = row_check("pos", p.pos, p.pos_type, p.pos_stride, 0)) return rc;
        if (int rc = row_check("y", p.y, p.y_type, nullptr, 1)) return rc;
        if (int rc = row_check("q", p.q, p.q_type, nullptr, 1)) return rc;
    } else {
        SEMIDETR_REQUIRE(p.gy || p.gq, SEMIDETR_E_BADARG, "add_norm backward: null pointer (gy and gq)");
        SEMIDETR_REQUIRE(p.grad_x || p.grad_residual, SEMIDETR_E_BADARG, "add_norm backward: null pointer (grad_x and grad_residual)");
        SEMIDETR_REQUIRE(!p.grad_residual || p.residual, SEMIDETR_E_BADARG, "add_norm backward: grad_residual without residual");
        SEMIDETR_REQUIRE(!p.grad_pos || p.gq, SEMIDETR_E_BADARG, "add_norm backward: grad_pos without gq");
        if (int rc = row_check("gy", p.gy, p.gy_type, p.gy_stride, 0)) return rc;
        if (int rc = row_check("gq", p.gq, p.gq_type, p.gq_stride, 0)) return rc;
        if (int rc = row_check("grad_x", p.grad_x, p.grad_x_type, nullptr, 1)) return rc;
        if (int rc = row_check("grad_residual", p.grad_residual, p.grad_residual_type, nullptr, 1)) return rc;
        if (int rc = row_check("grad_pos", p.grad_pos, p.grad_pos_type, nullptr, 1)) return rc;
    }
    rows = (int)((int64_t)p.rows0 * p.rows1);
    return SEMIDETR_OK;
}

// The fp32 block as the block the kernels take: every row fp32, no grad_residual, no grad_pos.  NULL stays NULL for plan().
const semidetr_add_norm_mixed *widen(const semidetr_add_norm *params, semidetr_add_norm_mixed &wide)
{
    static_assert(SEMIDETR_ROW_F32 == 0, "the zeroed block below has every type code fp32");
    if (!params) return nullptr;
    const semidetr_add_norm &p = params[0];
    wide = semidetr_add_norm_mixed{};
    wide.rows0 = p.rows0, wide.rows1 = p.rows1, wide.dim = p.dim, wide.eps = p.eps;
    wide.x = p.x, wide.residual = p.residual, wide.pos = p.pos, wide.gy = p.gy, wide.gq = p.gq;
    for (int k = 0; k < 2; ++k) {
        wide.x_stride[k] = p.x_stride[k], wide.residual_stride[k] = p.residual_stride[k], wide.pos_stride[k] = p.pos_stride[k];
        wide.gy_stride[k] = p.gy_stride[k], wide.gq_stride[k] = p.gq_stride[k];
    }
    wide.weight = p.weight, wide.bias = p.bias, wide.y = p.y, wide.q = p.q, wide.mean = p.mean, wide.rstd = p.rstd;
    wide.grad_x = p.grad_x, wide.grad_weight = p.grad_weight, wide.grad_bias = p.grad_bias;
    return &wide;
}

template <bool kTyped>
int forward(void *stream, const semidetr_add_norm_mixed *params)
{
    int rows = 0;
    if (int rc = plan(params, 0, rows)) return rc;
    const int per_group = kWaves * kFlight;
    hipLaunchKernelGGL(add_norm_fwd_kernel<kTyped>, dim3((rows + per_group - 1) / per_group), dim3(kThreads), 0,
                       semidetr::as_stream(stream), params[0], rows);
    return semidetr::launch_status("add_norm_fwd_kernel");
}

template <bool kTyped>
int backward(void *stream, const semidetr_add_norm_mixed *params, void *workspace, size_t workspace_bytes)
{
    int rows = 0;
    if (int rc = plan(params, 1, rows)) return rc;
    const semidetr_add_norm_mixed &p = params[0];
    const int groups = (int)num_slots(rows);
    hipStream_t st = semidetr::as_stream(stream);
    if (!p.grad_weight && !p.grad_bias) {
        hipLaunchKernelGGL((add_norm_bwd_kernel<kTyped, false>), dim3(groups), dim3(kThreads), 0, st, p, rows, nullptr);
        return semidetr::launch_status("add_norm_bwd_kernel");
    }
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= semidetr_add_norm_workspace_bytes(rows),
                     SEMIDETR_E_BADARG, "add_norm backward: workspace null, misaligned or smaller than semidetr_add_norm_workspace_bytes()");
    float *slots = static_cast<float *>(workspace);
    hipLaunchKernelGGL((add_norm_bwd_kernel<kTyped, true>), dim3(groups), dim3(kThreads), 0, st, p, rows, slots);
    if (int rc = semidetr::launch_status("add_norm_bwd_kernel")) return rc;
    hipLaunchKernelGGL(add_norm_param_kernel, dim3(kSlot / 64), dim3(64 * kParts), 0, st, slots, groups, p.grad_weight, p.grad_bias);
    return semidetr::launch_status("add_norm_param_kernel");
}

}  // namespace

extern "C" size_t semidetr_add_norm_workspace_bytes(int64_t rows)
{
    if (rows < 1 || rows >= ((int64_t)1 << 31)) return 0;
    return (size_t)num_slots(rows) * kSlot * sizeof(float);
}

// The forward needs no workspace.
extern "C" int semidetr_add_norm_forward_f32(void *stream, const semidetr_add_norm *params, void *, size_t)
{
    semidetr_add_norm_mixed wide;
    return forward<false>(stream, widen(params, wide));
}

extern "C" int semidetr_add_norm_backward_f32(void *stream, const semidetr_add_norm *params, void *workspace, size_t workspace_bytes)
{
    semidetr_add_norm_mixed wide;
    return backward<false>(stream, widen(params, wide), workspace, workspace_bytes);
}

extern "C" int semidetr_add_norm_forward_mixed(void *stream, const semidetr_add_norm_mixed *params, void *, size_t)
{
    return forward<true>(stream, params);
}

extern "C" int semidetr_add_norm_backward_mixed(void *stream, const semidetr_add_norm_mixed *params, void *workspace,
                                                size_t workspace_bytes)
{
    return backward<true>(stream, params, workspace, workspace_bytes);
}

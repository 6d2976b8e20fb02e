// Mixed-precision multi-scale deformable attention for gfx950 (MI355X, CDNA4): the value map, the output and their two
// gradients are fp16 or bf16; sampling locations, attention weights and their gradients stay fp32; ALL arithmetic is fp32.
//
// What autocast hands MSDeformAttn (detr_od/models/utils/ops/modules/ms_deform_attn.py:113-120, "for amp"): a 16-bit value
// map from value_proj and fp32 locations / weights.  The up-cast route (value.float() -> fp32 op -> .to(dtype)) writes an
// fp32 copy of the map per call, keeps it alive for the backward and rounds grad_value in a further kernel; the op is
// HBM-bound, so these kernels read the 16-bit rows directly and write 16-bit results.
//
// Numerical contract: every result is the fp32 op applied to the EXACTLY up-cast inputs; `out` and
// `grad_value` are then rounded ONCE, to nearest even, into the 16-bit type.  Nothing is accumulated in 16 bits (grad_value is
// summed with fp32 atomics in an fp32 workspace and converted by a last kernel; no packed 16-bit atomics), locations and
// weights are never narrowed, the pixel mapping is msda_geom.h's (the same code msda.hip samples with), and corners outside
// a level are never loaded (bounds-checked buffer loads / exec-masked loads).
//
// Kernels (T16 = __half | __hip_bfloat16):
//  * msda_fwd_h16<T16, SPLIT>       32 channels per head, <= 32 heads, any query set.  The shape of msda_fwd_d32 (msda_fast.h):
//                                   phase 1 turns the tile's samples into LDS records {4 corner byte offsets, 4 weights};
//                                   phase 2 covers one 64-byte value row with 8 lanes x ONE 8-byte buffer load of 4 channels,
//                                   so lane -> channel map and fp32 accumulation order are msda_fwd_d32's (8 lanes x float4).
//  * msda_bwd_h16<T16>              same shapes.  The shape of msda_bwd_d32: 32 lanes per value row (lane = channel), so every
//                                   global_atomic_add_f32 wave-instruction updates two complete 128-byte workspace rows;
//                                   channel sums for grad_attn / grad_loc by DPP inside the half-wave, staged in LDS.
//  * msda_h16_convert<T16>          fp32 workspace -> 16-bit grad_value, 8 elements (one 16-byte store) per thread.
//  * msda_{fwd,bwd}_h16_generic<T16> any D, any head count, any alignment: one wavefront per (n, q, m) row, lane per channel.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "common.h"

namespace semidetr_h16 {

#include "msda_geom.h"

constexpr int kD = 32;              // channels per head of the fast path
constexpr int kMaxLevels = 32;
thread_local const char *g_last_kernels = "";

#include "cvt16.h"                   // the two storage types: Cvt<T16>, unpack4, pack2, ld16, st16

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
// Sum over the 32 lanes of each wavefront half (the reduction of msda_bwd_d32, msda_fast.h half32_sum): lanes 16..31 of each
// half hold the half's total afterwards; the writer is lane 16 / 48.
__device__ __forceinline__ float half32_sum(float x)
{
    x += dpp_mov<0xB1>(x);    // quad_perm [1,0,3,2]
    x += dpp_mov<0x4E>(x);    // quad_perm [2,3,0,1]
    x += dpp_mov<0x141>(x);   // row_half_mirror
    x += dpp_mov<0x140>(x);   // row_mirror
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x142, 0xA, 0xF, true));   // row_bcast:15
    return x;
}
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// Workgroup -> (image, first query row, head): consecutive workgroups take consecutive heads and the head of a slot is rotated
// every 64 tiles, so that no XCD stays with one address class of the value map (measured on the fp32 kernels: msda_fast.h,
// tile_of).  Speed only -- any bijection is correct.
struct Tile {
    int n, q0, m;
};
__device__ __forceinline__ Tile tile_of_block(int M, int tiles_per_image, int rows_per_block)
{
    Tile t;
    const int b = (int)blockIdx.x, r = b / M;
    t.m = (b % M + r / 64) % M;
    t.q0 = (r % tiles_per_image) * rows_per_block;
    t.n = r / tiles_per_image;
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward, D == 32.  SPLIT = number of 8-lane groups that share one query row (each takes samples part, part + SPLIT, ...):
// small query sets still fill the chip.  LDS: (32 / SPLIT) x (L * P + 1) records of 32 bytes.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T16, int SPLIT>
__global__ __launch_bounds__(256) void msda_fwd_h16(const T16 *__restrict__ value, const int64_t *__restrict__ shapes,
                                                    const int64_t *__restrict__ starts, const float *__restrict__ loc,
                                                    const float *__restrict__ attn, int S, int M, int L, int Lq, int P,
                                                    int tiles_per_image, T16 *__restrict__ out)
{
    constexpr int RPB = 32 / SPLIT;
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1;      // +1 record of padding: rows land on different LDS banks
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_w = smem + RPB * LPP;
    const Tile t = tile_of_block(M, tiles_per_image, RPB);
    const unsigned row_bytes = (unsigned)(M * kD) * 2u;

    // ---- phase 1: sample records
    for (int s = threadIdx.x; s < RPB * LP; s += 256) {
        const int r = s / LP, k = s - r * LP;
        const int q = t.q0 + r;
        unsigned off[4] = {kOob, kOob, kOob, kOob};      // out of range -> the hardware returns zeros
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < Lq) {
            const int l = k / P;
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
            const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
            const float2 xy = *reinterpret_cast<const float2 *>(loc + (row * LP + k) * 2);
            const float a = attn[row * LP + k];
            float lw, lh;
            if (sample_setup_oob(xy.x, xy.y, H, W, st, row_bytes, off, lw, lh)) {
                const float hh = 1.f - lh, hw = 1.f - lw;
                w = make_float4(a * (hh * hw), a * (hh * lw), a * (lh * hw), a * (lh * lw));
            }
        }
        rec_off[r * LPP + k] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
        rec_w[r * LPP + k] = w;
    }
    __syncthreads();

    // ---- phase 2: gather + weighted sum in fp32
    const int g = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int r = g / SPLIT, part = g % SPLIT;
    const int q = t.q0 + r;
    // value slice of image n as a raw buffer of exactly S * M * D * 2 bytes: kOob (invalid corners) reads as zero
    const __amdgpu_buffer_rsrc_t vr = image_rsrc(reinterpret_cast<const float *>(value + (int64_t)t.n * S * M * kD),
                                                 (unsigned)S * M * kD * 2u);
    const unsigned lane_b = (unsigned)(t.m * kD + 4 * j) * 2u;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int4 *ro = rec_off + r * LPP;
    const float4 *rw = rec_w + r * LPP;
#pragma unroll 4
    for (int k = part; k < LP; k += SPLIT) {
        const int4 o = ro[k];
        const float4 w = rw[k];
        const float4 v1 = unpack4<T16>(buf_ld2(vr, (unsigned)o.x + lane_b)), v2 = unpack4<T16>(buf_ld2(vr, (unsigned)o.y + lane_b));
        const float4 v3 = unpack4<T16>(buf_ld2(vr, (unsigned)o.z + lane_b)), v4 = unpack4<T16>(buf_ld2(vr, (unsigned)o.w + lane_b));
        acc.x += w.x * v1.x + w.y * v2.x + w.z * v3.x + w.w * v4.x;
        acc.y += w.x * v1.y + w.y * v2.y + w.z * v3.y + w.w * v4.y;
        acc.z += w.x * v1.z + w.y * v2.z + w.z * v3.z + w.w * v4.z;
        acc.w += w.x * v1.w + w.y * v2.w + w.z * v3.w + w.w * v4.w;
    }
    if (SPLIT > 1) {
#pragma unroll
        for (int s = 8; s < 8 * SPLIT; s <<= 1) {
            acc.x += __shfl_xor(acc.x, s, 64);
            acc.y += __shfl_xor(acc.y, s, 64);
            acc.z += __shfl_xor(acc.z, s, 64);
            acc.w += __shfl_xor(acc.w, s, 64);
        }
    }
    if (part == 0 && q < Lq) {      // every row is written, a row without a sample on the map as zeros (`out` is not pre-cleared)
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        u32x2 pk;
        pk.x = pack2<T16>(acc.x, acc.y);
        pk.y = pack2<T16>(acc.z, acc.w);
        __builtin_nontemporal_store(pk, reinterpret_cast<u32x2 *>(out + row * kD + 4 * j));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward, D == 32: rpb query rows per 256-thread workgroup (8 half-waves, each walks rpb / 8 rows), lane = channel.
// grad_value contributions go into the fp32 workspace `gws` (N * S * M * D floats, zero on entry) with fp32 atomics.
// LDS: rpb x (L * P + 1) x 2 records of 16 bytes + the level table.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T16>
__global__ __launch_bounds__(256) void msda_bwd_h16(const T16 *__restrict__ gout, const T16 *__restrict__ value,
                                                    const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                    const float *__restrict__ loc, const float *__restrict__ attn, int S, int M,
                                                    int L, int Lq, int P, int tiles_per_image, int rpb, float *__restrict__ gws,
                                                    float *__restrict__ gloc, float *__restrict__ gattn)
{
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1;
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_p = smem + rpb * LPP;      // {lw, lh, a, level}; overwritten with {g_attn, g_x, g_y, -}
    float *lev_w = reinterpret_cast<float *>(smem + 2 * rpb * LPP), *lev_h = lev_w + kMaxLevels;
    const Tile t = tile_of_block(M, tiles_per_image, rpb);
    const unsigned row_bytes = (unsigned)(M * kD) * 2u;
    if (threadIdx.x < L) {
        lev_h[threadIdx.x] = (float)shapes[2 * threadIdx.x];
        lev_w[threadIdx.x] = (float)shapes[2 * threadIdx.x + 1];
    }
    for (int s = threadIdx.x; s < rpb * LP; s += 256) {
        const int r = s / LP, k = s - r * LP;
        const int q = t.q0 + r;
        unsigned off[4] = {kOob, kOob, kOob, kOob};
        const int l = k / P;
        float4 pr = make_float4(0.f, 0.f, 0.f, __int_as_float(l));
        if (q < Lq) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
            const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
            const float2 xy = *reinterpret_cast<const float2 *>(loc + (row * LP + k) * 2);
            pr.z = attn[row * LP + k];
            float lw, lh;
            if (sample_setup_oob(xy.x, xy.y, H, W, st, row_bytes, off, lw, lh)) {
                pr.x = lw;
                pr.y = lh;
            }
        }
        rec_off[r * LPP + k] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
        rec_p[r * LPP + k] = pr;
    }
    __syncthreads();

    const int hw = threadIdx.x >> 5, c = threadIdx.x & 31;      // half-wave index, channel
    const __amdgpu_buffer_rsrc_t vr = image_rsrc(reinterpret_cast<const float *>(value + (int64_t)t.n * S * M * kD),
                                                 (unsigned)S * M * kD * 2u);
    const unsigned lane_b = (unsigned)(t.m * kD + c) * 2u;
    float *gvb = gws + (int64_t)t.n * S * M * kD + t.m * kD + c;      // + corner byte offset / 2
    for (int r = hw; r < rpb; r += 8) {
        const int q = t.q0 + r;
        if (q >= Lq) break;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        const float go = ld16(gout + row * kD + c);
        const int4 *ro = rec_off + r * LPP;
        float4 *rp = rec_p + r * LPP;
#pragma unroll 4
        for (int k = 0; k < LP; ++k) {
            const int4 o = ro[k];
            const float4 pr = rp[k];
            const float lw = pr.x, lh = pr.y, a = pr.z;
            const int l = __float_as_int(pr.w);
            const float hh = 1.f - lh, hwt = 1.f - lw;
            const float ga = go * a;
            // d_i = grad_out[c] * v_i[c]; corners outside the level read as zero (buffer bounds check)
            const float d1 = go * Cvt<T16>::up((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(vr, (unsigned)o.x + lane_b, 0, 0));
            const float d2 = go * Cvt<T16>::up((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(vr, (unsigned)o.y + lane_b, 0, 0));
            const float d3 = go * Cvt<T16>::up((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(vr, (unsigned)o.z + lane_b, 0, 0));
            const float d4 = go * Cvt<T16>::up((unsigned short)__builtin_amdgcn_raw_buffer_load_b16(vr, (unsigned)o.w + lane_b, 0, 0));
            if ((unsigned)o.x != kOob) unsafeAtomicAdd(gvb + ((unsigned)o.x >> 1), hh * hwt * ga);
            if ((unsigned)o.y != kOob) unsafeAtomicAdd(gvb + ((unsigned)o.y >> 1), hh * lw * ga);
            if ((unsigned)o.z != kOob) unsafeAtomicAdd(gvb + ((unsigned)o.z >> 1), lh * hwt * ga);
            if ((unsigned)o.w != kOob) unsafeAtomicAdd(gvb + ((unsigned)o.w >> 1), lh * lw * ga);
            float pa = hh * hwt * d1 + hh * lw * d2 + lh * hwt * d3 + lh * lw * d4;
            float px = a * (hh * (d2 - d1) + lh * (d4 - d3));
            float py = a * (hwt * (d3 - d1) + lw * (d4 - d2));
            pa = half32_sum(pa);
            px = half32_sum(px);
            py = half32_sum(py);
            if (c == 16) rp[k] = make_float4(pa, lev_w[l] * px, lev_h[l] * py, a);
        }
    }
    __syncthreads();

    // ---- coalesced write-back of grad_attn_weight / grad_sampling_loc (fp32, unrounded)
    for (int s = threadIdx.x; s < rpb * LP; s += 256) {
        const int rr = s / LP, k = s - rr * LP;
        const int qq = t.q0 + rr;
        if (qq >= Lq) continue;
        const int64_t row = ((int64_t)t.n * Lq + qq) * M + t.m;
        const float4 res = rec_p[rr * LPP + k];
        gattn[row * LP + k] = res.x;
        *reinterpret_cast<float2 *>(gloc + (row * LP + k) * 2) = make_float2(res.y, res.z);
    }
}

// fp32 workspace -> 16-bit grad_value: the ONE rounding of grad_value.  VEC: both pointers 16-byte aligned -- two 16-byte
// loads and one 16-byte store per thread; the last (count % 8) elements, and every element otherwise, go one by one.
template <typename T16, bool VEC>
__global__ __launch_bounds__(256) void msda_h16_convert(const float *__restrict__ ws, int64_t count, T16 *__restrict__ dst)
{
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= count) return;
    if (VEC && i + 8 <= count) {
        const float4 a = *reinterpret_cast<const float4 *>(ws + i), b = *reinterpret_cast<const float4 *>(ws + i + 4);
        uint4 pk;
        pk.x = pack2<T16>(a.x, a.y);
        pk.y = pack2<T16>(a.z, a.w);
        pk.z = pack2<T16>(b.x, b.y);
        pk.w = pack2<T16>(b.z, b.w);
        *reinterpret_cast<uint4 *>(dst + i) = pk;
        return;
    }
    const int64_t end = i + 8 < count ? i + 8 : count;
    for (int64_t e = i; e < end; ++e) st16(dst + e, ws[e]);
}

// ---------------------------------------------------------------------------------------------------------------------
// generic path: one wavefront per (n, q, m) row, lanes stride the channels (msda_{fwd,bwd}_generic of msda.hip with a
// 16-bit value map): any D, any head count, a value pointer on any 2-byte boundary.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T16>
__global__ __launch_bounds__(256) void msda_fwd_h16_generic(const T16 *__restrict__ value, const int64_t *__restrict__ shapes,
                                                            const int64_t *__restrict__ starts, const float *__restrict__ loc,
                                                            const float *__restrict__ attn, int N, int S, int M, int D, int L,
                                                            int Lq, int P, T16 *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)N * Lq * M) return;
    const int m = (int)(row % M);
    const int n = (int)(row / ((int64_t)M * Lq));
    const T16 *vb = value + ((int64_t)n * S * M + m) * D;
    const float *lrow = loc + row * L * P * 2;
    const float *arow = attn + row * L * P;
    const int rs = M * D;
    for (int c0 = 0; c0 < D; c0 += 64) {
        const int c = c0 + lane;
        const bool act = c < D;
        float acc = 0.f;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
            for (int p = 0; p < P; ++p) {
                int off[4];
                float lw, lh;
                const float x = lrow[(l * P + p) * 2], y = lrow[(l * P + p) * 2 + 1];
                if (!sample_setup(x, y, H, W, st, rs, off, lw, lh)) continue;
                const float a = arow[l * P + p];
                const float hh = 1.f - lh, hw = 1.f - lw;
                if (act) {
                    const float v1 = off[0] >= 0 ? ld16(vb + off[0] + c) : 0.f;
                    const float v2 = off[1] >= 0 ? ld16(vb + off[1] + c) : 0.f;
                    const float v3 = off[2] >= 0 ? ld16(vb + off[2] + c) : 0.f;
                    const float v4 = off[3] >= 0 ? ld16(vb + off[3] + c) : 0.f;
                    acc += a * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4);
                }
            }
        }
        if (act) st16(out + row * D + c, acc);
    }
}

template <typename T16>
__global__ __launch_bounds__(256) void msda_bwd_h16_generic(const T16 *__restrict__ gout, const T16 *__restrict__ value,
                                                            const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                            const float *__restrict__ loc, const float *__restrict__ attn, int N,
                                                            int S, int M, int D, int L, int Lq, int P, float *__restrict__ gws,
                                                            float *__restrict__ gloc, float *__restrict__ gattn)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (int64_t)N * Lq * M) return;
    const int m = (int)(row % M);
    const int n = (int)(row / ((int64_t)M * Lq));
    const int64_t vo = ((int64_t)n * S * M + m) * D;
    const T16 *vb = value + vo;
    float *gvb = gws + vo;
    const float *lrow = loc + row * L * P * 2;
    const float *arow = attn + row * L * P;
    const T16 *grow = gout + row * D;
    const int rs = M * D;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
        for (int p = 0; p < P; ++p) {
            int off[4];
            float lw, lh;
            const float x = lrow[(l * P + p) * 2], y = lrow[(l * P + p) * 2 + 1];
            const bool inside = sample_setup(x, y, H, W, st, rs, off, lw, lh);
            float s_attn = 0.f, s_x = 0.f, s_y = 0.f;
            if (inside) {
                const float a = arow[l * P + p];
                const float hh = 1.f - lh, hw = 1.f - lw;
                const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
                for (int c = lane; c < D; c += 64) {
                    const float g = ld16(grow + c), ga = g * a;
                    float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
                    if (off[0] >= 0) { v1 = ld16(vb + off[0] + c); unsafeAtomicAdd(gvb + off[0] + c, w1 * ga); }
                    if (off[1] >= 0) { v2 = ld16(vb + off[1] + c); unsafeAtomicAdd(gvb + off[1] + c, w2 * ga); }
                    if (off[2] >= 0) { v3 = ld16(vb + off[2] + c); unsafeAtomicAdd(gvb + off[2] + c, w3 * ga); }
                    if (off[3] >= 0) { v4 = ld16(vb + off[3] + c); unsafeAtomicAdd(gvb + off[3] + c, w4 * ga); }
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
                gloc[2 * k] = (float)W * s_x;
                gloc[2 * k + 1] = (float)H * s_y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
int check_common(const void *value, const void *shapes, const void *starts, const void *loc, const void *attn, int dtype, int N,
                 int S, int M, int D, int L, int Lq, int P)
{
    SEMIDETR_REQUIRE(value && shapes && starts && loc && attn, SEMIDETR_E_BADARG, "msda_h16: null pointer argument");
    SEMIDETR_REQUIRE(dtype == SEMIDETR_H16_FP16 || dtype == SEMIDETR_H16_BF16, SEMIDETR_E_BADARG,
                     "msda_h16: dtype must be SEMIDETR_H16_FP16 (0) or SEMIDETR_H16_BF16 (1), got %d", dtype);
    SEMIDETR_REQUIRE(N > 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq > 0 && P > 0, SEMIDETR_E_BADARG,
                     "msda_h16: sizes must be positive (N=%d S=%d M=%d D=%d L=%d Lq=%d P=%d)", N, S, M, D, L, Lq, P);
    SEMIDETR_REQUIRE(((uintptr_t)value & 1) == 0, SEMIDETR_E_BADARG, "msda_h16: value must be 2-byte aligned");
    // device index arithmetic inside one image is 32-bit, as in the fp32 op (msda.hip check_common)
    SEMIDETR_REQUIRE((int64_t)(S + 1) * M * D < INT32_MAX, SEMIDETR_E_TOOLARGE,
                     "msda_h16: spatial_size*num_heads*channels = %lld exceeds 32-bit indexing", (long long)S * M * D);
    SEMIDETR_REQUIRE((int64_t)N * Lq * M < INT32_MAX / 4, SEMIDETR_E_TOOLARGE, "msda_h16: too many (n,q,m) rows");
    return SEMIDETR_OK;
}

// fast path: 32 channels, <= 32 heads (kOob + in-row offset must stay out of range: M * 64 bytes < the 4096-byte guard band),
// 8-byte aligned rows, an image slice below the buffer instructions' 32-bit byte range, records of 8 rows within 64 KB of LDS
bool fast_ok(const void *a, const void *b, const void *c, int S, int M, int D, int L, int P)
{
    const uintptr_t al = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c;
    return D == kD && M <= 32 && L <= kMaxLevels && (al & 7) == 0 && (int64_t)L * P <= 254 &&
           (int64_t)S * M * kD * 2 < (int64_t)0xFFFFF000u;
}

int pick_split(int N, int Lq, int M)      // as the fp32 forward (msda_dispatch.h pick_split): small query sets spread a row over more lanes
{
    const int64_t wg32 = (int64_t)N * M * ((Lq + 31) / 32);
    return wg32 >= 2048 ? 1 : (wg32 >= 1024 ? 2 : 4);
}

template <typename T16>
int forward_impl(hipStream_t st, const T16 *value, const int64_t *shapes, const int64_t *starts, const float *loc, const float *attn,
                 int N, int S, int M, int D, int L, int Lq, int P, T16 *out)
{
    if (!fast_ok(value, out, loc, S, M, D, L, P)) {
        const int64_t rows = (int64_t)N * Lq * M;
        hipLaunchKernelGGL(msda_fwd_h16_generic<T16>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, value, shapes, starts, loc,
                           attn, N, S, M, D, L, Lq, P, out);
        g_last_kernels = "msda_fwd_h16_generic";
        return semidetr::launch_status("msda_fwd_h16_generic");
    }
    int split = pick_split(N, Lq, M);
    while (split < 4 && (size_t)(32 / split) * (L * P + 1) * 32 > 64 * 1024) split *= 2;      // wide rows: fewer per workgroup
    const int rpb = 32 / split;
    const int tiles = (Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)N * tiles * M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_forward_h16: grid too large");
    const size_t lds = (size_t)rpb * (L * P + 1) * 32;
    const dim3 grid((unsigned)((int64_t)N * tiles * M));
    if (split == 1)
        hipLaunchKernelGGL((msda_fwd_h16<T16, 1>), grid, dim3(256), lds, st, value, shapes, starts, loc, attn, S, M, L, Lq, P, tiles, out);
    else if (split == 2)
        hipLaunchKernelGGL((msda_fwd_h16<T16, 2>), grid, dim3(256), lds, st, value, shapes, starts, loc, attn, S, M, L, Lq, P, tiles, out);
    else
        hipLaunchKernelGGL((msda_fwd_h16<T16, 4>), grid, dim3(256), lds, st, value, shapes, starts, loc, attn, S, M, L, Lq, P, tiles, out);
    g_last_kernels = split == 1 ? "msda_fwd_h16<1" : (split == 2 ? "msda_fwd_h16<2" : "msda_fwd_h16<4");
    return semidetr::launch_status("msda_fwd_h16");
}

template <typename T16>
int backward_impl(hipStream_t st, const T16 *gout, const T16 *value, const int64_t *shapes, const int64_t *starts, const float *loc,
                  const float *attn, int N, int S, int M, int D, int L, int Lq, int P, float *ws, T16 *gvalue, float *gloc,
                  float *gattn)
{
    const int64_t count = (int64_t)N * S * M * D;
    const char *name;
    if (!fast_ok(value, gout, loc, S, M, D, L, P) || (((uintptr_t)gloc) & 7) != 0) {
        const int64_t rows = (int64_t)N * Lq * M;
        hipLaunchKernelGGL(msda_bwd_h16_generic<T16>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, gout, value, shapes, starts,
                           loc, attn, N, S, M, D, L, Lq, P, ws, gloc, gattn);
        name = "msda_bwd_h16_generic+msda_h16_convert";
    } else {
        // 32 query rows per workgroup, 8 when that would not fill the chip or 32 rows of records would not fit 64 KB of LDS
        const int rpb = ((int64_t)N * M * ((Lq + 31) / 32) >= 1024 &&
                         (size_t)32 * (L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float) <= 64 * 1024) ? 32 : 8;
        const int tiles = (Lq + rpb - 1) / rpb;
        SEMIDETR_REQUIRE((int64_t)N * tiles * M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward_h16: grid too large");
        const size_t lds = (size_t)rpb * (L * P + 1) * 32 + 2 * kMaxLevels * sizeof(float);
        if (int rc = semidetr::allow_big_lds(&msda_bwd_h16<T16>, lds, "msda_backward_h16")) return rc;      // only L * P = 254 at 8 rows
        hipLaunchKernelGGL(msda_bwd_h16<T16>, dim3((unsigned)((int64_t)N * tiles * M)), dim3(256), lds, st, gout, value, shapes, starts,
                           loc, attn, S, M, L, Lq, P, tiles, rpb, ws, gloc, gattn);
        name = "msda_bwd_h16+msda_h16_convert";
    }
    if (int rc = semidetr::launch_status(name)) return rc;
    const int64_t blocks = (count + 2047) / 2048;
    SEMIDETR_REQUIRE(blocks < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_backward_h16: grad_value too large");
    if ((((uintptr_t)ws | (uintptr_t)gvalue) & 15) == 0)
        hipLaunchKernelGGL((msda_h16_convert<T16, true>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    else
        hipLaunchKernelGGL((msda_h16_convert<T16, false>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    g_last_kernels = name;
    return semidetr::launch_status("msda_h16_convert");
}

}  // namespace semidetr_h16

extern "C" const char *semidetr_msda_h16_last_kernels(void) { return semidetr_h16::g_last_kernels; }

extern "C" size_t semidetr_msda_backward_h16_workspace_bytes(int batch, int spatial_size, int num_heads, int channels)
{
    if (batch <= 0 || spatial_size <= 0 || num_heads <= 0 || channels <= 0) return 0;
    return sizeof(float) * (size_t)batch * (size_t)spatial_size * (size_t)num_heads * (size_t)channels;
}

extern "C" int semidetr_msda_forward_h16(void *stream, int dtype, const void *value, const int64_t *spatial_shapes,
                                         const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                                         int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query,
                                         int num_point, void *out)
{
    using namespace semidetr_h16;
    if (int rc = check_common(value, spatial_shapes, level_start, sampling_loc, attn_weight, dtype, batch, spatial_size, num_heads,
                              channels, num_levels, num_query, num_point))
        return rc;
    SEMIDETR_REQUIRE(out && ((uintptr_t)out & 1) == 0, SEMIDETR_E_BADARG, "msda_forward_h16: null or odd output pointer");
    const hipStream_t st = semidetr::as_stream(stream);
    if (dtype == SEMIDETR_H16_FP16)
        return forward_impl<__half>(st, static_cast<const __half *>(value), spatial_shapes, level_start, sampling_loc, attn_weight,
                                    batch, spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                    static_cast<__half *>(out));
    return forward_impl<__hip_bfloat16>(st, static_cast<const __hip_bfloat16 *>(value), spatial_shapes, level_start, sampling_loc,
                                        attn_weight, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point,
                                        static_cast<__hip_bfloat16 *>(out));
}

extern "C" int semidetr_msda_backward_h16(void *stream, int dtype, const void *grad_out, const void *value,
                                          const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                                          const float *attn_weight, int batch, int spatial_size, int num_heads, int channels,
                                          int num_levels, int num_query, int num_point, void *workspace, void *grad_value,
                                          float *grad_sampling_loc, float *grad_attn_weight)
{
    using namespace semidetr_h16;
    if (int rc = check_common(value, spatial_shapes, level_start, sampling_loc, attn_weight, dtype, batch, spatial_size, num_heads,
                              channels, num_levels, num_query, num_point))
        return rc;
    SEMIDETR_REQUIRE(grad_out && workspace && grad_value && grad_sampling_loc && grad_attn_weight, SEMIDETR_E_BADARG,
                     "msda_backward_h16: null pointer argument");
    SEMIDETR_REQUIRE((((uintptr_t)grad_out | (uintptr_t)grad_value) & 1) == 0 && ((uintptr_t)workspace & 3) == 0, SEMIDETR_E_BADARG,
                     "msda_backward_h16: grad_out / grad_value must be 2-byte aligned, workspace 4-byte aligned");
    const hipStream_t st = semidetr::as_stream(stream);
    if (dtype == SEMIDETR_H16_FP16)
        return backward_impl<__half>(st, static_cast<const __half *>(grad_out), static_cast<const __half *>(value), spatial_shapes,
                                     level_start, sampling_loc, attn_weight, batch, spatial_size, num_heads, channels, num_levels,
                                     num_query, num_point, static_cast<float *>(workspace), static_cast<__half *>(grad_value),
                                     grad_sampling_loc, grad_attn_weight);
    return backward_impl<__hip_bfloat16>(st, static_cast<const __hip_bfloat16 *>(grad_out), static_cast<const __hip_bfloat16 *>(value),
                                         spatial_shapes, level_start, sampling_loc, attn_weight, batch, spatial_size, num_heads,
                                         channels, num_levels, num_query, num_point, static_cast<float *>(workspace),
                                         static_cast<__hip_bfloat16 *>(grad_value), grad_sampling_loc, grad_attn_weight);
}

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
//  * msda_fwd_h16_fused<T16, PT, SPLIT>, msda_bwd_h16_fused<T16, PT>: the two fast kernels with the MSDeformAttn prologue / epilogue
//                                   inside (semidetr_msda_fused_{forward,backward}_h16): the sample records come from the fp32
//                                   reference points, the RAW offsets and logits (PT = float | T16) and the padding mask bytes;
//                                   softmax over L * P and ref + off * scale (msda_geom.h fused_loc_xy, the fp32 kernels' code) in
//                                   fp32; the backward's write-back applies the softmax backward and the offset scale and rounds a
//                                   16-bit PT once.  The gather / row phases are the SAME device functions as the unfused kernels'.
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

// Phase 2 of the D == 32 forwards (msda_fwd_h16, msda_fwd_h16_fused): gather + weighted sum in fp32 from the tile's LDS records,
// one 8-byte non-temporal store per lane.
template <typename T16, int SPLIT>
__device__ __forceinline__ void fwd_gather_store(const T16 *__restrict__ value, const int4 *rec_off, const float4 *rec_w, const Tile t,
                                                 int S, int M, int LP, int LPP, int Lq, T16 *__restrict__ out)
{
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
    fwd_gather_store<T16, SPLIT>(value, rec_off, rec_w, t, S, M, LP, LPP, Lq, out);
}

// Row phase of the D == 32 backwards (msda_bwd_h16, msda_bwd_h16_fused): each half-wave walks its rows' LDS records {corner
// offsets} / {lw, lh, a, level}: fp32 atomics into the workspace, and the record overwritten with {g_attn, g_x, g_y, a}.
template <typename T16>
__device__ __forceinline__ void bwd_rows(const T16 *__restrict__ gout, const T16 *__restrict__ value, const int4 *rec_off,
                                         float4 *rec_p, const float *lev_w, const float *lev_h, const Tile t, int S, int M, int LP,
                                         int LPP, int Lq, int rpb, float *__restrict__ gws)
{
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

    bwd_rows<T16>(gout, value, rec_off, rec_p, lev_w, lev_h, t, S, M, LP, LPP, Lq, rpb, gws);
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
// Fused prologue / epilogue on a 16-bit value map: the kernels above with the sample records built from the
// fp32 reference points, the RAW sampling offsets and the RAW attention logits, and the padding mask as bytes -- what RawIO
// (msda_fast.h) is to the fp32 kernels.  Offsets, logits and their gradients are PT = float or T16 (the C ABI's prologue_type);
// the softmax, the locations and every sum are fp32.
// ---------------------------------------------------------------------------------------------------------------------
template <typename PT>
struct Prologue {
    const float *ref;               // (N, Lq, L, ref_dim), fp32 always: locations are never narrowed
    const PT *off, *logit;          // (N, Lq, M, L, P, 2), (N, Lq, M, L * P)
    const unsigned char *mask;      // (N, S) bytes, nonzero = padded pixel, or null
    int ref_dim;
};
// element access of the raw operands: a 16-bit offset pair is one dword (x in the low half)
template <typename PT>
struct RawOp {
    static __device__ __forceinline__ float2 ld_off(const PT *p, int64_t i)
    {
        const unsigned b = *reinterpret_cast<const unsigned *>(p + 2 * i);
        return make_float2(Cvt<PT>::up(b & 0xffffu), Cvt<PT>::up(b >> 16));
    }
    static __device__ __forceinline__ float ld_logit(const PT *p, int64_t i) { return ld16(p + i); }
    static __device__ __forceinline__ void st_off(PT *p, int64_t i, float2 v) { *reinterpret_cast<unsigned *>(p + 2 * i) = pack2<PT>(v.x, v.y); }
    static __device__ __forceinline__ void st_logit(PT *p, int64_t i, float v) { st16(p + i, v); }
};
template <>
struct RawOp<float> {
    static __device__ __forceinline__ float2 ld_off(const float *p, int64_t i) { return *reinterpret_cast<const float2 *>(p + 2 * i); }
    static __device__ __forceinline__ float ld_logit(const float *p, int64_t i) { return p[i]; }
    static __device__ __forceinline__ void st_off(float *p, int64_t i, float2 v) { *reinterpret_cast<float2 *>(p + 2 * i) = v; }
    static __device__ __forceinline__ void st_logit(float *p, int64_t i, float v) { p[i] = v; }
};

// Reductions over a lane-aligned group of LP threads, LP a power of two <= 64 (msda_fast.h lp_group_max / lp_group_sum: DPP inside
// a 16-lane row, shuffles beyond); every lane of the group gets the result.
__device__ __forceinline__ bool lp_shuffles(int LP) { return (LP & (LP - 1)) == 0 && LP <= 64; }
__device__ __forceinline__ float lp_group_sum(float x, int LP)
{
    if (LP >= 2) x += dpp_mov<0xB1>(x);
    if (LP >= 4) x += dpp_mov<0x4E>(x);
    if (LP >= 8) x += dpp_mov<0x141>(x);
    if (LP >= 16) x += dpp_mov<0x140>(x);
    if (LP >= 32) x += __shfl_xor(x, 16, 64);
    if (LP >= 64) x += __shfl_xor(x, 32, 64);
    return x;
}
__device__ __forceinline__ float lp_group_max(float x, int LP)
{
    if (LP >= 2) x = fmaxf(x, dpp_mov<0xB1>(x));
    if (LP >= 4) x = fmaxf(x, dpp_mov<0x4E>(x));
    if (LP >= 8) x = fmaxf(x, dpp_mov<0x141>(x));
    if (LP >= 16) x = fmaxf(x, dpp_mov<0x140>(x));
    if (LP >= 32) x = fmaxf(x, __shfl_xor(x, 16, 64));
    if (LP >= 64) x = fmaxf(x, __shfl_xor(x, 32, 64));
    return x;
}

// The reference point of (query, level) as {x, y, w, h}: one 8-byte buffer load for a point, two for a box -- branch-free: a
// point's second load is sent out of range and returns zeros.  `rr` covers the image's Lq * L * ref_dim floats.
__device__ __forceinline__ float4 ld_ref(__amdgpu_buffer_rsrc_t rr, int ql, int ref_dim)
{
    const unsigned b = (unsigned)(ql * ref_dim) * 4u;
    const float2 c = buf_ld2(rr, b), wh = buf_ld2(rr, ref_dim == 4 ? b + 8u : kOob);
    return make_float4(c.x, c.y, wh.x, wh.y);
}

// exp(logit - row max) of every sample of the tile into LDS, for an L * P whose rows do not line up with the shuffle groups
// (five levels x four points = 20).  sm: 2 x rows x LP floats; the exponentials are sm[rows * LP + s].  Ends with a barrier.
template <typename PT>
__device__ __forceinline__ void tile_exp_to_lds(const PT *logit, const Tile t, int rows, int M, int LP, int Lq, float *sm)
{
    const int total = rows * LP;
    for (int s = threadIdx.x; s < total; s += 256) {
        const int r = s / LP;
        sm[s] = t.q0 + r < Lq ? RawOp<PT>::ld_logit(logit, (((int64_t)t.n * Lq + t.q0 + r) * M + t.m) * LP + (s - r * LP)) : 0.f;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < total; s += 256) {
        const float *lr = sm + (s / LP) * LP;
        float mx = lr[0];
        for (int j = 1; j < LP; ++j) mx = fmaxf(mx, lr[j]);
        sm[total + s] = __expf(sm[s] - mx);
    }
    __syncthreads();
}

// One sample record of a tile from the raw operands: the softmax weight `a` of the sample (fp32, over the row's L * P logits),
// its location by msda_geom.h's fused_loc_xy, its corners by sample_setup_oob, and a corner on a padded pixel -> kOob (never
// loaded, no gradient).  Called by ALL threads of the workgroup (the softmax reduces across lanes); `in`: the thread has a
// sample slot, `live`: that slot's query row exists.  Returns whether the sample is on the map.
template <typename PT>
__device__ __forceinline__ bool fused_record(const Prologue<PT> &pg, __amdgpu_buffer_rsrc_t rr, const int64_t *__restrict__ shapes,
                                             const int64_t *__restrict__ starts, const float *sm_e, bool in, bool live, int n, int q,
                                             int64_t row, int r, int k, int S, int L, int P, unsigned row_bytes, unsigned (&off)[4],
                                             float &lw, float &lh, float &a)
{
    const int LP = L * P, l = k / P;
    float2 o = make_float2(0.f, 0.f);
    float4 rp = make_float4(0.f, 0.f, 0.f, 0.f);
    float raw = 0.f;
    int H = 1, W = 1, st = 0;
    const bool shuf = lp_shuffles(LP);      // (workgroup-uniform)
    if (live) {
        o = RawOp<PT>::ld_off(pg.off, row * LP + k);
        if (shuf) raw = RawOp<PT>::ld_logit(pg.logit, row * LP + k);
        rp = ld_ref(rr, q * L + l, pg.ref_dim);
        H = (int)shapes[2 * l];
        W = (int)shapes[2 * l + 1];
        st = (int)starts[l];
    }
    if (shuf) {      // __expf / v_rcp_f32 as the fp32 kernels' row_softmax (msda_fast.h)
        const float e = __expf(raw - lp_group_max(raw, LP));
        a = e * fast_rcp(lp_group_sum(e, LP));
    } else {
        float sum = 0.f;
        if (in)
            for (int j = 0; j < LP; ++j) sum += sm_e[r * LP + j];      // fixed order
        a = in ? sm_e[r * LP + k] * fast_rcp(sum) : 0.f;
    }
    off[0] = off[1] = off[2] = off[3] = kOob;
    lw = lh = 0.f;
    if (!live) return false;
    float x, y;
    fused_loc_xy(o, rp, pg.ref_dim, P, H, W, x, y);
    if (!sample_setup_oob(x, y, H, W, st, row_bytes, off, lw, lh)) return false;
    if (pg.mask) {      // (x, y) -> top-left pixel exactly as sample_setup_oob derives it
        const int h0 = (int)floorf(sub_rn(mul_rn(y, (float)H), 0.5f)), w0 = (int)floorf(sub_rn(mul_rn(x, (float)W), 0.5f));
        const int pix = st + h0 * W + w0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = pix + (c & 1) + (c >> 1) * W;
            // (a level table that does not tile [0, S) must not reach past the mask)
            if (off[c] != kOob && ((unsigned)p >= (unsigned)S || pg.mask[(int64_t)n * S + p] != 0)) off[c] = kOob;
        }
    }
    return true;
}

// forward: msda_fwd_h16 with phase 1 from the raw operands.  LDS: the records + 2 x RPB x L * P floats when L * P is no power of two.
template <typename T16, typename PT, int SPLIT>
__global__ __launch_bounds__(256) void msda_fwd_h16_fused(const T16 *__restrict__ value, const int64_t *__restrict__ shapes,
                                                          const int64_t *__restrict__ starts, const Prologue<PT> pg, int S, int M,
                                                          int L, int Lq, int P, int tiles_per_image, T16 *__restrict__ out)
{
    constexpr int RPB = 32 / SPLIT;
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1, total = RPB * LP;
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_w = smem + RPB * LPP;
    float *sm = reinterpret_cast<float *>(smem + 2 * RPB * LPP);
    const Tile t = tile_of_block(M, tiles_per_image, RPB);
    const unsigned row_bytes = (unsigned)(M * kD) * 2u;
    if (!lp_shuffles(LP)) tile_exp_to_lds<PT>(pg.logit, t, RPB, M, LP, Lq, sm);
    const __amdgpu_buffer_rsrc_t rr = image_rsrc(pg.ref + (int64_t)t.n * Lq * L * pg.ref_dim, (unsigned)(Lq * L * pg.ref_dim) * 4u);

    // ---- phase 1: sample records (every thread walks every trip: the softmax reduces across lanes)
    for (int s0 = 0; s0 < total; s0 += 256) {
        const int s = s0 + (int)threadIdx.x;
        const bool in = s < total;
        const int r = in ? s / LP : 0, k = in ? s - r * LP : 0;
        const int q = t.q0 + r;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        unsigned off[4];
        float lw, lh, a;
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (fused_record<PT>(pg, rr, shapes, starts, sm + total, in, in && q < Lq, t.n, q, row, r, k, S, L, P, row_bytes, off, lw, lh, a)) {
            const float hh = 1.f - lh, hw = 1.f - lw;
            w = make_float4(a * (hh * hw), a * (hh * lw), a * (lh * hw), a * (lh * lw));
        }
        if (in) {
            rec_off[r * LPP + k] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
            rec_w[r * LPP + k] = w;
        }
    }
    __syncthreads();

    // ---- phase 2: gather + weighted sum in fp32
    fwd_gather_store<T16, SPLIT>(value, rec_off, rec_w, t, S, M, LP, LPP, Lq, out);
}

// backward: msda_bwd_h16 with the records from the raw operands and the fused epilogue in the write-back: the softmax backward
// grad_logits = a_k (g_k - sum_j a_j g_j) with the row's dot from LDS in a fixed order, grad_offsets = grad_loc * scale; both
// rounded once when PT is 16-bit.  LDS: as msda_bwd_h16 + 2 x rpb x L * P floats when L * P is no power of two.
template <typename T16, typename PT>
__global__ __launch_bounds__(256) void msda_bwd_h16_fused(const T16 *__restrict__ gout, const T16 *__restrict__ value,
                                                          const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                          const Prologue<PT> pg, int S, int M, int L, int Lq, int P,
                                                          int tiles_per_image, int rpb, float *__restrict__ gws, PT *__restrict__ goff,
                                                          PT *__restrict__ glogit)
{
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1, total = rpb * LP;
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_p = smem + rpb * LPP;      // {lw, lh, a, level}; overwritten with {g_attn, g_x, g_y, a}
    float *lev_w = reinterpret_cast<float *>(smem + 2 * rpb * LPP), *lev_h = lev_w + kMaxLevels;
    float *sm = lev_h + kMaxLevels;
    const Tile t = tile_of_block(M, tiles_per_image, rpb);
    const unsigned row_bytes = (unsigned)(M * kD) * 2u;
    if (threadIdx.x < L) {
        lev_h[threadIdx.x] = (float)shapes[2 * threadIdx.x];
        lev_w[threadIdx.x] = (float)shapes[2 * threadIdx.x + 1];
    }
    if (!lp_shuffles(LP)) tile_exp_to_lds<PT>(pg.logit, t, rpb, M, LP, Lq, sm);
    const __amdgpu_buffer_rsrc_t rr = image_rsrc(pg.ref + (int64_t)t.n * Lq * L * pg.ref_dim, (unsigned)(Lq * L * pg.ref_dim) * 4u);
    for (int s0 = 0; s0 < total; s0 += 256) {
        const int s = s0 + (int)threadIdx.x;
        const bool in = s < total;
        const int r = in ? s / LP : 0, k = in ? s - r * LP : 0;
        const int q = t.q0 + r;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        unsigned off[4];
        float lw, lh, a;
        fused_record<PT>(pg, rr, shapes, starts, sm + total, in, in && q < Lq, t.n, q, row, r, k, S, L, P, row_bytes, off, lw, lh, a);
        if (in) {      // `a` is kept for skipped samples too: the softmax backward needs every probability
            rec_off[r * LPP + k] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
            rec_p[r * LPP + k] = make_float4(lw, lh, q < Lq ? a : 0.f, __int_as_float(k / P));
        }
    }
    __syncthreads();

    bwd_rows<T16>(gout, value, rec_off, rec_p, lev_w, lev_h, t, S, M, LP, LPP, Lq, rpb, gws);
    __syncthreads();

    // ---- coalesced write-back of grad_attn_logits / grad_sampling_offsets, each in PT
    for (int s = threadIdx.x; s < total; s += 256) {
        const int r = s / LP, k = s - r * LP;
        const int q = t.q0 + r;
        if (q >= Lq) continue;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        const float4 *rowp = rec_p + r * LPP;
        const float4 res = rowp[k];      // {d/d a_k, d/d loc.x, d/d loc.y, a_k}
        float dot = 0.f;
        for (int j = 0; j < LP; ++j) dot += rowp[j].w * rowp[j].x;
        const int l = k / P;
        const float2 sc = fused_loc_scale(ld_ref(rr, q * L + l, pg.ref_dim), pg.ref_dim, P, (int)lev_h[l], (int)lev_w[l]);
        RawOp<PT>::st_logit(glogit, row * LP + k, res.w * (res.x - dot));
        RawOp<PT>::st_off(goff, row * LP + k, make_float2(res.y * sc.x, res.z * sc.y));
    }
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

// ---- fused prologue / epilogue: the fast kernels or SEMIDETR_E_BADARG (there is no generic fused kernel)
struct FusedArgs {
    const void *value;
    const int64_t *shapes, *starts;
    const float *ref;
    int ref_dim;
    const void *off, *logit;
    int prologue_type;
    const unsigned char *mask;
    int N, S, M, D, L, Lq, P;
};

// LDS of a fused kernel with `rows` query rows: the records (+ the backward's level table) + the softmax rows when L * P is no power of two
size_t fused_lds(int rows, int LP, bool backward)
{
    const bool shuf = (LP & (LP - 1)) == 0;
    return (size_t)rows * (LP + 1) * 32 + (backward ? 2 * kMaxLevels * sizeof(float) : 0) + (shuf ? 0 : (size_t)2 * rows * LP * sizeof(float));
}

int check_fused(const FusedArgs &a, int dtype, const void *io16, const char *what)
{
    if (int rc = check_common(a.value, a.shapes, a.starts, a.off, a.logit, dtype, a.N, a.S, a.M, a.D, a.L, a.Lq, a.P)) return rc;
    SEMIDETR_REQUIRE(a.ref && io16, SEMIDETR_E_BADARG, "%s: null pointer argument", what);
    SEMIDETR_REQUIRE(a.ref_dim == 2 || a.ref_dim == 4, SEMIDETR_E_BADARG, "%s: ref_dim must be 2 or 4, got %d", what, a.ref_dim);
    SEMIDETR_REQUIRE(a.prologue_type == SEMIDETR_ROW_F32 || a.prologue_type == (dtype == SEMIDETR_H16_FP16 ? SEMIDETR_ROW_FP16 : SEMIDETR_ROW_BF16),
                     SEMIDETR_E_BADARG, "%s: prologue_type must be SEMIDETR_ROW_F32 (0) or the 16-bit type of dtype (%s), got %d", what,
                     dtype == SEMIDETR_H16_FP16 ? "SEMIDETR_ROW_FP16 (1)" : "SEMIDETR_ROW_BF16 (2)", a.prologue_type);
    SEMIDETR_REQUIRE(a.D == kD && a.M <= 32, SEMIDETR_E_BADARG,
                     "%s: the fused 16-bit kernels take channels == 32 and num_heads <= 32 (got %d, %d); there is no generic fused kernel",
                     what, a.D, a.M);
    SEMIDETR_REQUIRE(a.L <= kMaxLevels && (int64_t)a.L * a.P <= 64, SEMIDETR_E_BADARG,
                     "%s: num_levels * num_point = %lld exceeds the 64 samples per row the fused 16-bit kernels hold in LDS", what,
                     (long long)a.L * a.P);
    SEMIDETR_REQUIRE((((uintptr_t)a.value | (uintptr_t)io16 | (uintptr_t)a.ref | (uintptr_t)a.off) & 7) == 0 && ((uintptr_t)a.logit & 3) == 0,
                     SEMIDETR_E_BADARG,
                     "%s: value, out / grad_out, reference_points and sampling_offsets must be 8-byte aligned, attn_logits 4-byte aligned",
                     what);
    SEMIDETR_REQUIRE((int64_t)a.S * a.M * kD * 2 < (int64_t)kOob && (int64_t)a.Lq * a.L * a.ref_dim * 4 < (int64_t)kOob, SEMIDETR_E_TOOLARGE,
                     "%s: an image's value slice or reference points exceed the buffer instructions' 32-bit byte range", what);
    return SEMIDETR_OK;
}

template <typename T16, typename PT>
int fused_forward_impl(hipStream_t st, const FusedArgs &a, T16 *out)
{
    const Prologue<PT> pg = {a.ref, static_cast<const PT *>(a.off), static_cast<const PT *>(a.logit), a.mask, a.ref_dim};
    const T16 *value = static_cast<const T16 *>(a.value);
    const int LP = a.L * a.P;
    int split = pick_split(a.N, a.Lq, a.M);
    while (split < 4 && fused_lds(32 / split, LP, false) > 64 * 1024) split *= 2;
    const int rpb = 32 / split;
    const int tiles = (a.Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)a.N * tiles * a.M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_fused_forward_h16: grid too large");
    const size_t lds = fused_lds(rpb, LP, false);
    const dim3 grid((unsigned)((int64_t)a.N * tiles * a.M));
    if (split == 1)
        hipLaunchKernelGGL((msda_fwd_h16_fused<T16, PT, 1>), grid, dim3(256), lds, st, value, a.shapes, a.starts, pg, a.S, a.M, a.L, a.Lq, a.P, tiles, out);
    else if (split == 2)
        hipLaunchKernelGGL((msda_fwd_h16_fused<T16, PT, 2>), grid, dim3(256), lds, st, value, a.shapes, a.starts, pg, a.S, a.M, a.L, a.Lq, a.P, tiles, out);
    else
        hipLaunchKernelGGL((msda_fwd_h16_fused<T16, PT, 4>), grid, dim3(256), lds, st, value, a.shapes, a.starts, pg, a.S, a.M, a.L, a.Lq, a.P, tiles, out);
    g_last_kernels = split == 1 ? "msda_fwd_h16_fused<1" : (split == 2 ? "msda_fwd_h16_fused<2" : "msda_fwd_h16_fused<4");
    return semidetr::launch_status("msda_fwd_h16_fused");
}

template <typename T16, typename PT>
int fused_backward_impl(hipStream_t st, const FusedArgs &a, const T16 *gout, float *ws, T16 *gvalue, void *goff, void *glogit)
{
    const Prologue<PT> pg = {a.ref, static_cast<const PT *>(a.off), static_cast<const PT *>(a.logit), a.mask, a.ref_dim};
    const int LP = a.L * a.P;
    // 32 query rows per workgroup, 8 when that would not fill the chip or 32 rows would not fit 64 KB of LDS (as backward_impl)
    const int rpb = ((int64_t)a.N * a.M * ((a.Lq + 31) / 32) >= 1024 && fused_lds(32, LP, true) <= 64 * 1024) ? 32 : 8;
    const int tiles = (a.Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)a.N * tiles * a.M < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_fused_backward_h16: grid too large");
    hipLaunchKernelGGL((msda_bwd_h16_fused<T16, PT>), dim3((unsigned)((int64_t)a.N * tiles * a.M)), dim3(256), fused_lds(rpb, LP, true), st, gout,
                       static_cast<const T16 *>(a.value), a.shapes, a.starts, pg, a.S, a.M, a.L, a.Lq, a.P, tiles, rpb, ws,
                       static_cast<PT *>(goff), static_cast<PT *>(glogit));
    if (int rc = semidetr::launch_status("msda_bwd_h16_fused")) return rc;
    const int64_t count = (int64_t)a.N * a.S * a.M * a.D;
    const int64_t blocks = (count + 2047) / 2048;
    SEMIDETR_REQUIRE(blocks < INT32_MAX, SEMIDETR_E_TOOLARGE, "msda_fused_backward_h16: grad_value too large");
    if ((((uintptr_t)ws | (uintptr_t)gvalue) & 15) == 0)
        hipLaunchKernelGGL((msda_h16_convert<T16, true>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    else
        hipLaunchKernelGGL((msda_h16_convert<T16, false>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    g_last_kernels = "msda_bwd_h16_fused+msda_h16_convert";
    return semidetr::launch_status("msda_h16_convert");
}

}  // namespace semidetr_h16

extern "C" int semidetr_msda_fused_forward_h16(void *stream, int dtype, const void *value, const int64_t *spatial_shapes,
                                               const int64_t *level_start, const float *reference_points, int ref_dim,
                                               const void *sampling_offsets, const void *attn_logits, int prologue_type,
                                               const unsigned char *padding_mask, int batch, int spatial_size, int num_heads,
                                               int channels, int num_levels, int num_query, int num_point, void *out)
{
    using namespace semidetr_h16;
    const FusedArgs a = {value, spatial_shapes, level_start, reference_points, ref_dim, sampling_offsets, attn_logits, prologue_type,
                         padding_mask, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
    if (int rc = check_fused(a, dtype, out, "msda_fused_forward_h16")) return rc;
    const hipStream_t st = semidetr::as_stream(stream);
    const bool f32 = prologue_type == SEMIDETR_ROW_F32;
    if (dtype == SEMIDETR_H16_FP16)
        return f32 ? fused_forward_impl<__half, float>(st, a, static_cast<__half *>(out))
                   : fused_forward_impl<__half, __half>(st, a, static_cast<__half *>(out));
    return f32 ? fused_forward_impl<__hip_bfloat16, float>(st, a, static_cast<__hip_bfloat16 *>(out))
               : fused_forward_impl<__hip_bfloat16, __hip_bfloat16>(st, a, static_cast<__hip_bfloat16 *>(out));
}

extern "C" int semidetr_msda_fused_backward_h16(void *stream, int dtype, const void *grad_out, const void *value,
                                                const int64_t *spatial_shapes, const int64_t *level_start,
                                                const float *reference_points, int ref_dim, const void *sampling_offsets,
                                                const void *attn_logits, int prologue_type, const unsigned char *padding_mask,
                                                int batch, int spatial_size, int num_heads, int channels, int num_levels,
                                                int num_query, int num_point, void *workspace, void *grad_value,
                                                void *grad_sampling_offsets, void *grad_attn_logits)
{
    using namespace semidetr_h16;
    const FusedArgs a = {value, spatial_shapes, level_start, reference_points, ref_dim, sampling_offsets, attn_logits, prologue_type,
                         padding_mask, batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
    if (int rc = check_fused(a, dtype, grad_out, "msda_fused_backward_h16")) return rc;
    SEMIDETR_REQUIRE(workspace && grad_value && grad_sampling_offsets && grad_attn_logits, SEMIDETR_E_BADARG,
                     "msda_fused_backward_h16: null pointer argument");
    SEMIDETR_REQUIRE(((uintptr_t)grad_value & 1) == 0 && ((uintptr_t)workspace & 3) == 0 && ((uintptr_t)grad_sampling_offsets & 7) == 0 &&
                         ((uintptr_t)grad_attn_logits & 3) == 0,
                     SEMIDETR_E_BADARG,
                     "msda_fused_backward_h16: grad_value must be 2-byte, workspace and grad_attn_logits 4-byte, grad_sampling_offsets "
                     "8-byte aligned");
    const hipStream_t st = semidetr::as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    const bool f32 = prologue_type == SEMIDETR_ROW_F32;
    if (dtype == SEMIDETR_H16_FP16) {
        const __half *go = static_cast<const __half *>(grad_out);
        __half *gv = static_cast<__half *>(grad_value);
        return f32 ? fused_backward_impl<__half, float>(st, a, go, ws, gv, grad_sampling_offsets, grad_attn_logits)
                   : fused_backward_impl<__half, __half>(st, a, go, ws, gv, grad_sampling_offsets, grad_attn_logits);
    }
    const __hip_bfloat16 *go = static_cast<const __hip_bfloat16 *>(grad_out);
    __hip_bfloat16 *gv = static_cast<__hip_bfloat16 *>(grad_value);
    return f32 ? fused_backward_impl<__hip_bfloat16, float>(st, a, go, ws, gv, grad_sampling_offsets, grad_attn_logits)
               : fused_backward_impl<__hip_bfloat16, __hip_bfloat16>(st, a, go, ws, gv, grad_sampling_offsets, grad_attn_logits);
}

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

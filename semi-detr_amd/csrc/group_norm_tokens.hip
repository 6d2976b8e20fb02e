// Input projection for gfx950: GroupNorm(32, 256) of every pyramid level written straight into the (N, S, 256) token tensor, with
// the positional add of encoder layer 0, forward and backward.  Replaces the GroupNorm of nn.Sequential(Conv2d, GroupNorm(32, 256))
// (dino_detr_ssod_head.py:251-259, dino_detr_head.py:223-231), src.flatten(2).transpose(1, 2), torch.cat(src_flatten, 1) and the
// src + pos in front of layer 0 (detr_od/models/utils/transformer.py:1276-1287, 635).  One parameter block with a level table
// (semidetr_gn_tokens) serves every launch; a launch covers the whole pyramid.
//
//   gn_stats_kernel           workgroup = one chunk of kChunk = 8192 consecutive elements of a group (a group is the contiguous
//                             run of 8 planes = 8 * hw elements): 32 elements per thread in registers, sum -> chunk mean -> sum of
//                             squared deviations from it.  Writes (sum, M2) of the chunk.  Level 0 of the bench pyramid has 14
//                             chunks per group, level 3 one: the work per workgroup is the same within a factor of the ragged tail.
//   gn_tokens_fwd_kernel      workgroup = (image, level, tile of kTile = 64 pixels) x 256 channels.  Each wave merges the chunks of
//                             8 groups in fp64 (lane k takes chunks k, k + 64, ..., then a xor butterfly: a fixed order), rounds
//                             mean and rstd once.  Planes are read along pixels (16 / 8 bytes per lane where hw % 4 == 0, else one
//                             element per lane), normalised, stored in the LDS tile [channel][pixel] (leading dimension 65);
//                             then a wave per pixel reads its lane's 4 channels and stores the complete token row (and q = y + pos).
//   gn_tokens_bwd_sums_kernel workgroup = (image, level, unit of kUnit = 128 pixels = 2 tiles).  xhat goes through the tile; each
//                             lane adds, over its wave's pixels in pixel order, g * xhat and g of its 4 channels and g * w and
//                             g * w * xhat; lane pairs form the group sums; the 4 waves combine through LDS in wave order into
//                             one slot (256 dweight | 256 dbias | 32 sum gw | 32 sum gw xhat).
//   gn_tokens_bwd_dx_kernel   workgroup = (image, level, tile).  Merges the group sums of the level's units in fp64 (as above), puts
//                             g * w of the tile's rows into the LDS tile, then walks the planes as the forward does and writes dx.
//   gn_tokens_param_kernel    per level 8 workgroups x 64 columns x 16 parts over the level's slots, fp64, one rounding.
// No float atomics, no memset; every grid, map and order depends on batch, levels and hw[] alone: two runs are bitwise equal.
//
// Arithmetic (tests/input_proj_ref64.py bounds it), every product and sum rounded on its own (contraction off):
//   chunk: s_c = sum x; m_c = s_c / n_c; M2_c = sum (x - m_c)^2.  group: mean = fp32(sum_c s_c / n); M2 = sum_c (M2_c +
//   n_c * (m_c - mean)^2) with m_c - mean rounded to fp32 and the rest in fp64; var = fp32(M2 / n); rstd = 1 / sqrt(var + eps);
//   y = ((x - mean) * rstd) * w + b; q = y + pos.
//   backward: g = gy + gq; xhat = (x - mean) * rstd; gw = g * w; c1 = fp32(sum gw / n); c2 = fp32(sum gw * xhat / n);
//   dx = rstd * ((gw - c1) - xhat * c2).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"

constexpr int kC = 256, kG = 32, kCg = kC / kG;      // channels, groups, channels per group
constexpr int kMaxLevels = SEMIDETR_GN_MAX_LEVELS;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kSlots4 = 8;                           // float4 a thread of the statistics kernel holds
constexpr int kChunk = kThreads * 4 * kSlots4;       // 8192 elements of a group per workgroup
constexpr int kTile = 64, kLd = kTile + 1;           // pixels of a transpose tile; leading dimension of tile[channel][pixel]
constexpr int kUnitTiles = 2, kUnit = kUnitTiles * kTile;      // pixels of one backward slot
constexpr int kSlot = 2 * kC + 2 * kG;               // floats of a slot: dweight | dbias | sum gw | sum gw xhat
constexpr int kParts = 16;
constexpr int kStatLds = 4 * kG;                     // mean | rstd | c1 | c2 behind the tile
constexpr size_t kLdsBytes = (size_t)(kC * kLd + kStatLds) * sizeof(float);
static_assert(kWaves * kSlot <= kC * kLd, "the four waves' slots fit in the tile");

// The grids: level-major, then image, then the part of the level.
struct Plan {
    int cfirst[kMaxLevels + 1], chunks[kMaxLevels];  // statistics: first workgroup (= partial) of a level, chunks per group
    int tfirst[kMaxLevels + 1], tiles[kMaxLevels];   // tiles per image
    int ufirst[kMaxLevels + 1], units[kMaxLevels];   // units (= slots) per image
    int vec[kMaxLevels];                             // planes of the level are walked 4 pixels per lane
};

__device__ __forceinline__ float wave_sum(float v)
{
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double wave_sum64(double v)
{
    #pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the four waves' sums in wave order; every thread gets the same bits
__device__ __forceinline__ float block_sum(float v, float *red, int lane, int wave)
{
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- elements in their type (SEMIDETR_ROW_*): the branch is one scalar branch of the whole wave --------------------------------
__device__ __forceinline__ float4 ld4(const void *base, int type, int64_t i)
{
    if (type == SEMIDETR_ROW_F32) return *reinterpret_cast<const float4 *>(static_cast<const float *>(base) + i);
    const float2 r = *reinterpret_cast<const float2 *>(static_cast<const unsigned short *>(base) + i);
    return type == SEMIDETR_ROW_FP16 ? unpack4<__half>(r) : unpack4<__hip_bfloat16>(r);
}

__device__ __forceinline__ float ld1(const void *base, int type, int64_t i)
{
    if (type == SEMIDETR_ROW_F32) return static_cast<const float *>(base)[i];
    const unsigned bits = static_cast<const unsigned short *>(base)[i];
    return type == SEMIDETR_ROW_FP16 ? Cvt<__half>::up(bits) : Cvt<__hip_bfloat16>::up(bits);
}

__device__ __forceinline__ void st4(void *base, int type, int64_t i, const float4 &v)
{
    if (type == SEMIDETR_ROW_F32) {
        *reinterpret_cast<float4 *>(static_cast<float *>(base) + i) = v;
        return;
    }
    uint2 bits;
    if (type == SEMIDETR_ROW_FP16) bits = make_uint2(pack2<__half>(v.x, v.y), pack2<__half>(v.z, v.w));
    else bits = make_uint2(pack2<__hip_bfloat16>(v.x, v.y), pack2<__hip_bfloat16>(v.z, v.w));
    *reinterpret_cast<uint2 *>(static_cast<unsigned short *>(base) + i) = bits;
}

__device__ __forceinline__ void st1(void *base, int type, int64_t i, float v)
{
    if (type == SEMIDETR_ROW_F32) static_cast<float *>(base)[i] = v;
    else static_cast<unsigned short *>(base)[i] =
        (unsigned short)(type == SEMIDETR_ROW_FP16 ? Cvt<__half>::down(v) : Cvt<__hip_bfloat16>::down(v));
}

// ---- the arithmetic of one element: the only statement of it, contraction off, so the bits do not depend on the path ----------
__device__ __forceinline__ float norm1(float x, float m, float rs, float w, float b)
{
    #pragma clang fp contract(off)
    return ((x - m) * rs) * w + b;
}

__device__ __forceinline__ float xhat1(float x, float m, float rs)
{
    #pragma clang fp contract(off)
    return (x - m) * rs;
}

__device__ __forceinline__ float dx1(float gw, float xh, float rs, float c1, float c2)
{
    #pragma clang fp contract(off)
    return rs * ((gw - c1) - xh * c2);
}

__device__ __forceinline__ float sq4(const float4 &v, float m)
{
    #pragma clang fp contract(off)
    const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
    return (a * a + b * b) + (c * c + d * d);
}

__device__ __forceinline__ float sum4(const float4 &a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(const float4 &a, const float4 &b)
{
    #pragma clang fp contract(off)
    return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

__device__ __forceinline__ int level_of(const int *first, int levels, int block)
{
    int l = 0;
    while (l + 1 < levels && block >= first[l + 1]) ++l;
    return l;
}

// elements of chunk c of a group of `len` elements
__device__ __forceinline__ int chunk_count(int64_t len, int c) { return (int)min((int64_t)kChunk, len - (int64_t)c * kChunk); }

// upstream gradient of the lane's 4 channels of one token row: gy + gq, either may be absent
__device__ __forceinline__ float4 load_g(const semidetr_gn_tokens &p, int n, int64_t row, int lane)
{
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.gy) g = ld4(p.gy, p.out_type, n * p.gy_stride[0] + row * p.gy_stride[1] + 4 * lane);
    if (p.gq) {
        const float4 h = ld4(p.gq, p.out_type, n * p.gq_stride[0] + row * p.gq_stride[1] + 4 * lane);
        g = p.gy ? add4(g, h) : h;
    }
    return g;
}

// ---- 1. statistics -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gn_stats_kernel(const semidetr_gn_tokens p, const Plan pl, float2 *partial)
{
    __shared__ float red[2][kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.cfirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.cfirst[l], C = pl.chunks[l];
    const int ng = r / C, c = r - ng * C, n = ng / kG, g = ng - n * kG;
    const int64_t len = (int64_t)kCg * p.hw[l];
    const int cnt = chunk_count(len, c);             // a multiple of 8
    const int64_t base = (int64_t)n * p.x_batch_stride[l] + g * len + (int64_t)c * kChunk;
    const void *x = p.x[l];
    const int xt = p.x_type;
    float4 v[kSlots4];
    #pragma unroll
    for (int j = 0; j < kSlots4; ++j) {
        const int i = (j * kThreads + t) * 4;
        v[j] = i < cnt ? ld4(x, xt, base + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s = sum4(v[0]);
    #pragma unroll
    for (int j = 1; j < kSlots4; ++j) s += sum4(v[j]);
    s = block_sum(s, red[0], lane, wave);
    const float m = s / (float)cnt;
    float q = 0.f;
    #pragma unroll
    for (int j = 0; j < kSlots4; ++j)
        if ((j * kThreads + t) * 4 < cnt) q += sq4(v[j], m);
    q = block_sum(q, red[1], lane, wave);
    if (t == 0) partial[blockIdx.x] = make_float2(s, q);
}

// mean and rstd of group g of (image n, level l) from its chunks, by one wave; every lane gets the same bits
__device__ __forceinline__ void merge_chunks(const float2 *pc, int C, int64_t len, float eps, int lane, float &mean, float &rstd)
{
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)pc[c].x;
    s = wave_sum64(s);
    mean = (float)(s / (double)len);
    double m2 = 0.0;
    for (int c = lane; c < C; c += 64) {
        const int cnt = chunk_count(len, c);
        const float dm = pc[c].x / (float)cnt - mean;
        m2 += (double)pc[c].y + (double)cnt * ((double)dm * (double)dm);
    }
    m2 = wave_sum64(m2);
    const float var = (float)(m2 / (double)len);
    rstd = 1.0f / sqrtf(var + eps);
}

// ---- 2. normalise + transpose -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gn_tokens_fwd_kernel(const semidetr_gn_tokens p, const Plan pl, const float2 *partial)
{
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    float *tile = gn_smem, *s_mean = gn_smem + kC * kLd, *s_rstd = s_mean + kG;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.tfirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.tfirst[l], T = pl.tiles[l];
    const int n = r / T, p0 = (r - n * T) * kTile;
    const int hw = (int)p.hw[l], npix = min(kTile, hw - p0);
    const int64_t len = (int64_t)kCg * hw;
    for (int j = 0; j < kG / kWaves; ++j) {
        const int g = wave * (kG / kWaves) + j;
        float mean, rstd;
        merge_chunks(partial + pl.cfirst[l] + (int64_t)(n * kG + g) * pl.chunks[l], pl.chunks[l], len, p.eps, lane, mean, rstd);
        if (lane == 0) {
            s_mean[g] = mean;
            s_rstd[g] = rstd;
            if (p0 == 0) {
                p.mean[(n * p.levels + l) * kG + g] = mean;
                p.rstd[(n * p.levels + l) * kG + g] = rstd;
            }
        }
    }
    __syncthreads();
    const void *x = p.x[l];
    const float *w = p.weight[l], *b = p.bias[l];
    const int xt = p.x_type, ot = p.out_type;
    const int64_t xb = (int64_t)n * p.x_batch_stride[l] + p0;
    if (pl.vec[l]) {                                 // hw % 4 == 0: npix is a multiple of 4 and every plane starts aligned
        const int cc = lane >> 4, p4 = (lane & 15) * 4;
        if (p4 < npix) {
            #pragma unroll 4
            for (int i = 0; i < kC / 16; ++i) {
                const int c = i * 16 + wave * 4 + cc;
                const float4 v = ld4(x, xt, xb + (int64_t)c * hw + p4);
                const float m = s_mean[c >> 3], rs = s_rstd[c >> 3], wc = w[c], bc = b[c];
                float *d = tile + c * kLd + p4;
                d[0] = norm1(v.x, m, rs, wc, bc);
                d[1] = norm1(v.y, m, rs, wc, bc);
                d[2] = norm1(v.z, m, rs, wc, bc);
                d[3] = norm1(v.w, m, rs, wc, bc);
            }
        }
    } else if (lane < npix) {
        #pragma unroll 8
        for (int i = 0; i < kC / kWaves; ++i) {
            const int c = i * kWaves + wave;
            const float v = ld1(x, xt, xb + (int64_t)c * hw + lane);
            tile[c * kLd + lane] = norm1(v, s_mean[c >> 3], s_rstd[c >> 3], w[c], b[c]);
        }
    }
    __syncthreads();
    const float *col = tile + 4 * lane * kLd;
    for (int pp = wave; pp < npix; pp += kWaves) {
        const int64_t row = p.start[l] + p0 + pp, out = ((int64_t)n * p.tokens_per_image + row) * kC + 4 * lane;
        const float4 y = make_float4(col[pp], col[kLd + pp], col[2 * kLd + pp], col[3 * kLd + pp]);
        st4(p.tokens, ot, out, y);
        if (p.q) st4(p.q, ot, out, add4(y, ld4(p.pos, p.pos_type, n * p.pos_stride[0] + row * p.pos_stride[1] + 4 * lane)));
    }
}

// ---- 3. backward: sums ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gn_tokens_bwd_sums_kernel(const semidetr_gn_tokens p, const Plan pl, float *slots)
{
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    float *tile = gn_smem, *s_mean = gn_smem + kC * kLd, *s_rstd = s_mean + kG;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.ufirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.ufirst[l], U = pl.units[l];
    const int n = r / U, u0 = (r - n * U) * kUnit;
    const int hw = (int)p.hw[l];
    if (t < kG) {
        s_mean[t] = p.mean[(n * p.levels + l) * kG + t];
        s_rstd[t] = p.rstd[(n * p.levels + l) * kG + t];
    }
    const void *x = p.x[l];
    const int xt = p.x_type;
    const float4 w4 = reinterpret_cast<const float4 *>(p.weight[l])[lane];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dw = zero, db = zero, ga = zero, gb = zero;
    const float *col = tile + 4 * lane * kLd;
    for (int tl = 0; tl < kUnitTiles; ++tl) {
        const int p0 = u0 + tl * kTile;
        if (p0 >= hw) break;                         // the same for the whole workgroup
        const int npix = min(kTile, hw - p0);
        const int64_t xb = (int64_t)n * p.x_batch_stride[l] + p0;
        __syncthreads();                             // the statistics are there; the previous tile has been read
        if (pl.vec[l]) {
            const int cc = lane >> 4, p4 = (lane & 15) * 4;
            if (p4 < npix) {
                #pragma unroll 4
                for (int i = 0; i < kC / 16; ++i) {
                    const int c = i * 16 + wave * 4 + cc;
                    const float4 v = ld4(x, xt, xb + (int64_t)c * hw + p4);
                    const float m = s_mean[c >> 3], rs = s_rstd[c >> 3];
                    float *d = tile + c * kLd + p4;
                    d[0] = xhat1(v.x, m, rs);
                    d[1] = xhat1(v.y, m, rs);
                    d[2] = xhat1(v.z, m, rs);
                    d[3] = xhat1(v.w, m, rs);
                }
            }
        } else if (lane < npix) {
            #pragma unroll 8
            for (int i = 0; i < kC / kWaves; ++i) {
                const int c = i * kWaves + wave;
                tile[c * kLd + lane] = xhat1(ld1(x, xt, xb + (int64_t)c * hw + lane), s_mean[c >> 3], s_rstd[c >> 3]);
            }
        }
        __syncthreads();
        for (int pp = wave; pp < npix; pp += kWaves) {
            const float4 g = load_g(p, n, p.start[l] + p0 + pp, lane);
            const float4 xh = make_float4(col[pp], col[kLd + pp], col[2 * kLd + pp], col[3 * kLd + pp]);
            const float4 gw = mul4(g, w4);
            dw = add4(dw, mul4(g, xh));
            db = add4(db, g);
            ga = add4(ga, gw);
            gb = add4(gb, mul4(gw, xh));
        }
    }
    float a = sum4(ga), bsum = sum4(gb);             // 4 of the group's 8 channels; the lane pair holds the other 4
    a += __shfl_xor(a, 1);
    bsum += __shfl_xor(bsum, 1);
    __syncthreads();                                 // the tile becomes the four waves' slots
    float *part = tile + wave * kSlot;
    reinterpret_cast<float4 *>(part)[lane] = dw;
    reinterpret_cast<float4 *>(part + kC)[lane] = db;
    if ((lane & 1) == 0) {
        part[2 * kC + (lane >> 1)] = a;
        part[2 * kC + kG + (lane >> 1)] = bsum;
    }
    __syncthreads();
    for (int c = t; c < kSlot; c += kThreads) {
        float acc = tile[c];
        #pragma unroll
        for (int k = 1; k < kWaves; ++k) acc += tile[k * kSlot + c];
        slots[(int64_t)blockIdx.x * kSlot + c] = acc;
    }
}

// ---- 4. backward: dx -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gn_tokens_bwd_dx_kernel(const semidetr_gn_tokens p, const Plan pl, const float *slots)
{
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    float *tile = gn_smem, *s_mean = gn_smem + kC * kLd, *s_rstd = s_mean + kG, *s_c1 = s_rstd + kG, *s_c2 = s_c1 + kG;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.tfirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.tfirst[l], T = pl.tiles[l];
    const int n = r / T, p0 = (r - n * T) * kTile;
    const int hw = (int)p.hw[l], npix = min(kTile, hw - p0);
    const double len = (double)kCg * hw;
    const int U = pl.units[l];
    const float *unit0 = slots + (int64_t)(pl.ufirst[l] + n * U) * kSlot + 2 * kC;
    for (int j = 0; j < kG / kWaves; ++j) {
        const int g = wave * (kG / kWaves) + j;
        double a = 0.0, b = 0.0;
        for (int u = lane; u < U; u += 64) {
            a += (double)unit0[(int64_t)u * kSlot + g];
            b += (double)unit0[(int64_t)u * kSlot + kG + g];
        }
        a = wave_sum64(a);
        b = wave_sum64(b);
        if (lane == 0) {
            s_c1[g] = (float)(a / len);
            s_c2[g] = (float)(b / len);
            s_mean[g] = p.mean[(n * p.levels + l) * kG + g];
            s_rstd[g] = p.rstd[(n * p.levels + l) * kG + g];
        }
    }
    const float4 w4 = reinterpret_cast<const float4 *>(p.weight[l])[lane];
    float *col = tile + 4 * lane * kLd;
    for (int pp = wave; pp < npix; pp += kWaves) {
        const float4 gw = mul4(load_g(p, n, p.start[l] + p0 + pp, lane), w4);
        col[pp] = gw.x;
        col[kLd + pp] = gw.y;
        col[2 * kLd + pp] = gw.z;
        col[3 * kLd + pp] = gw.w;
    }
    __syncthreads();
    const void *x = p.x[l];
    void *gx = p.grad_x[l];
    const int xt = p.x_type;
    const int64_t xb = (int64_t)n * p.x_batch_stride[l] + p0, gb = (int64_t)n * kC * hw + p0;
    if (pl.vec[l]) {
        const int cc = lane >> 4, p4 = (lane & 15) * 4;
        if (p4 < npix) {
            #pragma unroll 4
            for (int i = 0; i < kC / 16; ++i) {
                const int c = i * 16 + wave * 4 + cc;
                const float4 v = ld4(x, xt, xb + (int64_t)c * hw + p4);
                const float m = s_mean[c >> 3], rs = s_rstd[c >> 3], c1 = s_c1[c >> 3], c2 = s_c2[c >> 3];
                const float *s = tile + c * kLd + p4;
                st4(gx, xt, gb + (int64_t)c * hw + p4,
                    make_float4(dx1(s[0], xhat1(v.x, m, rs), rs, c1, c2), dx1(s[1], xhat1(v.y, m, rs), rs, c1, c2),
                                dx1(s[2], xhat1(v.z, m, rs), rs, c1, c2), dx1(s[3], xhat1(v.w, m, rs), rs, c1, c2)));
            }
        }
    } else if (lane < npix) {
        #pragma unroll 8
        for (int i = 0; i < kC / kWaves; ++i) {
            const int c = i * kWaves + wave;
            const float m = s_mean[c >> 3], rs = s_rstd[c >> 3];
            const float xh = xhat1(ld1(x, xt, xb + (int64_t)c * hw + lane), m, rs);
            st1(gx, xt, gb + (int64_t)c * hw + lane, dx1(tile[c * kLd + lane], xh, rs, s_c1[c >> 3], s_c2[c >> 3]));
        }
    }
}

// ---- 5. backward: parameter reduce ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kParts) void gn_tokens_param_kernel(const semidetr_gn_tokens p, const Plan pl, const float *slots)
{
    __shared__ double part[kParts][64];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, l = blockIdx.y;
    const int col = blockIdx.x * 64 + lane;                      // 0 .. 511: dweight | dbias
    float *out = col < kC ? p.grad_weight[l] : p.grad_bias[l];   // the same for the whole workgroup (64 divides 256)
    if (!out) return;
    const int num = pl.ufirst[l + 1] - pl.ufirst[l];
    const float *base = slots + (int64_t)pl.ufirst[l] * kSlot + col;
    const int chunk = (num + kParts - 1) / kParts;
    const int first = k * chunk, last = min(first + chunk, num);
    double acc = 0.0;
    #pragma unroll 8
    for (int sl = first; sl < last; ++sl) acc += (double)base[(int64_t)sl * kSlot];
    part[k][lane] = acc;
    __syncthreads();
    if (k == 0) {
        #pragma unroll
        for (int j = 1; j < kParts; ++j) acc += part[j][lane];
        out[col & (kC - 1)] = (float)acc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
bool known_type(int type) { return type == SEMIDETR_ROW_F32 || type == SEMIDETR_ROW_FP16 || type == SEMIDETR_ROW_BF16; }
bool aligned(const void *ptr, int type) { return ((uintptr_t)ptr & (type == SEMIDETR_ROW_F32 ? 15 : 7)) == 0; }
bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

int rows_check(const char *what, const void *ptr, int type, const int64_t *stride)
{
    SEMIDETR_REQUIRE(aligned(ptr, type) && stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0,
                     SEMIDETR_E_BADARG, "gn_tokens: the rows of %s must be %d-byte aligned (base; strides non-negative multiples of 4 elements)",
                     what, type == SEMIDETR_ROW_F32 ? 16 : 8);
    return SEMIDETR_OK;
}

// Host-side check of the parameter block (everything but the workspace) and the grids.
int plan(const semidetr_gn_tokens *params, int for_backward, Plan &pl)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "gn_tokens: null pointer (parameter block)");
    const semidetr_gn_tokens &p = params[0];
    SEMIDETR_REQUIRE(p.channels == kC && p.groups == kG, SEMIDETR_E_BADARG,
                     "gn_tokens: %d channels in %d groups (only %d in %d is built)", p.channels, p.groups, kC, kG);
    SEMIDETR_REQUIRE(p.levels >= 1 && p.levels <= kMaxLevels, SEMIDETR_E_BADARG, "gn_tokens: %d levels (1 .. %d)", p.levels, kMaxLevels);
    SEMIDETR_REQUIRE(p.batch >= 1, SEMIDETR_E_BADARG, "gn_tokens: bad sizes (batch=%d)", p.batch);
    SEMIDETR_REQUIRE(p.eps == p.eps, SEMIDETR_E_BADARG, "gn_tokens: eps is NaN");
    SEMIDETR_REQUIRE(known_type(p.x_type) && known_type(p.out_type), SEMIDETR_E_BADARG,
                     "gn_tokens: unknown type code (x_type=%d out_type=%d; SEMIDETR_ROW_F32 / _FP16 / _BF16)", p.x_type, p.out_type);
    SEMIDETR_REQUIRE(p.out_type == SEMIDETR_ROW_F32 || p.out_type == p.x_type, SEMIDETR_E_BADARG,
                     "gn_tokens: out_type %d is neither fp32 nor x_type %d", p.out_type, p.x_type);
    SEMIDETR_REQUIRE(p.tokens_per_image >= 1, SEMIDETR_E_BADARG, "gn_tokens: bad sizes (tokens_per_image=%lld)", (long long)p.tokens_per_image);
    SEMIDETR_REQUIRE(p.batch <= 65535 && p.tokens_per_image < ((int64_t)1 << 31) &&
                         (int64_t)p.batch * p.tokens_per_image * kC < ((int64_t)1 << 31),
                     SEMIDETR_E_TOOLARGE, "gn_tokens: too large (batch * tokens_per_image * 256 < 2^31, batch <= 65535)");
    int64_t end = 0;
    for (int l = 0; l < p.levels; ++l) {
        SEMIDETR_REQUIRE(p.hw[l] >= 1, SEMIDETR_E_BADARG, "gn_tokens: bad sizes (hw[%d]=%lld)", l, (long long)p.hw[l]);
        SEMIDETR_REQUIRE(p.start[l] >= end && p.hw[l] <= p.tokens_per_image - p.start[l], SEMIDETR_E_BADARG,
                         "gn_tokens: rows [%lld, %lld + %lld) of level %d overlap the level before it or pass tokens_per_image=%lld",
                         (long long)p.start[l], (long long)p.start[l], (long long)p.hw[l], l, (long long)p.tokens_per_image);
        end = p.start[l] + p.hw[l];
    }
    SEMIDETR_REQUIRE(p.mean && p.rstd, SEMIDETR_E_BADARG, "gn_tokens: null pointer (mean / rstd)");
    for (int l = 0; l < p.levels; ++l) {
        SEMIDETR_REQUIRE(p.x[l] && p.weight[l], SEMIDETR_E_BADARG, "gn_tokens: null pointer (x[%d] / weight[%d])", l, l);
        SEMIDETR_REQUIRE(p.x_batch_stride[l] >= 0 && p.x_batch_stride[l] < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                         "gn_tokens: x_batch_stride[%d] outside [0, 2^31)", l);
        SEMIDETR_REQUIRE(aligned(p.x[l], p.x_type) && p.x_batch_stride[l] % 4 == 0 && aligned16(p.weight[l]), SEMIDETR_E_BADARG,
                         "gn_tokens: x[%d] must be %d-byte aligned with a batch stride that is a multiple of 4 elements, weight[%d] 16-byte aligned",
                         l, p.x_type == SEMIDETR_ROW_F32 ? 16 : 8, l);
        if (!for_backward) {
            SEMIDETR_REQUIRE(p.bias[l] && aligned16(p.bias[l]), SEMIDETR_E_BADARG, "gn_tokens forward: bias[%d] null or not 16-byte aligned", l);
        } else {
            SEMIDETR_REQUIRE(p.grad_x[l] && aligned(p.grad_x[l], p.x_type), SEMIDETR_E_BADARG,
                             "gn_tokens backward: grad_x[%d] null or misaligned", l);
        }
    }
    if (!for_backward) {
        SEMIDETR_REQUIRE(p.tokens && aligned(p.tokens, p.out_type), SEMIDETR_E_BADARG, "gn_tokens forward: tokens null or misaligned");
        SEMIDETR_REQUIRE(!p.q == !p.pos, SEMIDETR_E_BADARG, "gn_tokens forward: q and pos come together");
        if (p.q) {
            SEMIDETR_REQUIRE(known_type(p.pos_type), SEMIDETR_E_BADARG,
                             "gn_tokens forward: unknown type code (pos_type=%d; SEMIDETR_ROW_F32 / _FP16 / _BF16)", p.pos_type);
            SEMIDETR_REQUIRE(aligned(p.q, p.out_type), SEMIDETR_E_BADARG, "gn_tokens forward: q misaligned");
            if (int rc = rows_check("pos", p.pos, p.pos_type, p.pos_stride)) return rc;
        }
    } else {
        SEMIDETR_REQUIRE(p.gy || p.gq, SEMIDETR_E_BADARG, "gn_tokens backward: null pointer (gy and gq)");
        if (p.gy) if (int rc = rows_check("gy", p.gy, p.out_type, p.gy_stride)) return rc;
        if (p.gq) if (int rc = rows_check("gq", p.gq, p.out_type, p.gq_stride)) return rc;
    }
    pl.cfirst[0] = pl.tfirst[0] = pl.ufirst[0] = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        const int64_t hw = l < p.levels ? p.hw[l] : 0;
        pl.chunks[l] = (int)((kCg * hw + kChunk - 1) / kChunk);
        pl.tiles[l] = (int)((hw + kTile - 1) / kTile);
        pl.units[l] = (int)((hw + kUnit - 1) / kUnit);
        pl.vec[l] = hw % 4 == 0;
        pl.cfirst[l + 1] = pl.cfirst[l] + p.batch * kG * pl.chunks[l];
        pl.tfirst[l + 1] = pl.tfirst[l] + p.batch * pl.tiles[l];
        pl.ufirst[l + 1] = pl.ufirst[l] + p.batch * pl.units[l];
    }
    return SEMIDETR_OK;
}

size_t workspace_bytes(const semidetr_gn_tokens &p, const Plan &pl, int for_backward)
{
    return for_backward ? (size_t)pl.ufirst[p.levels] * kSlot * sizeof(float) : (size_t)pl.cfirst[p.levels] * sizeof(float2);
}

int workspace_check(const semidetr_gn_tokens &p, const Plan &pl, int for_backward, const void *workspace, size_t bytes)
{
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) && bytes >= workspace_bytes(p, pl, for_backward), SEMIDETR_E_BADARG,
                     "gn_tokens: workspace null, misaligned or smaller than semidetr_gn_tokens_workspace_bytes()");
    return SEMIDETR_OK;
}

}  // namespace

extern "C" size_t semidetr_gn_tokens_workspace_bytes(const semidetr_gn_tokens *params, int for_backward)
{
    // sizes only: the pointers of the block are not looked at
    if (!params) return 0;
    const semidetr_gn_tokens &p = params[0];
    if (p.channels != kC || p.groups != kG || p.levels < 1 || p.levels > kMaxLevels || p.batch < 1 || p.batch > 65535) return 0;
    if (p.tokens_per_image < 1 || p.tokens_per_image >= ((int64_t)1 << 31) ||
        (int64_t)p.batch * p.tokens_per_image * kC >= ((int64_t)1 << 31)) return 0;
    Plan pl{};
    for (int l = 0; l < p.levels; ++l) {
        if (p.hw[l] < 1 || p.hw[l] > p.tokens_per_image) return 0;
        pl.cfirst[l + 1] = pl.cfirst[l] + p.batch * kG * (int)((kCg * p.hw[l] + kChunk - 1) / kChunk);
        pl.ufirst[l + 1] = pl.ufirst[l] + p.batch * (int)((p.hw[l] + kUnit - 1) / kUnit);
    }
    return workspace_bytes(p, pl, for_backward);
}

extern "C" int semidetr_gn_tokens_forward(void *stream, const semidetr_gn_tokens *params, void *workspace, size_t workspace_bytes)
{
    Plan pl;
    if (int rc = plan(params, 0, pl)) return rc;
    const semidetr_gn_tokens &p = params[0];
    if (int rc = workspace_check(p, pl, 0, workspace, workspace_bytes)) return rc;
    if (int rc = semidetr::allow_big_lds(&gn_tokens_fwd_kernel, kLdsBytes, "gn_tokens_forward")) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    float2 *partial = static_cast<float2 *>(workspace);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(pl.cfirst[p.levels]), dim3(kThreads), 0, st, p, pl, partial);
    if (int rc = semidetr::launch_status("gn_stats_kernel")) return rc;
    hipLaunchKernelGGL(gn_tokens_fwd_kernel, dim3(pl.tfirst[p.levels]), dim3(kThreads), kLdsBytes, st, p, pl, partial);
    return semidetr::launch_status("gn_tokens_fwd_kernel");
}

extern "C" int semidetr_gn_tokens_backward(void *stream, const semidetr_gn_tokens *params, void *workspace, size_t workspace_bytes)
{
    Plan pl;
    if (int rc = plan(params, 1, pl)) return rc;
    const semidetr_gn_tokens &p = params[0];
    if (int rc = workspace_check(p, pl, 1, workspace, workspace_bytes)) return rc;
    if (int rc = semidetr::allow_big_lds(&gn_tokens_bwd_sums_kernel, kLdsBytes, "gn_tokens_backward")) return rc;
    if (int rc = semidetr::allow_big_lds(&gn_tokens_bwd_dx_kernel, kLdsBytes, "gn_tokens_backward")) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    float *slots = static_cast<float *>(workspace);
    hipLaunchKernelGGL(gn_tokens_bwd_sums_kernel, dim3(pl.ufirst[p.levels]), dim3(kThreads), kLdsBytes, st, p, pl, slots);
    if (int rc = semidetr::launch_status("gn_tokens_bwd_sums_kernel")) return rc;
    hipLaunchKernelGGL(gn_tokens_bwd_dx_kernel, dim3(pl.tfirst[p.levels]), dim3(kThreads), kLdsBytes, st, p, pl, slots);
    if (int rc = semidetr::launch_status("gn_tokens_bwd_dx_kernel")) return rc;
    bool params_wanted = false;
    for (int l = 0; l < p.levels; ++l) params_wanted = params_wanted || p.grad_weight[l] || p.grad_bias[l];
    if (!params_wanted) return SEMIDETR_OK;
    hipLaunchKernelGGL(gn_tokens_param_kernel, dim3(2 * kC / 64, p.levels), dim3(64 * kParts), 0, st, p, pl, slots);
    return semidetr::launch_status("gn_tokens_param_kernel");
}

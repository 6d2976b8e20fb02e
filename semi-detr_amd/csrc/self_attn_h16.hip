// Decoder self-attention core for gfx950 on fp16 / bf16 operands: the second, named arithmetic ("operand") beside the fp32 one
// of self_attn.hip, as msda_h16.hip stands beside msda.hip.  q, k, v, grad_out and the saved out are read in place as 16-bit
// (rows 8-byte aligned), tiles sit in LDS as 16-bit, out / dq / dk / dv are written as 16-bit by the kernels; no fp32 copy of
// an operand exists in memory or in LDS.  All four products run on v_mfma_f32_32x32x16_{f16,bf16}: 2 MFMAs per 32 x 32 x 32
// product where the fp32 chain takes 16.  T16 = __half | __hip_bfloat16.
//
// Kernels and geometry are those of self_attn.hip (self_attn_tiles.h holds what the two share):
//   sattn_class_kernel        tile classes of the byte mask
//   sattn16_q_kernel<T, 0>    forward: workgroup = 2 waves = 64 queries of one (image, head); key tiles of 32 through LDS
//   sattn16_q_kernel<T, 1>    backward: delta_i = sum_d dO_id O_id (fp32, written for the next launch), P, dS, dQ
//   sattn16_dkv_kernel<T>     workgroup = 2 waves = 64 keys; query tiles of 32 through LDS; dK and dV
// Blocked tiles are neither staged nor multiplied.  No float atomics, no memset, every sum in a fixed order: bitwise
// reproducible.
//
// Data flow (lane l: c = l & 31, h = l >> 5).  A 32x32x16 MFMA takes A[row c][k = 8 h + j] and B[k = 8 h + j][col c] in element
// j = 0..7 of a lane's fragment and leaves row R(r, h) = (r & 3) + 8 (r >> 2) + 4 h of column c in accumulator register r, the map
// of the fp32 kernel.  Two kinds of product:
//   over d      S^T = K Q^T, dP^T = V dO^T (query side); S = Q K^T, dP = dO V^T (key side).  Step s = 0, 1 takes d = 16 s + 8 h + j:
//               A = 16 bytes of row c of a row-major LDS image, B = 16 bytes of the lane's own row, loaded once from memory.
//   over rows   O^T = V^T P^T, dQ^T = K^T dS^T, dV^T = dO^T P, dK^T = Q^T dS sum over the first product's ROW index, so P / dS
//               convert in registers: registers 8 s .. 8 s + 7, rounded and packed, ARE the B fragment of step s, element j
//               standing for row R(8 s + j, h).  A wants the other operand keyed the same way: a transposed LDS image
//               Xt[d][pos(row)] with pos = row with its bits 2 and 3 swapped, so that row R(8 s + j, h) sits at 16 s + 8 h + j
//               and the fragment is again one 16-byte read.
// LDS rows are 40 elements (80 bytes): 16-byte aligned, and 16 rows of a 16-byte read fall on 16 different bank quads.
//
// Numerics contract (include/semidetr_hip.h; tests/self_attn_h16_ref64.py bounds it), in this order:
//   s = (fp32 MFMA sum of the exact products q_d k_d) * scale, the scale applied in fp32 to the score, never to q;
//   running maximum, exp2, the row sum l and lse = m + logf(l) in fp32 on the UNROUNDED probabilities;
//   P rounded once to T16 for P V and P^T dO;
//   dP = fp32 MFMA sum of the exact products dO_d v_d; delta in fp32 from dO and the saved 16-bit out;
//   dS = p (dP - delta) in fp32 with p = exp2((s - lse) log2e) unrounded, then rounded once to T16 for dS K and dS^T Q;
//   scale is applied to the fp32 accumulators of dQ and dK; every result is rounded once (RNE) on the way out.
// A row whose every key is blocked gives NaN in `out`; its backward is outside the contract.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"
#include "self_attn_tiles.h"

constexpr int kRow = kD + 8;                 // LDS row stride in elements

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

struct Launch16 : Tiles {
    semidetr_self_attn_h16 p;
    float *delta;              // (B, H, Lq)
};

template <typename T16>
__device__ __forceinline__ f32x16 mfma16(uint4 a, uint4 b, f32x16 c);
template <>
__device__ __forceinline__ f32x16 mfma16<__half>(uint4 a, uint4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16 mfma16<__hip_bfloat16>(uint4 a, uint4 b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// where row `row` of a tile sits in a transposed image: bits 2 and 3 swapped (file header)
__device__ __forceinline__ int pos_of(int row) { return (row & 0x13) | ((row & 4) << 1) | ((row & 8) >> 1); }

// A tile of 32 rows x 32 elements of `base` (row stride s0 elements, rows from row0, valid below `rows`) in the registers of the
// workgroup's 128 threads: two 8-byte loads per thread; rows past the end read as zeros.
struct TileRegs { uint2 v[2]; };

__device__ __forceinline__ TileRegs tile_load(const u16 *base, int64_t s0, int row0, int rows)
{
    TileRegs t;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
        t.v[i] = make_uint2(0u, 0u);
        if (row0 + row < rows) t.v[i] = *reinterpret_cast<const uint2 *>(base + (int64_t)(row0 + row) * s0 + 4 * c4);
    }
    return t;
}

// row-major image X[row][d]
__device__ __forceinline__ void tile_store(u16 *lds, const TileRegs &t)
{
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
        *reinterpret_cast<uint2 *>(lds + row * kRow + 4 * c4) = t.v[i];
    }
}

// transposed image Xt[d][pos_of(row)]
__device__ __forceinline__ void tile_store_t(u16 *lds, const TileRegs &t)
{
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, at = pos_of(idx >> 3), d0 = 4 * (idx & 7);
        lds[(d0 + 0) * kRow + at] = (u16)(t.v[i].x & 0xffffu);
        lds[(d0 + 1) * kRow + at] = (u16)(t.v[i].x >> 16);
        lds[(d0 + 2) * kRow + at] = (u16)(t.v[i].y & 0xffffu);
        lds[(d0 + 3) * kRow + at] = (u16)(t.v[i].y >> 16);
    }
}

// fragment of step s of row c of an image: elements 16 s + 8 h .. + 7
__device__ __forceinline__ uint4 frag(const u16 *lds, int c, int h, int s)
{
    return *reinterpret_cast<const uint4 *>(lds + c * kRow + 16 * s + 8 * h);
}

// the two fragments of a 32-element row in memory (8-byte aligned)
__device__ __forceinline__ void row_frags(uint4 (&f)[2], const u16 *row, int h)
{
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint2 a = *reinterpret_cast<const uint2 *>(row + 16 * s + 8 * h);
        const uint2 b = *reinterpret_cast<const uint2 *>(row + 16 * s + 8 * h + 4);
        f[s] = make_uint4(a.x, a.y, b.x, b.y);
    }
}

// registers 8 s .. 8 s + 7 of an accumulator, each rounded once to T16: the B fragment of step s of a product over its rows
template <typename T16>
__device__ __forceinline__ uint4 acc_frag(const f32x16 &x, int s)
{
    return make_uint4(pack2<T16>(x[8 * s], x[8 * s + 1]), pack2<T16>(x[8 * s + 2], x[8 * s + 3]),
                      pack2<T16>(x[8 * s + 4], x[8 * s + 5]), pack2<T16>(x[8 * s + 6], x[8 * s + 7]));
}

// sum over the lane's 16 elements of two rows' fragments, in fp32, in element order
template <typename T16>
__device__ __forceinline__ float dot_frags(const uint4 (&a)[2], const uint4 (&b)[2])
{
    float acc = 0.f;
    #pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned aw[4] = {a[s].x, a[s].y, a[s].z, a[s].w}, bw[4] = {b[s].x, b[s].y, b[s].z, b[s].w};
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc += Cvt<T16>::up(aw[i] & 0xffffu) * Cvt<T16>::up(bw[i] & 0xffffu);
            acc += Cvt<T16>::up(aw[i] >> 16) * Cvt<T16>::up(bw[i] >> 16);
        }
    }
    return acc;
}

// 16 accumulator registers (d = R(r, h)) of the lane's row, each rounded once -> four 8-byte stores at dst[8 g + 4 h]
template <typename T16>
__device__ __forceinline__ void row_store(u16 *dst, const f32x16 &o, int h)
{
    #pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<uint2 *>(dst + 8 * g + 4 * h) = make_uint2(pack2<T16>(o[4 * g], o[4 * g + 1]), pack2<T16>(o[4 * g + 2], o[4 * g + 3]));
}

template <typename T16, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void sattn16_q_kernel(const Launch16 L)
{
    // forward: K row-major, V transposed.  backward: K row-major, V row-major, K transposed.
    __shared__ __attribute__((aligned(16))) u16 Ks[kTile * kRow], Vx[kTile * kRow], Kt[BACKWARD ? kTile * kRow : 8];
    const semidetr_self_attn_h16 &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int qt0 = blockIdx.x * kWaves, qt = qt0 + wv;
    const int q = qt * kTile + c, qc = q < p.len_q ? q : p.len_q - 1;
    const int64_t lse_at = (int64_t)bh * p.len_q + qc;

    uint4 qf[2], gf[2];
    row_frags(qf, static_cast<const u16 *>(p.q) + qc * p.q_stride[0] + b * p.q_stride[1] + hd * kD, h);
    float delta = 0.f, lse = 0.f;
    if (BACKWARD) {
        uint4 of[2];
        const int64_t at = ((int64_t)qc * p.batch + b) * (p.heads * kD) + hd * kD;
        row_frags(gf, static_cast<const u16 *>(p.grad_out) + at, h);
        row_frags(of, static_cast<const u16 *>(p.out) + at, h);
        delta = dot_frags<T16>(gf, of);
        delta += __shfl_xor(delta, 32, 64);
        lse = p.lse[lse_at];
        if (h == 0 && q < p.len_q) L.delta[lse_at] = delta;
        if (!p.grad_q) return;
    }

    const u16 *kbase = static_cast<const u16 *>(p.k) + b * p.k_stride[1] + hd * kD;
    const u16 *vbase = static_cast<const u16 *>(p.v) + b * p.v_stride[1] + hd * kD;
    f32x16 acc = {0};                        // O^T (forward) or dQ^T (backward): d in the registers
    float m = -INFINITY, l = 0.f;
    TileScan<true> scan(L, qt0, wv);
    int kt = scan.next(L, 0);
    TileRegs kr, vr;
    if (kt < L.nkt) {
        kr = tile_load(kbase, p.k_stride[0], kt * kTile, p.len_k);
        vr = tile_load(vbase, p.v_stride[0], kt * kTile, p.len_k);
    }
    while (kt < L.nkt) {
        __syncthreads();
        tile_store(Ks, kr);
        if (BACKWARD) {
            tile_store(Vx, vr);
            tile_store_t(Kt, kr);
        } else {
            tile_store_t(Vx, vr);
        }
        __syncthreads();
        const int cls = scan.cls(kt);
        const int nxt = scan.next(L, kt + 1);
        if (nxt < L.nkt) {
            kr = tile_load(kbase, p.k_stride[0], nxt * kTile, p.len_k);
            vr = tile_load(vbase, p.v_stride[0], nxt * kTile, p.len_k);
        }
        if (cls) {
            f32x16 s = {0};                  // S^T: the lane's query against the keys R(r, h) of the tile
            #pragma unroll
            for (int i = 0; i < 2; ++i) s = mfma16<T16>(frag(Ks, c, h, i), qf[i], s);
            #pragma unroll
            for (int r = 0; r < 16; ++r) s[r] *= p.scale;
            if (cls == 1 || kt * kTile + kTile > p.len_k) {
                const uint8_t *mrow = (p.mask && cls == 1) ? p.mask + (int64_t)qc * p.len_k : nullptr;
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * kTile + row_of(r, h);
                    bool blocked = key >= p.len_k;
                    if (!blocked && mrow) blocked = mrow[key] != 0;
                    if (blocked) s[r] = -INFINITY;
                }
            }
            if (!BACKWARD) {
                float mx = s[0];
                #pragma unroll
                for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mnew = fmaxf(m, mx), msafe = mnew == -INFINITY ? 0.f : mnew;
                const float alpha = exp2_hw((m - msafe) * kLog2e);
                float psum = 0.f;
                #pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[r] = exp2_hw((s[r] - msafe) * kLog2e);
                    psum += s[r];
                }
                psum += __shfl_xor(psum, 32, 64);
                l = l * alpha + psum;
                m = mnew;
                #pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] *= alpha;
                #pragma unroll
                for (int i = 0; i < 2; ++i) acc = mfma16<T16>(frag(Vx, c, h, i), acc_frag<T16>(s, i), acc);
            } else {
                f32x16 dp = {0};
                #pragma unroll
                for (int i = 0; i < 2; ++i) dp = mfma16<T16>(frag(Vx, c, h, i), gf[i], dp);
                #pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = exp2_hw((s[r] - lse) * kLog2e) * (dp[r] - delta);
                #pragma unroll
                for (int i = 0; i < 2; ++i) acc = mfma16<T16>(frag(Kt, c, h, i), acc_frag<T16>(s, i), acc);
            }
        }
        kt = nxt;
    }
    if (q >= p.len_q) return;
    if (!BACKWARD) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] / l;
        row_store<T16>(static_cast<u16 *>(p.out) + ((int64_t)q * p.batch + b) * (p.heads * kD) + hd * kD, acc, h);
        if (h == 0) p.lse[lse_at] = m + logf(l);
    } else {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= p.scale;
        row_store<T16>(static_cast<u16 *>(p.grad_q) + q * p.gq_stride[0] + b * p.gq_stride[1] + hd * kD, acc, h);
    }
}

template <typename T16>
__global__ __launch_bounds__(kThreads) void sattn16_dkv_kernel(const Launch16 L)
{
    __shared__ __attribute__((aligned(16))) u16 Qs[kTile * kRow], Gs[kTile * kRow], Qt[kTile * kRow], Gt[kTile * kRow];
    __shared__ float lse_s[kTile], delta_s[kTile];
    const semidetr_self_attn_h16 &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int kt0 = blockIdx.x * kWaves, kt = kt0 + wv;
    const int key = kt * kTile + c, kc = key < p.len_k ? key : p.len_k - 1;

    uint4 kf[2], vf[2];
    row_frags(kf, static_cast<const u16 *>(p.k) + kc * p.k_stride[0] + b * p.k_stride[1] + hd * kD, h);
    row_frags(vf, static_cast<const u16 *>(p.v) + kc * p.v_stride[0] + b * p.v_stride[1] + hd * kD, h);
    const u16 *qbase = static_cast<const u16 *>(p.q) + b * p.q_stride[1] + hd * kD;
    const u16 *gbase = static_cast<const u16 *>(p.grad_out) + (int64_t)b * (p.heads * kD) + hd * kD;
    const int64_t gs0 = (int64_t)p.batch * p.heads * kD;
    const float *lse_g = p.lse + (int64_t)bh * p.len_q, *delta_g = L.delta + (int64_t)bh * p.len_q;

    f32x16 dk = {0}, dv = {0};               // dK^T, dV^T: d in the registers, the key on the lane
    TileScan<false> scan(L, kt0, wv);
    int qt = scan.next(L, 0);
    TileRegs qr, gr;
    float lse_r = 0.f, delta_r = 0.f;        // threads 0..31: one query's lse and delta of the tile in flight
    auto fetch = [&](int t) {
        qr = tile_load(qbase, p.q_stride[0], t * kTile, p.len_q);
        gr = tile_load(gbase, gs0, t * kTile, p.len_q);
        if (threadIdx.x < kTile) {
            const int qq = t * kTile + threadIdx.x;
            lse_r = qq < p.len_q ? lse_g[qq] : INFINITY;       // p = exp2(-inf) = 0 past the last query
            delta_r = qq < p.len_q ? delta_g[qq] : 0.f;
        }
    };
    if (qt < L.nqt) fetch(qt);
    while (qt < L.nqt) {
        __syncthreads();
        tile_store(Qs, qr);
        tile_store(Gs, gr);
        tile_store_t(Qt, qr);
        tile_store_t(Gt, gr);
        if (threadIdx.x < kTile) { lse_s[threadIdx.x] = lse_r; delta_s[threadIdx.x] = delta_r; }
        __syncthreads();
        const int cls = scan.cls(qt);
        const int nxt = scan.next(L, qt + 1);
        if (nxt < L.nqt) fetch(nxt);
        if (cls) {
            f32x16 s = {0}, dp = {0};        // S, dP: the lane's key against the queries R(r, h) of the tile
            #pragma unroll
            for (int i = 0; i < 2; ++i) s = mfma16<T16>(frag(Qs, c, h, i), kf[i], s);
            #pragma unroll
            for (int i = 0; i < 2; ++i) dp = mfma16<T16>(frag(Gs, c, h, i), vf[i], dp);
            const bool mixed = cls == 1 && p.mask && key < p.len_k;
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = row_of(r, h), qq = qt * kTile + qi;
                float pr = exp2_hw((s[r] * p.scale - lse_s[qi]) * kLog2e);
                if (mixed && qq < p.len_q && p.mask[(int64_t)qq * p.len_k + key]) pr = 0.f;
                s[r] = pr;
                dp[r] = pr * (dp[r] - delta_s[qi]);
            }
            #pragma unroll
            for (int i = 0; i < 2; ++i) dv = mfma16<T16>(frag(Gt, c, h, i), acc_frag<T16>(s, i), dv);
            #pragma unroll
            for (int i = 0; i < 2; ++i) dk = mfma16<T16>(frag(Qt, c, h, i), acc_frag<T16>(dp, i), dk);
        }
        qt = nxt;
    }
    if (key >= p.len_k) return;
    if (p.grad_k) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) dk[r] *= p.scale;
        row_store<T16>(static_cast<u16 *>(p.grad_k) + key * p.gk_stride[0] + b * p.gk_stride[1] + hd * kD, dk, h);
    }
    if (p.grad_v) row_store<T16>(static_cast<u16 *>(p.grad_v) + key * p.gv_stride[0] + b * p.gv_stride[1] + hd * kD, dv, h);
}

bool aligned(const void *ptr, uintptr_t to) { return ((uintptr_t)ptr & (to - 1)) == 0; }
bool rows_ok(const void *ptr, const int64_t *stride) { return aligned(ptr, 8) && stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0; }

// Host-side check of the parameter block + launch geometry.  Returns SEMIDETR_OK or an error (message set).
int plan(const semidetr_self_attn_h16 *params, void *workspace, size_t workspace_bytes, Launch16 &L, int for_backward)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "self_attn_h16: null pointer (parameter block)");
    const semidetr_self_attn_h16 &p = params[0];
    SEMIDETR_REQUIRE(p.type == SEMIDETR_ROW_FP16 || p.type == SEMIDETR_ROW_BF16, SEMIDETR_E_BADARG,
                     "self_attn_h16: element type %d (SEMIDETR_ROW_FP16 or SEMIDETR_ROW_BF16; fp32 rows take semidetr_self_attn_*_f32)",
                     p.type);
    SEMIDETR_REQUIRE(p.head_dim == kD, SEMIDETR_E_BADARG, "self_attn_h16: head dimension %d (only %d is built)", p.head_dim, kD);
    if (int rc = sizes_ok(p, "self_attn_h16")) return rc;
    SEMIDETR_REQUIRE(p.q && p.k && p.v && p.out && p.lse, SEMIDETR_E_BADARG, "self_attn_h16: null pointer (q / k / v / out / lse)");
    SEMIDETR_REQUIRE(rows_ok(p.q, p.q_stride) && rows_ok(p.k, p.k_stride) && rows_ok(p.v, p.v_stride) && aligned(p.out, 8) &&
                         aligned(p.lse, 4),
                     SEMIDETR_E_BADARG, "self_attn_h16: rows must be 8-byte aligned (base, strides multiples of 4) with non-negative strides");
    if (for_backward) {
        SEMIDETR_REQUIRE(p.grad_out && aligned(p.grad_out, 8), SEMIDETR_E_BADARG, "self_attn_h16 backward: null or misaligned grad_out");
        SEMIDETR_REQUIRE(p.grad_q || p.grad_k || p.grad_v, SEMIDETR_E_BADARG, "self_attn_h16 backward: no gradient asked for");
        SEMIDETR_REQUIRE((!p.grad_q || rows_ok(p.grad_q, p.gq_stride)) && (!p.grad_k || rows_ok(p.grad_k, p.gk_stride)) &&
                             (!p.grad_v || rows_ok(p.grad_v, p.gv_stride)),
                         SEMIDETR_E_BADARG, "self_attn_h16 backward: gradient rows must be 8-byte aligned (base, strides multiples of 4)");
    }
    SEMIDETR_REQUIRE(workspace && aligned(workspace, 16) &&
                         workspace_bytes >= semidetr_self_attn_workspace_bytes(p.batch, p.heads, p.len_q, p.len_k),
                     SEMIDETR_E_BADARG, "self_attn_h16: workspace null, misaligned or smaller than semidetr_self_attn_workspace_bytes()");
    L.p = p;
    carve(p, workspace, L, L.delta);
    return SEMIDETR_OK;
}

template <typename T16>
int forward(hipStream_t st, const Launch16 &L)
{
    const dim3 grid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn16_q_kernel<T16, false>), grid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status("sattn16_q_kernel (forward)");
}

template <typename T16>
int backward(hipStream_t st, const Launch16 &L)
{
    const dim3 qgrid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn16_q_kernel<T16, true>), qgrid, dim3(kThreads), 0, st, L);
    if (int rc = semidetr::launch_status("sattn16_q_kernel (backward)")) return rc;
    if (!L.p.grad_k && !L.p.grad_v) return SEMIDETR_OK;
    const dim3 kgrid((L.nkt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn16_dkv_kernel<T16>), kgrid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status("sattn16_dkv_kernel");
}

}  // namespace

extern "C" int semidetr_self_attn_forward_h16(void *stream, const semidetr_self_attn_h16 *params, void *workspace,
                                              size_t workspace_bytes)
{
    Launch16 L;
    if (int rc = plan(params, workspace, workspace_bytes, L, 0)) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    if (int rc = launch_class(st, L, L.p.mask, L.p.len_q, L.p.len_k)) return rc;
    return L.p.type == SEMIDETR_ROW_FP16 ? forward<__half>(st, L) : forward<__hip_bfloat16>(st, L);
}

extern "C" int semidetr_self_attn_backward_h16(void *stream, const semidetr_self_attn_h16 *params, void *workspace,
                                               size_t workspace_bytes)
{
    Launch16 L;
    if (int rc = plan(params, workspace, workspace_bytes, L, 1)) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    if (int rc = launch_class(st, L, L.p.mask, L.p.len_q, L.p.len_k)) return rc;
    return L.p.type == SEMIDETR_ROW_FP16 ? backward<__half>(st, L) : backward<__hip_bfloat16>(st, L);
}

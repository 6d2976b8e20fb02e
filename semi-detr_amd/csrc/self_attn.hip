// Decoder self-attention core for gfx950: out = softmax(scale * Q K^T + mask) V, forward and backward, head dimension 32
// (DINOTransformerDecoderLayer.forward_sa, detr_od/models/utils/transformer.py:975-1039: the nn.MultiheadAttention call
// without its two projections, which stay GEMMs).  The (Lq, Lk) scores never reach memory.  Two arithmetics, one kernel template
// each for the query side and the key side; an arithmetic is a policy struct that holds what differs and nothing else:
//   ArithF32          fp32 in / arithmetic / out on v_mfma_f32_32x32x2_f32 (an exact k-ordered fmaf chain), rows 16-byte aligned
//   ArithH16<T16>     the "operand" arithmetic, T16 = __half | __hip_bfloat16: q, k, v, grad_out and the saved out are read in
//                     place as 16-bit (rows 8-byte aligned), tiles sit in LDS as 16-bit, out / dq / dk / dv are written as 16-bit;
//                     no fp32 copy of an operand exists in memory or in LDS.  All four products run on
//                     v_mfma_f32_32x32x16_{f16,bf16}: 2 MFMAs per 32 x 32 x 32 product where the fp32 chain takes 16.
//
//   sattn_class_kernel       one wave per 32 x 32 tile of the byte mask: 0 = every in-range element blocked, 2 = none, 1 = mixed
//   sattn_q_kernel<A, 0>     forward: workgroup = 2 waves = 64 queries of one (image, head), wave = 32 queries; key tiles of 32
//                            through LDS
//   sattn_q_kernel<A, 1>     backward, same geometry: delta_i = sum_d dO_id O_id (fp32, written for the next launch),
//                            P = exp(s - lse), dS, dQ
//   sattn_dkv_kernel<A>      workgroup = 2 waves = 64 keys, wave = 32 keys; query tiles of 32 through LDS; dK and dV
// A key tile of class 0 for both waves of a workgroup is neither staged nor multiplied; a wave skips the matrix work of a tile
// of class 0 for its own 32 rows; a tile of class 2 reads no mask byte.  No float atomics, no memset, every sum in a fixed
// order: bitwise reproducible.
//
// Data flow (lane l: c = l & 31, h = l >> 5; register r of an accumulator is row R(r, h) = (r & 3) + 8 (r >> 2) + 4 h of column c,
// in both arithmetics).  Two kinds of product:
//   over d      S^T = K Q^T, dP^T = V dO^T (query side: a lane owns one query and its registers are 16 keys, so row maximum and
//               row sum are in-lane plus one exchange with lane l ^ 32); S = Q K^T, dP = dO V^T (key side, the key on the lane).
//               A = row c of a row-major LDS image, B = the lane's own row, loaded once from memory.
//               fp32: 16 steps, d = 2 s + h, the row in 16 registers.  16-bit: 2 steps, d = 16 s + 8 h + j, both 16-byte fragments.
//   over rows   O^T = V^T P^T, dQ^T = K^T dS^T, dV^T = dO^T P, dK^T = Q^T dS sum over the first product's ROW index, so P / dS are
//               B straight from the registers.  fp32: step r takes B = register r and A = X[row R(r, h)][d = c] of the same image.
//               16-bit: registers 8 s .. 8 s + 7, rounded and packed, ARE the B fragment of step s, element j standing for row
//               R(8 s + j, h); A wants the other operand keyed the same way: a transposed LDS image Xt[d][pos(row)] with pos =
//               row with its bits 2 and 3 swapped, so that row R(8 s + j, h) sits at 16 s + 8 h + j and the fragment is again
//               one 16-byte read.
// LDS rows: 33 floats (an image read down a column of lanes), or 40 16-bit elements (80 bytes: 16-byte aligned, and 16 rows of a
// 16-byte read fall on 16 different bank quads).
//
// Arithmetic, in this order.  fp32 (tests/self_attn_ref64.py bounds it): Qs = q * scale (one rounding); s = fma chain over d;
//   per key tile: m' = max(m, max_j s_j); p_j = exp2((s_j - m') * log2e) (v_exp_f32); l = l * exp2((m - m') * log2e) + sum_j p_j;
//   O = O * exp2((m - m') * log2e) then the fma chain over the tile's keys; out = O / l; lse = m + logf(l).
//   backward: p = exp2((s - lse) * log2e), dS = p * (dP - delta), dQ = (fma chain of dS k) * scale, dK = fma chain of dS Qs.
// 16-bit (include/semidetr_hip.h; tests/self_attn_h16_ref64.py bounds it): s = (fp32 MFMA sum of the exact products q_d k_d) *
//   scale, the scale applied in fp32 to the score, never to q; running maximum, exp2, the row sum l and lse in fp32 on the
//   UNROUNDED probabilities; P rounded once to T16 for P V and P^T dO; dP = fp32 MFMA sum of the exact products dO_d v_d; delta in
//   fp32 from dO and the saved 16-bit out; dS = p (dP - delta) in fp32 with p unrounded, then rounded once to T16 for dS K and
//   dS^T Q; scale is applied to the fp32 accumulators of dQ and dK; every result is rounded once (RNE) on the way out.
// A row whose every key is blocked gives NaN in `out` (torch's softmax of a row of -inf); its backward is outside the contract.
//
// Which products the compiler contracts into fmas is its choice per basic block; every instance below inlines to the statements,
// in the order, of the kernel it replaced (two files, one per arithmetic), and tests/test_gpu_self_attn_bits.py holds the bits.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"

constexpr int kD = 32;                       // head dimension
constexpr int kTile = 32;                    // rows of an MFMA tile: queries per wave, keys per staged tile
constexpr int kWaves = 2, kThreads = 64 * kWaves;
constexpr float kLog2e = 1.44269504088896340736f;
constexpr int kPad = kD + 1;                 // fp32 LDS row stride in floats
constexpr int kRow = kD + 8;                 // 16-bit LDS row stride in elements

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

// The launch of every kernel: the (widened) parameter block and the workspace = delta (B, H, Lq) fp32, then the class bytes.
struct Launch {
    const uint8_t *cls;        // (nqt, nkt) tile classes, NULL without a mask
    int nqt, nkt;              // 32-row tiles of queries / keys
    semidetr_self_attn_h16 p;
    float *delta;              // (B, H, Lq)
};

// register r of a 32 x 32 accumulator in lane half h holds this row (the column is the lane & 31)
__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ int tile_class(const Launch &L, int qt, int kt)
{
    if (qt >= L.nqt || kt >= L.nkt) return 0;
    return L.cls ? (int)L.cls[qt * L.nkt + kt] : 2;
}

__global__ __launch_bounds__(64) void sattn_class_kernel(const uint8_t *__restrict__ mask, int Lq, int Lk, int nkt,
                                                         uint8_t *__restrict__ cls)
{
    const int kt = blockIdx.x, qt = blockIdx.y, lane = threadIdx.x;
    const int q = qt * kTile + (lane >> 1), k0 = kt * kTile + 16 * (lane & 1);
    bool open = false, blocked = false;
    if (q < Lq) {
        for (int j = 0; j < 16; ++j) {
            if (k0 + j >= Lk) break;
            const bool b = mask[(int64_t)q * Lk + k0 + j] != 0;
            open |= !b;
            blocked |= b;
        }
    }
    const bool any_open = __ballot(open) != 0, any_blocked = __ballot(blocked) != 0;
    if (lane == 0) cls[qt * nkt + kt] = any_open ? (any_blocked ? 1 : 2) : 0;
}

// The classes of 64 consecutive tiles at a time, one tile per lane, as wave-uniform bit masks: which tiles the workgroup stages
// (a tile open for either wave) and which this wave multiplies.  BY_KEY walks the key tiles of the query tiles (a0, a0 + 1),
// otherwise the query tiles of the key tiles (a0, a0 + 1).
template <bool BY_KEY>
struct TileScan {
    uint64_t open, mine, mixed;
    int base, n, a0, wv;
    __device__ __forceinline__ TileScan(const Launch &L, int a0_, int wv_) : n(BY_KEY ? L.nkt : L.nqt), a0(a0_), wv(wv_) { load(L, 0); }
    __device__ __forceinline__ void load(const Launch &L, int b)
    {
        base = b;
        const int t = b + (threadIdx.x & 63);
        const int c0 = BY_KEY ? tile_class(L, a0, t) : tile_class(L, t, a0);
        const int c1 = BY_KEY ? tile_class(L, a0 + 1, t) : tile_class(L, t, a0 + 1);
        const int cm = wv ? c1 : c0;
        open = __ballot((c0 | c1) != 0);
        mine = __ballot(cm != 0);
        mixed = __ballot(cm == 1);
    }
    // the first tile >= t that the workgroup stages, n when there is none
    __device__ __forceinline__ int next(const Launch &L, int t)
    {
        while (t < n) {
            if (t >= base + 64) load(L, t & ~63);
            const uint64_t m = open >> (t - base);
            if (m) return t + __builtin_ctzll(m);
            t = base + 64;
        }
        return n;
    }
    // this wave's class of tile t of the loaded 64
    __device__ __forceinline__ int cls(int t) const
    {
        const int s = t - base;
        return ((mine >> s) & 1) ? (((mixed >> s) & 1) ? 1 : 2) : 0;
    }
};

// A tile of 32 rows x 32 elements of `base` (row stride s0 elements, rows from row0, valid below `rows`) in the registers of the
// workgroup's 128 threads: two V per thread, V = four elements (float4 or uint2); rows past the end read as zeros.
template <typename V>
struct TileRegs { V v[2]; };

// the zero fill, written out per type: `V{}` compiles to other moves and to other kernel times
__device__ __forceinline__ void clear(float4 &v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void clear(uint2 &v) { v = make_uint2(0u, 0u); }

template <typename V, typename E>
__device__ __forceinline__ TileRegs<V> tile_load(const E *base, int64_t s0, int row0, int rows)
{
    TileRegs<V> t;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
        clear(t.v[i]);
        if (row0 + row < rows) t.v[i] = *reinterpret_cast<const V *>(base + (int64_t)(row0 + row) * s0 + 4 * c4);
    }
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The fp32 arithmetic.  scale is folded into q: into the lane's row at load (query side), into the staged Qs (key side), so dK
// needs none; dQ is scaled at the end.
// ---------------------------------------------------------------------------------------------------------------------------
struct ArithF32 {
    typedef float Elem;
    typedef float4 Vec;
    typedef float Frag[16];                  // the lane's row: the 16 elements d = 2 s + h

    static __device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

    static __device__ __forceinline__ void tile_store(float *lds, const TileRegs<Vec> &t, float mul)
    {
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
            float *d = lds + row * kPad + 4 * c4;
            d[0] = t.v[i].x * mul; d[1] = t.v[i].y * mul; d[2] = t.v[i].z * mul; d[3] = t.v[i].w * mul;
        }
    }
    // the 16 elements d = 2 s + h of a row, times mul
    static __device__ __forceinline__ void row_load(Frag &dst, const float *row, int h, float mul)
    {
        #pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(row + 4 * i);
            dst[2 * i] = (h ? v.y : v.x) * mul;
            dst[2 * i + 1] = (h ? v.w : v.z) * mul;
        }
    }
    static __device__ __forceinline__ void load_q(Frag &dst, const float *row, int h, float scale) { row_load(dst, row, h, scale); }
    static __device__ __forceinline__ void load_row(Frag &dst, const float *row, int h) { row_load(dst, row, h, 1.f); }
    static __device__ __forceinline__ float late(float x, float) { return x; }        // scale is in q already

    // one image per operand serves both kinds of product
    template <bool BACKWARD>
    struct QTile {
        float K[kTile * kPad], V[kTile * kPad];
        __device__ __forceinline__ void stage(const TileRegs<Vec> &kr, const TileRegs<Vec> &vr) { tile_store(K, kr, 1.f); tile_store(V, vr, 1.f); }
        __device__ __forceinline__ const float *k_d() const { return K; }
        __device__ __forceinline__ const float *v_d() const { return V; }
        __device__ __forceinline__ const float *k_rows() const { return K; }
        __device__ __forceinline__ const float *v_rows() const { return V; }
    };
    struct KvTile {
        float Q[kTile * kPad], G[kTile * kPad];
        __device__ __forceinline__ void stage(const TileRegs<Vec> &qr, const TileRegs<Vec> &gr, float scale) { tile_store(Q, qr, scale); tile_store(G, gr, 1.f); }
        __device__ __forceinline__ const float *q_d() const { return Q; }
        __device__ __forceinline__ const float *g_d() const { return G; }
        __device__ __forceinline__ const float *q_rows() const { return Q; }
        __device__ __forceinline__ const float *g_rows() const { return G; }
    };

    static __device__ __forceinline__ f32x16 over_d(const float *img, const Frag &f, int c, int h)
    {
        f32x16 s = {0};
        #pragma unroll
        for (int i = 0; i < 16; ++i) s = mfma(img[c * kPad + 2 * i + h], f[i], s);
        return s;
    }
    static __device__ __forceinline__ f32x16 over_rows(const float *img, const f32x16 &x, f32x16 acc, int c, int h)
    {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc = mfma(img[row_of(r, h) * kPad + c], x[r], acc);
        return acc;
    }
    // the lane's half of sum_d a_d b_d, in element order
    static __device__ __forceinline__ float dot(const Frag &a, const Frag &b)
    {
        float acc = 0.f;
        #pragma unroll
        for (int i = 0; i < 16; ++i) acc += a[i] * b[i];
        return acc;
    }
    // 16 accumulator registers (d = R(r, h)) of the lane's row -> four float4 at dst[8 g + 4 h]
    static __device__ __forceinline__ void row_store(float *dst, const f32x16 &o, int h)
    {
        #pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4 *>(dst + 8 * g + 4 * h) = make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The 16-bit arithmetic.  scale multiplies the fp32 score and the fp32 accumulators of dQ and dK, never an operand.
// ---------------------------------------------------------------------------------------------------------------------------
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

template <typename T16>
struct ArithH16 {
    typedef u16 Elem;
    typedef uint2 Vec;
    typedef uint4 Frag[2];                   // the lane's row: two fragments, elements d = 16 s + 8 h + j

    // row-major image X[row][d]
    static __device__ __forceinline__ void tile_store(u16 *lds, const TileRegs<Vec> &t)
    {
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
            *reinterpret_cast<uint2 *>(lds + row * kRow + 4 * c4) = t.v[i];
        }
    }
    // transposed image Xt[d][pos_of(row)]
    static __device__ __forceinline__ void tile_store_t(u16 *lds, const TileRegs<Vec> &t)
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
    static __device__ __forceinline__ uint4 frag(const u16 *lds, int c, int h, int s)
    {
        return *reinterpret_cast<const uint4 *>(lds + c * kRow + 16 * s + 8 * h);
    }
    // the two fragments of a 32-element row in memory (8-byte aligned)
    static __device__ __forceinline__ void row_frags(Frag &f, const u16 *row, int h)
    {
        #pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint2 a = *reinterpret_cast<const uint2 *>(row + 16 * s + 8 * h);
            const uint2 b = *reinterpret_cast<const uint2 *>(row + 16 * s + 8 * h + 4);
            f[s] = make_uint4(a.x, a.y, b.x, b.y);
        }
    }
    static __device__ __forceinline__ void load_q(Frag &f, const u16 *row, int h, float) { row_frags(f, row, h); }
    static __device__ __forceinline__ void load_row(Frag &f, const u16 *row, int h) { row_frags(f, row, h); }
    static __device__ __forceinline__ float late(float x, float scale) { return x * scale; }
    // registers 8 s .. 8 s + 7 of an accumulator, each rounded once to T16: the B fragment of step s of a product over its rows
    static __device__ __forceinline__ uint4 acc_frag(const f32x16 &x, int s)
    {
        return make_uint4(pack2<T16>(x[8 * s], x[8 * s + 1]), pack2<T16>(x[8 * s + 2], x[8 * s + 3]),
                          pack2<T16>(x[8 * s + 4], x[8 * s + 5]), pack2<T16>(x[8 * s + 6], x[8 * s + 7]));
    }

    // forward: K row-major, V transposed (no Kt).  backward: K row-major, V row-major, K transposed.
    template <bool BACKWARD>
    struct QTile {
        __attribute__((aligned(16))) u16 K[kTile * kRow], Vx[kTile * kRow], Kt[BACKWARD ? kTile * kRow : 0];
        __device__ __forceinline__ void stage(const TileRegs<Vec> &kr, const TileRegs<Vec> &vr)
        {
            tile_store(K, kr);
            if (BACKWARD) {
                tile_store(Vx, vr);
                tile_store_t(Kt, kr);
            } else {
                tile_store_t(Vx, vr);
            }
        }
        __device__ __forceinline__ const u16 *k_d() const { return K; }
        __device__ __forceinline__ const u16 *v_d() const { return Vx; }
        __device__ __forceinline__ const u16 *k_rows() const { return Kt; }
        __device__ __forceinline__ const u16 *v_rows() const { return Vx; }
    };
    struct KvTile {
        __attribute__((aligned(16))) u16 Q[kTile * kRow], G[kTile * kRow], Qt[kTile * kRow], Gt[kTile * kRow];
        __device__ __forceinline__ void stage(const TileRegs<Vec> &qr, const TileRegs<Vec> &gr, float)
        {
            tile_store(Q, qr);
            tile_store(G, gr);
            tile_store_t(Qt, qr);
            tile_store_t(Gt, gr);
        }
        __device__ __forceinline__ const u16 *q_d() const { return Q; }
        __device__ __forceinline__ const u16 *g_d() const { return G; }
        __device__ __forceinline__ const u16 *q_rows() const { return Qt; }
        __device__ __forceinline__ const u16 *g_rows() const { return Gt; }
    };

    static __device__ __forceinline__ f32x16 over_d(const u16 *img, const Frag &f, int c, int h)
    {
        f32x16 s = {0};
        #pragma unroll
        for (int i = 0; i < 2; ++i) s = mfma16<T16>(frag(img, c, h, i), f[i], s);
        return s;
    }
    static __device__ __forceinline__ f32x16 over_rows(const u16 *img_t, const f32x16 &x, f32x16 acc, int c, int h)
    {
        #pragma unroll
        for (int i = 0; i < 2; ++i) acc = mfma16<T16>(frag(img_t, c, h, i), acc_frag(x, i), acc);
        return acc;
    }
    // sum over the lane's 16 elements of two rows' fragments, in fp32, in element order
    static __device__ __forceinline__ float dot(const Frag &a, const Frag &b)
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
    static __device__ __forceinline__ void row_store(u16 *dst, const f32x16 &o, int h)
    {
        #pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint2 *>(dst + 8 * g + 4 * h) = make_uint2(pack2<T16>(o[4 * g], o[4 * g + 1]), pack2<T16>(o[4 * g + 2], o[4 * g + 3]));
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The kernels: geometry, scan / stage loop, mask, softmax, dS and the guards, once for every arithmetic.
// ---------------------------------------------------------------------------------------------------------------------------
// S^T of key tile kt for query qc: blocked elements (mask byte, key past the end) become -inf
__device__ __forceinline__ f32x16 mask_scores(f32x16 s, const semidetr_self_attn_h16 &p, int kt, int cls, int qc, int h)
{
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
    return s;
}

template <typename A, bool BACKWARD>
__global__ __launch_bounds__(kThreads) void sattn_q_kernel(const Launch L)
{
    typedef typename A::Elem E;
    __shared__ typename A::template QTile<BACKWARD> T;
    const semidetr_self_attn_h16 &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int qt0 = blockIdx.x * kWaves, qt = qt0 + wv;
    const int q = qt * kTile + c, qc = q < p.len_q ? q : p.len_q - 1;
    const int64_t lse_at = (int64_t)bh * p.len_q + qc;

    typename A::Frag qf, gf;
    A::load_q(qf, static_cast<const E *>(p.q) + qc * p.q_stride[0] + b * p.q_stride[1] + hd * kD, h, p.scale);
    float delta = 0.f, lse = 0.f;
    if (BACKWARD) {
        typename A::Frag of;
        const int64_t at = ((int64_t)qc * p.batch + b) * (p.heads * kD) + hd * kD;
        A::load_row(gf, static_cast<const E *>(p.grad_out) + at, h);
        A::load_row(of, static_cast<const E *>(p.out) + at, h);
        delta = A::dot(gf, of);
        delta += __shfl_xor(delta, 32, 64);
        lse = p.lse[lse_at];
        if (h == 0 && q < p.len_q) L.delta[lse_at] = delta;
        if (!p.grad_q) return;
    }

    const E *kbase = static_cast<const E *>(p.k) + b * p.k_stride[1] + hd * kD;
    const E *vbase = static_cast<const E *>(p.v) + b * p.v_stride[1] + hd * kD;
    f32x16 acc = {0};                        // O^T (forward) or dQ^T (backward): d in the registers
    float m = -INFINITY, l = 0.f;
    TileScan<true> scan(L, qt0, wv);
    int kt = scan.next(L, 0);
    TileRegs<typename A::Vec> kr, vr;
    if (kt < L.nkt) {
        kr = tile_load<typename A::Vec>(kbase, p.k_stride[0], kt * kTile, p.len_k);
        vr = tile_load<typename A::Vec>(vbase, p.v_stride[0], kt * kTile, p.len_k);
    }
    while (kt < L.nkt) {
        __syncthreads();
        T.stage(kr, vr);
        __syncthreads();
        const int cls = scan.cls(kt);
        const int nxt = scan.next(L, kt + 1);
        if (nxt < L.nkt) {
            kr = tile_load<typename A::Vec>(kbase, p.k_stride[0], nxt * kTile, p.len_k);
            vr = tile_load<typename A::Vec>(vbase, p.v_stride[0], nxt * kTile, p.len_k);
        }
        if (cls) {
            f32x16 s = A::over_d(T.k_d(), qf, c, h);         // S^T: the lane's query against the keys R(r, h) of the tile
            #pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = A::late(s[r], p.scale);
            s = mask_scores(s, p, kt, cls, qc, h);
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
                acc = A::over_rows(T.v_rows(), s, acc, c, h);
            } else {
                const f32x16 dp = A::over_d(T.v_d(), gf, c, h);
                #pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = exp2_hw((s[r] - lse) * kLog2e) * (dp[r] - delta);
                acc = A::over_rows(T.k_rows(), s, acc, c, h);
            }
        }
        kt = nxt;
    }
    if (q >= p.len_q) return;
    if (!BACKWARD) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] / l;
        A::row_store(static_cast<E *>(p.out) + ((int64_t)q * p.batch + b) * (p.heads * kD) + hd * kD, acc, h);
        if (h == 0) p.lse[lse_at] = m + logf(l);
    } else {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= p.scale;
        A::row_store(static_cast<E *>(p.grad_q) + q * p.gq_stride[0] + b * p.gq_stride[1] + hd * kD, acc, h);
    }
}

template <typename A>
__global__ __launch_bounds__(kThreads) void sattn_dkv_kernel(const Launch L)
{
    typedef typename A::Elem E;
    __shared__ typename A::KvTile T;
    __shared__ float lse_s[kTile], delta_s[kTile];
    const semidetr_self_attn_h16 &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int kt0 = blockIdx.x * kWaves, kt = kt0 + wv;
    const int key = kt * kTile + c, kc = key < p.len_k ? key : p.len_k - 1;

    typename A::Frag kf, vf;
    A::load_row(kf, static_cast<const E *>(p.k) + kc * p.k_stride[0] + b * p.k_stride[1] + hd * kD, h);
    A::load_row(vf, static_cast<const E *>(p.v) + kc * p.v_stride[0] + b * p.v_stride[1] + hd * kD, h);
    const E *qbase = static_cast<const E *>(p.q) + b * p.q_stride[1] + hd * kD;
    const E *gbase = static_cast<const E *>(p.grad_out) + (int64_t)b * (p.heads * kD) + hd * kD;
    const int64_t gs0 = (int64_t)p.batch * p.heads * kD;
    const float *lse_g = p.lse + (int64_t)bh * p.len_q, *delta_g = L.delta + (int64_t)bh * p.len_q;

    f32x16 dk = {0}, dv = {0};               // dK^T, dV^T: d in the registers, the key on the lane
    TileScan<false> scan(L, kt0, wv);
    int qt = scan.next(L, 0);
    TileRegs<typename A::Vec> qr, gr;
    float lse_r = 0.f, delta_r = 0.f;        // threads 0..31: one query's lse and delta of the tile in flight
    auto fetch = [&](int t) {
        qr = tile_load<typename A::Vec>(qbase, p.q_stride[0], t * kTile, p.len_q);
        gr = tile_load<typename A::Vec>(gbase, gs0, t * kTile, p.len_q);
        if (threadIdx.x < kTile) {
            const int qq = t * kTile + threadIdx.x;
            lse_r = qq < p.len_q ? lse_g[qq] : INFINITY;       // p = exp2(-inf) = 0 past the last query
            delta_r = qq < p.len_q ? delta_g[qq] : 0.f;
        }
    };
    if (qt < L.nqt) fetch(qt);
    while (qt < L.nqt) {
        __syncthreads();
        T.stage(qr, gr, p.scale);
        if (threadIdx.x < kTile) { lse_s[threadIdx.x] = lse_r; delta_s[threadIdx.x] = delta_r; }
        __syncthreads();
        const int cls = scan.cls(qt);
        const int nxt = scan.next(L, qt + 1);
        if (nxt < L.nqt) fetch(nxt);
        if (cls) {
            f32x16 s = A::over_d(T.q_d(), kf, c, h);         // S, dP: the lane's key against the queries R(r, h) of the tile
            f32x16 dp = A::over_d(T.g_d(), vf, c, h);
            const bool mixed = cls == 1 && p.mask && key < p.len_k;
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = row_of(r, h), qq = qt * kTile + qi;
                float pr = exp2_hw((A::late(s[r], p.scale) - lse_s[qi]) * kLog2e);
                if (mixed && qq < p.len_q && p.mask[(int64_t)qq * p.len_k + key]) pr = 0.f;
                s[r] = pr;
                dp[r] = pr * (dp[r] - delta_s[qi]);
            }
            dv = A::over_rows(T.g_rows(), s, dv, c, h);
            dk = A::over_rows(T.q_rows(), dp, dk, c, h);
        }
        qt = nxt;
    }
    if (key >= p.len_k) return;
    if (p.grad_k) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) dk[r] = A::late(dk[r], p.scale);
        A::row_store(static_cast<E *>(p.grad_k) + key * p.gk_stride[0] + b * p.gk_stride[1] + hd * kD, dk, h);
    }
    if (p.grad_v) A::row_store(static_cast<E *>(p.grad_v) + key * p.gv_stride[0] + b * p.gv_stride[1] + hd * kD, dv, h);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Host side: one plan, one launch helper per direction; what differs between the two entry-point pairs is data.
// ---------------------------------------------------------------------------------------------------------------------------
struct Rules {
    const char *op;            // in every message
    bool typed;                // the block's `type` is the caller's and must be a 16-bit code
    uintptr_t row, lse;        // alignment of a row's base in bytes; of lse
    const char *how;           // ... and how the message puts it
    const char *q_fwd, *q_bwd, *dkv;                         // the kernels' names in a launch failure
};
const Rules kF32 = {"self_attn", false, 16, 1, "(base and strides)", "sattn_q_kernel (forward)", "sattn_q_kernel (backward)", "sattn_dkv_kernel"};
const Rules kH16 = {"self_attn_h16", true, 8, 4, "(base, strides multiples of 4)", "sattn16_q_kernel (forward)", "sattn16_q_kernel (backward)",
                    "sattn16_dkv_kernel"};

size_t delta_bytes(int batch, int heads, int len_q) { return (((size_t)batch * heads * len_q * sizeof(float)) + 15) & ~(size_t)15; }

bool aligned(const void *ptr, uintptr_t to) { return ((uintptr_t)ptr & (to - 1)) == 0; }
bool rows_ok(const void *ptr, const int64_t *stride, uintptr_t to)
{
    return aligned(ptr, to) && stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0;
}

// Host-side check of the parameter block + launch geometry.  Returns SEMIDETR_OK or an error (message set).
int plan(const semidetr_self_attn_h16 *params, const Rules &R, void *workspace, size_t workspace_bytes, Launch &L, int for_backward)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "%s: null pointer (parameter block)", R.op);
    const semidetr_self_attn_h16 &p = params[0];
    SEMIDETR_REQUIRE(!R.typed || p.type == SEMIDETR_ROW_FP16 || p.type == SEMIDETR_ROW_BF16, SEMIDETR_E_BADARG,
                     "%s: element type %d (SEMIDETR_ROW_FP16 or SEMIDETR_ROW_BF16; fp32 rows take semidetr_self_attn_*_f32)", R.op, p.type);
    SEMIDETR_REQUIRE(p.head_dim == kD, SEMIDETR_E_BADARG, "%s: head dimension %d (only %d is built)", R.op, p.head_dim, kD);
    SEMIDETR_REQUIRE(p.batch > 0 && p.heads > 0 && p.len_q > 0 && p.len_k > 0, SEMIDETR_E_BADARG,
                     "%s: bad sizes (B=%d H=%d Lq=%d Lk=%d)", R.op, p.batch, p.heads, p.len_q, p.len_k);
    SEMIDETR_REQUIRE(p.scale == p.scale, SEMIDETR_E_BADARG, "%s: scale is NaN", R.op);
    SEMIDETR_REQUIRE((int64_t)p.batch * p.heads <= 65535 && (int64_t)p.len_q * p.len_k < ((int64_t)1 << 40) &&
                         (int64_t)p.len_q < (1 << 24) && (int64_t)p.len_k < (1 << 24) &&
                         (int64_t)((p.len_q + 31) / 32) * ((p.len_k + 31) / 32) < ((int64_t)1 << 31) &&
                         (int64_t)p.batch * p.heads * (p.len_q > p.len_k ? p.len_q : p.len_k) * kD < ((int64_t)1 << 40),
                     SEMIDETR_E_TOOLARGE, "%s: too large (B * H <= 65535, Lq and Lk < 2^24)", R.op);
    SEMIDETR_REQUIRE(p.q && p.k && p.v && p.out && p.lse, SEMIDETR_E_BADARG, "%s: null pointer (q / k / v / out / lse)", R.op);
    SEMIDETR_REQUIRE(rows_ok(p.q, p.q_stride, R.row) && rows_ok(p.k, p.k_stride, R.row) && rows_ok(p.v, p.v_stride, R.row) &&
                         aligned(p.out, R.row) && aligned(p.lse, R.lse),
                     SEMIDETR_E_BADARG, "%s: rows must be %d-byte aligned %s with non-negative strides", R.op, (int)R.row, R.how);
    if (for_backward) {
        SEMIDETR_REQUIRE(p.grad_out && aligned(p.grad_out, R.row), SEMIDETR_E_BADARG, "%s backward: null or misaligned grad_out", R.op);
        SEMIDETR_REQUIRE(p.grad_q || p.grad_k || p.grad_v, SEMIDETR_E_BADARG, "%s backward: no gradient asked for", R.op);
        SEMIDETR_REQUIRE((!p.grad_q || rows_ok(p.grad_q, p.gq_stride, R.row)) && (!p.grad_k || rows_ok(p.grad_k, p.gk_stride, R.row)) &&
                             (!p.grad_v || rows_ok(p.grad_v, p.gv_stride, R.row)),
                         SEMIDETR_E_BADARG, "%s backward: gradient rows must be %d-byte aligned %s", R.op, (int)R.row, R.how);
    }
    SEMIDETR_REQUIRE(workspace && aligned(workspace, 16) &&
                         workspace_bytes >= semidetr_self_attn_workspace_bytes(p.batch, p.heads, p.len_q, p.len_k),
                     SEMIDETR_E_BADARG, "%s: workspace null, misaligned or smaller than semidetr_self_attn_workspace_bytes()", R.op);
    L.p = p;
    L.nqt = (p.len_q + kTile - 1) / kTile;
    L.nkt = (p.len_k + kTile - 1) / kTile;
    L.delta = static_cast<float *>(workspace);
    L.cls = p.mask ? reinterpret_cast<uint8_t *>(workspace) + delta_bytes(p.batch, p.heads, p.len_q) : nullptr;
    return SEMIDETR_OK;
}

template <typename A>
int forward(hipStream_t st, const Launch &L, const Rules &R)
{
    const dim3 grid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn_q_kernel<A, false>), grid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status(R.q_fwd);
}

template <typename A>
int backward(hipStream_t st, const Launch &L, const Rules &R)
{
    const dim3 qgrid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn_q_kernel<A, true>), qgrid, dim3(kThreads), 0, st, L);
    if (int rc = semidetr::launch_status(R.q_bwd)) return rc;
    if (!L.p.grad_k && !L.p.grad_v) return SEMIDETR_OK;
    const dim3 kgrid((L.nkt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL((sattn_dkv_kernel<A>), kgrid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status(R.dkv);
}

// plan, tile classes, then the instance of the block's element type
int run(void *stream, const semidetr_self_attn_h16 *params, const Rules &R, void *workspace, size_t workspace_bytes, int for_backward)
{
    Launch L;
    if (int rc = plan(params, R, workspace, workspace_bytes, L, for_backward)) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    if (L.cls) {
        hipLaunchKernelGGL(sattn_class_kernel, dim3(L.nkt, L.nqt), dim3(64), 0, st, L.p.mask, L.p.len_q, L.p.len_k, L.nkt, const_cast<uint8_t *>(L.cls));
        if (int rc = semidetr::launch_status("sattn_class_kernel")) return rc;
    }
    switch (L.p.type) {
    case SEMIDETR_ROW_F32: return for_backward ? backward<ArithF32>(st, L, R) : forward<ArithF32>(st, L, R);
    case SEMIDETR_ROW_FP16: return for_backward ? backward<ArithH16<__half>>(st, L, R) : forward<ArithH16<__half>>(st, L, R);
    default: return for_backward ? backward<ArithH16<__hip_bfloat16>>(st, L, R) : forward<ArithH16<__hip_bfloat16>>(st, L, R);
    }
}

// the fp32 block as the kernels take it: every field, type = SEMIDETR_ROW_F32
const semidetr_self_attn_h16 *widen(const semidetr_self_attn *params, semidetr_self_attn_h16 &w)
{
    if (!params) return nullptr;
    const semidetr_self_attn &p = params[0];
    w = semidetr_self_attn_h16{};
    w.batch = p.batch, w.heads = p.heads, w.head_dim = p.head_dim, w.len_q = p.len_q, w.len_k = p.len_k, w.scale = p.scale;
    w.type = SEMIDETR_ROW_F32;
    w.q = p.q, w.k = p.k, w.v = p.v, w.mask = p.mask, w.out = p.out, w.lse = p.lse;
    w.grad_out = p.grad_out, w.grad_q = p.grad_q, w.grad_k = p.grad_k, w.grad_v = p.grad_v;
    for (int i = 0; i < 2; ++i) {
        w.q_stride[i] = p.q_stride[i], w.k_stride[i] = p.k_stride[i], w.v_stride[i] = p.v_stride[i];
        w.gq_stride[i] = p.gq_stride[i], w.gk_stride[i] = p.gk_stride[i], w.gv_stride[i] = p.gv_stride[i];
    }
    return &w;
}

}  // namespace

extern "C" size_t semidetr_self_attn_workspace_bytes(int batch, int heads, int len_q, int len_k)
{
    if (batch < 1 || heads < 1 || len_q < 1 || len_k < 1) return 0;
    return delta_bytes(batch, heads, len_q) + (size_t)((len_q + kTile - 1) / kTile) * (size_t)((len_k + kTile - 1) / kTile);
}

extern "C" int semidetr_self_attn_forward_f32(void *stream, const semidetr_self_attn *params, void *workspace, size_t workspace_bytes)
{
    semidetr_self_attn_h16 wide;
    return run(stream, widen(params, wide), kF32, workspace, workspace_bytes, 0);
}

extern "C" int semidetr_self_attn_backward_f32(void *stream, const semidetr_self_attn *params, void *workspace, size_t workspace_bytes)
{
    semidetr_self_attn_h16 wide;
    return run(stream, widen(params, wide), kF32, workspace, workspace_bytes, 1);
}

extern "C" int semidetr_self_attn_forward_h16(void *stream, const semidetr_self_attn_h16 *params, void *workspace, size_t workspace_bytes)
{
    return run(stream, params, kH16, workspace, workspace_bytes, 0);
}

extern "C" int semidetr_self_attn_backward_h16(void *stream, const semidetr_self_attn_h16 *params, void *workspace, size_t workspace_bytes)
{
    return run(stream, params, kH16, workspace, workspace_bytes, 1);
}

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
// Kernels (T16 = __half | __hip_bfloat16).  As in msda_fast.h, each fast kernel is ONE template over an IO policy that says where
// a sample's (x, y, attention) and its corner mask come from and where the backward puts the two small gradients:
//   LocAttnIO16   the reference op contract: fp32 locations and softmaxed weights in, fp32 grad_loc / grad_attn out
//                 (semidetr_msda_{forward,backward}_h16; reported as msda_fwd_h16<SPLIT / msda_bwd_h16);
//   RawIO16<PT>   the MSDeformAttn prologue / epilogue inside (semidetr_msda_fused_{forward,backward}_h16; reported as
//                 msda_fwd_h16_fused<SPLIT / msda_bwd_h16_fused): fp32 reference points, the RAW offsets and logits (PT = float |
//                 T16) and the padding mask bytes; softmax over L * P and ref + off * scale (msda_geom.h fused_loc_xy, the fp32
//                 kernels' code) in fp32; the write-back applies the softmax backward and the offset scale and rounds a 16-bit
//                 PT once.
//  * msda_fwd_h16<T16, IO, SPLIT>   32 channels per head, <= 32 heads, any query set.  The shape of msda_fwd_d32 (msda_fast.h):
//                                   phase 1 turns the tile's samples into LDS records {4 corner byte offsets, 4 weights};
//                                   phase 2 covers one 64-byte value row with 8 lanes x ONE 8-byte buffer load of 4 channels,
//                                   so lane -> channel map and fp32 accumulation order are msda_fwd_d32's (8 lanes x float4).
//  * msda_bwd_h16<T16, IO>          same shapes.  The shape of msda_bwd_d32: 32 lanes per value row (lane = channel), so every
//                                   global_atomic_add_f32 wave-instruction updates two complete 128-byte workspace rows;
//                                   channel sums for grad_attn / grad_loc by DPP inside the half-wave, staged in LDS.
//  * msda_h16_convert<T16>          fp32 workspace -> 16-bit grad_value, 8 elements (one 16-byte store) per thread.
//  * msda_{fwd,bwd}_h16_generic<T16> any D, any head count, any alignment: one wavefront per (n, q, m) row, lane per channel
//                                   (reference contract only: there is no generic fused kernel).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "common.h"

namespace semidetr_h16 {

#include "msda_geom.h"
#include "msda_lanes.h"              // dpp_mov, half32_sum, lp_group_max / lp_group_sum, Tile / tile_of_block: the fp32 kernels' own

constexpr int kD = 32;              // channels per head of the fast path
constexpr int kMaxLevels = 32;
thread_local const char *g_last_kernels = "";

#include "cvt16.h"                   // the two storage types: Cvt<T16>, unpack4, pack2, ld16, st16

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// IO policies of the fast kernels: what LocAttnIO / RawIO (msda_fast.h) are to the fp32 kernels, under the same names where the
// meaning is the same -- kSoftmax, record(...) (the record-building call), store(...).  Not merged with the fp32 structs: these
// store plainly (nothing streams), test the padding mask byte by byte (no summarised extents) and need no 32-bit image view.
//   begin_tile(...)  once per workgroup, by all threads: what the policy sets up for the tile (TileState)
//   record(...)      one sample of the tile -> its corner byte offsets (kOob: never loaded, no gradient), the bilinear fractions
//                    and the attention weight `a`; returns whether the sample is on the map
//   store(...)       the backward's write-back of one sample: res = {d/d a_k, d/d loc.x, d/d loc.y, a_k}, row_res = the L * P
//                    results of the same (n, q, m) row
//   softmax_lds      (host) LDS bytes beyond the records that `rows` query rows need
// ---------------------------------------------------------------------------------------------------------------------
struct LocAttnIO16 {
    const float *loc, *attn;        // (N, Lq, M, L, P, 2), (N, Lq, M, L * P): fp32, attn already holds probabilities
    float *gloc, *gattn;            // their gradients, fp32 and unrounded (backward; null in the forward)
    static constexpr bool kSoftmax = false;
    static constexpr const char *kFwd[3] = {"msda_fwd_h16<1", "msda_fwd_h16<2", "msda_fwd_h16<4"};      // by log2(SPLIT)
    static constexpr const char *kBwd = "msda_bwd_h16+msda_h16_convert";
    static size_t softmax_lds(int rows, int LP) { (void)rows; (void)LP; return 0; }
    struct TileState {};
    __device__ __forceinline__ TileState begin_tile(const Tile t, int rows, int M, int L, int P, int Lq, float *sm) const
    {
        (void)t; (void)rows; (void)M; (void)L; (void)P; (void)Lq; (void)sm;
        return TileState{};
    }
    // `live`: the thread has a sample slot and that slot's query row exists; l = k / P, the sample's level
    __device__ __forceinline__ bool record(const TileState &ts, const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                           bool in, bool live, int n, int q, int64_t row, int r, int k, int l, int S, int L, int P,
                                           unsigned row_bytes, unsigned (&off)[4], float &lw, float &lh, float &a) const
    {
        (void)ts; (void)in; (void)n; (void)q; (void)r; (void)S;
        off[0] = off[1] = off[2] = off[3] = kOob;      // out of range -> the hardware returns zeros
        lw = lh = a = 0.f;
        if (!live) return false;
        const int LP = L * P;
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
        const float2 xy = *reinterpret_cast<const float2 *>(loc + (row * LP + k) * 2);
        a = attn[row * LP + k];
        return sample_setup_oob(xy.x, xy.y, H, W, st, row_bytes, off, lw, lh);
    }
    // grad_attn_weight / grad_sampling_loc as they are
    __device__ __forceinline__ void store(const TileState &ts, int64_t row, int q, int k, int l, int L, int P, int H, int W,
                                          const float4 res, const float4 *row_res) const
    {
        (void)ts; (void)q; (void)l; (void)H; (void)W; (void)row_res;
        const int64_t i = row * (L * P) + k;
        gattn[i] = res.x;
        *reinterpret_cast<float2 *>(gloc + i * 2) = make_float2(res.y, res.z);
    }
};

// Offsets, logits and their gradients are PT = float or T16 (the C ABI's prologue_type); the softmax, the locations and every sum
// are fp32.
template <typename PT>
struct RawIO16 {
    const float *ref;               // (N, Lq, L, ref_dim), fp32 always: locations are never narrowed
    const PT *off, *logit;          // (N, Lq, M, L, P, 2), (N, Lq, M, L * P)
    const unsigned char *mask;      // (N, S) bytes, nonzero = padded pixel, or null
    int ref_dim;
    PT *goff, *glogit;              // gradients of off / logit (backward; null in the forward)
    static constexpr bool kSoftmax = true;      // logit holds raw logits: record() normalises the row across the lanes that own it
    static constexpr const char *kFwd[3] = {"msda_fwd_h16_fused<1", "msda_fwd_h16_fused<2", "msda_fwd_h16_fused<4"};
    static constexpr const char *kBwd = "msda_bwd_h16_fused+msda_h16_convert";
    // the softmax rows (logits, then exponentials) when L * P is no power of two (<= 64: check_fused)
    static size_t softmax_lds(int rows, int LP) { return (LP & (LP - 1)) == 0 ? 0 : (size_t)2 * rows * LP * sizeof(float); }

    // element access of the raw operands: a 16-bit offset pair is one dword (x in the low half)
    static constexpr bool kF32 = std::is_same<PT, float>::value;
    static __device__ __forceinline__ float2 ld_off(const PT *p, int64_t i)
    {
        if constexpr (kF32) {
            return *reinterpret_cast<const float2 *>(p + 2 * i);
        } else {
            const unsigned b = *reinterpret_cast<const unsigned *>(p + 2 * i);
            return make_float2(Cvt<PT>::up(b & 0xffffu), Cvt<PT>::up(b >> 16));
        }
    }
    static __device__ __forceinline__ float ld_logit(const PT *p, int64_t i)
    {
        if constexpr (kF32) return p[i];
        else return ld16(p + i);
    }
    static __device__ __forceinline__ void st_off(PT *p, int64_t i, float2 v)
    {
        if constexpr (kF32) *reinterpret_cast<float2 *>(p + 2 * i) = v;
        else *reinterpret_cast<unsigned *>(p + 2 * i) = pack2<PT>(v.x, v.y);
    }
    static __device__ __forceinline__ void st_logit(PT *p, int64_t i, float v)
    {
        if constexpr (kF32) p[i] = v;
        else st16(p + i, v);
    }

    struct TileState {
        __amdgpu_buffer_rsrc_t rr;      // the image's reference points: Lq * L * ref_dim floats
        const float *sm_e;              // exp(logit - row max) of the tile's samples in LDS (L * P no power of two)
    };
    // The reference point of (query, level) as {x, y, w, h}: one 8-byte buffer load for a point, two for a box -- branch-free: a
    // point's second load is sent out of range and returns zeros.
    __device__ __forceinline__ float4 ld_ref(const TileState &ts, int ql) const
    {
        const unsigned b = (unsigned)(ql * ref_dim) * 4u;
        const float2 c = buf_ld2(ts.rr, b), wh = buf_ld2(ts.rr, ref_dim == 4 ? b + 8u : kOob);
        return make_float4(c.x, c.y, wh.x, wh.y);
    }
    // For an L * P whose rows do not line up with the shuffle groups (five levels x four points = 20): exp(logit - row max) of every
    // sample of the tile into LDS.  sm: 2 x rows x LP floats; the exponentials are sm[rows * LP + s].  Ends with a barrier.
    __device__ __forceinline__ TileState begin_tile(const Tile t, int rows, int M, int L, int P, int Lq, float *sm) const
    {
        const int LP = L * P, total = rows * LP;
        if (!lp_shuffles(LP)) {
            for (int s = threadIdx.x; s < total; s += 256) {
                const int r = s / LP;
                sm[s] = t.q0 + r < Lq ? ld_logit(logit, (((int64_t)t.n * Lq + t.q0 + r) * M + t.m) * LP + (s - r * LP)) : 0.f;
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
        return TileState{image_rsrc(ref + (int64_t)t.n * Lq * L * ref_dim, (unsigned)(Lq * L * ref_dim) * 4u), sm + total};
    }
    // The softmax weight `a` of the sample (fp32, over the row's L * P logits), its location by msda_geom.h's fused_loc_xy, its
    // corners by sample_setup_oob, and a corner on a padded pixel -> kOob.  Called by ALL threads of the workgroup (the softmax
    // reduces across lanes); `in`: the thread has a sample slot, `live`: that slot's query row exists.  `a` is kept for samples
    // off the map too (the softmax backward needs every probability) and is 0 for a row that does not exist.
    __device__ __forceinline__ bool record(const TileState &ts, const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                           bool in, bool live, int n, int q, int64_t row, int r, int k, int l, int S, int L, int P,
                                           unsigned row_bytes, unsigned (&off)[4], float &lw, float &lh, float &a) const
    {
        const int LP = L * P;
        float2 o = make_float2(0.f, 0.f);
        float4 rp = make_float4(0.f, 0.f, 0.f, 0.f);
        float raw = 0.f;
        int H = 1, W = 1, st = 0;
        const bool shuf = lp_shuffles(LP);      // (workgroup-uniform)
        if (live) {
            o = ld_off(this->off, row * LP + k);
            if (shuf) raw = ld_logit(logit, row * LP + k);
            rp = ld_ref(ts, q * L + l);
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
                for (int j = 0; j < LP; ++j) sum += ts.sm_e[r * LP + j];      // fixed order
            a = in ? ts.sm_e[r * LP + k] * fast_rcp(sum) : 0.f;
        }
        off[0] = off[1] = off[2] = off[3] = kOob;
        lw = lh = 0.f;
        if (!live) {
            a = 0.f;
            return false;
        }
        float x, y;
        fused_loc_xy(o, rp, ref_dim, P, H, W, x, y);
        if (!sample_setup_oob(x, y, H, W, st, row_bytes, off, lw, lh)) return false;
        if (mask) {      // (x, y) -> top-left pixel exactly as sample_setup_oob derives it
            const int h0 = (int)floorf(sub_rn(mul_rn(y, (float)H), 0.5f)), w0 = (int)floorf(sub_rn(mul_rn(x, (float)W), 0.5f));
            const int pix = st + h0 * W + w0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int p = pix + (c & 1) + (c >> 1) * W;
                // (a level table that does not tile [0, S) must not reach past the mask)
                if (off[c] != kOob && ((unsigned)p >= (unsigned)S || mask[(int64_t)n * S + p] != 0)) off[c] = kOob;
            }
        }
        return true;
    }
    // The fused epilogue: the softmax backward grad_logits = a_k (g_k - sum_j a_j g_j) with the row's dot from LDS in a fixed order,
    // grad_offsets = grad_loc * scale; both rounded once when PT is 16-bit.
    __device__ __forceinline__ void store(const TileState &ts, int64_t row, int q, int k, int l, int L, int P, int H, int W,
                                          const float4 res, const float4 *row_res) const
    {
        const int LP = L * P;
        float dot = 0.f;
        for (int j = 0; j < LP; ++j) dot += row_res[j].w * row_res[j].x;
        const float2 sc = fused_loc_scale(ld_ref(ts, q * L + l), ref_dim, P, H, W);
        st_logit(glogit, row * LP + k, res.w * (res.x - dot));
        st_off(goff, row * LP + k, make_float2(res.y * sc.x, res.z * sc.y));
    }
};

// Phase 1 of both fast kernels: one record per sample of the tile's `rows` query rows, built by the policy and handed to
// put(record index, level, off, lw, lh, a, on the map).  Records of a row are LP + 1 apart: rows land on different LDS banks.
template <typename IO, typename Put>
__device__ __forceinline__ void tile_records(const IO &io, const typename IO::TileState &ts, const int64_t *__restrict__ shapes,
                                             const int64_t *__restrict__ starts, const Tile t, int rows, int S, int M, int L, int Lq,
                                             int P, Put put)
{
    const int LP = L * P, total = rows * LP;
    const unsigned row_bytes = (unsigned)(M * kD) * 2u;
    auto slot = [&](int s, bool in) {      // `in`: s is a sample of the tile
        const int r = in ? s / LP : 0, k = in ? s - r * LP : 0;
        const int q = t.q0 + r, l = k / P;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        unsigned off[4];
        float lw, lh, a;
        const bool on = io.record(ts, shapes, starts, in, in && q < Lq, t.n, q, row, r, k, l, S, L, P, row_bytes, off, lw, lh, a);
        if (in) put(r * (LP + 1) + k, l, off, lw, lh, a, on);
    };
    // (Two loop headers on purpose: as ONE uniform loop with an early exit, the reference contract's SPLIT 2 forward took 68 VGPRs
    //  instead of 42 and lost a wave -- profiles/msda_h16_one_template.txt.)
    if constexpr (IO::kSoftmax) {      // the softmax reduces across lanes: every thread walks every trip
        for (int s0 = 0; s0 < total; s0 += 256) slot(s0 + (int)threadIdx.x, s0 + (int)threadIdx.x < total);
    } else {
        for (int s = threadIdx.x; s < total; s += 256) slot(s, true);
    }
}

// Phase 2 of the D == 32 forward: gather + weighted sum in fp32 from the tile's LDS records, one 8-byte non-temporal store per lane.
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
// small query sets still fill the chip.  LDS: (32 / SPLIT) x (L * P + 1) records of 32 bytes + IO::softmax_lds.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T16, typename IO, int SPLIT>
__global__ __launch_bounds__(256) void msda_fwd_h16(const T16 *__restrict__ value, const int64_t *__restrict__ shapes,
                                                    const int64_t *__restrict__ starts, const IO io, int S, int M, int L, int Lq,
                                                    int P, int tiles_per_image, T16 *__restrict__ out)
{
    constexpr int RPB = 32 / SPLIT;
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1;
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_w = smem + RPB * LPP;
    const Tile t = tile_of_block(M, tiles_per_image, RPB);
    const auto ts = io.begin_tile(t, RPB, M, L, P, Lq, reinterpret_cast<float *>(smem + 2 * RPB * LPP));

    // ---- phase 1: sample records {4 corner byte offsets, 4 weights}
    tile_records(io, ts, shapes, starts, t, RPB, S, M, L, Lq, P,
                 [&](int i, int l, const unsigned (&off)[4], float lw, float lh, float a, bool on) {
                     (void)l;
                     float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                     if (on) {
                         const float hh = 1.f - lh, hw = 1.f - lw;
                         w = make_float4(a * (hh * hw), a * (hh * lw), a * (lh * hw), a * (lh * lw));
                     }
                     rec_off[i] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
                     rec_w[i] = w;
                 });
    __syncthreads();

    // ---- phase 2: gather + weighted sum in fp32
    fwd_gather_store<T16, SPLIT>(value, rec_off, rec_w, t, S, M, LP, LPP, Lq, out);
}

// Row phase of the D == 32 backward: each half-wave walks its rows' LDS records {corner offsets} / {lw, lh, a, level}: fp32
// atomics into the workspace, and the record overwritten with {g_attn, g_x, g_y, a}.
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
// LDS: rpb x (L * P + 1) x 2 records of 16 bytes + the level table + IO::softmax_lds.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T16, typename IO>
__global__ __launch_bounds__(256) void msda_bwd_h16(const T16 *__restrict__ gout, const T16 *__restrict__ value,
                                                    const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                    const IO io, int S, int M, int L, int Lq, int P, int tiles_per_image, int rpb,
                                                    float *__restrict__ gws)
{
    extern __shared__ float4 smem[];
    const int LP = L * P, LPP = LP + 1;
    int4 *rec_off = reinterpret_cast<int4 *>(smem);
    float4 *rec_p = smem + rpb * LPP;      // {lw, lh, a, level}; overwritten with {g_attn, g_x, g_y, a}
    float *lev_w = reinterpret_cast<float *>(smem + 2 * rpb * LPP), *lev_h = lev_w + kMaxLevels;
    const Tile t = tile_of_block(M, tiles_per_image, rpb);
    if (threadIdx.x < L) {
        lev_h[threadIdx.x] = (float)shapes[2 * threadIdx.x];
        lev_w[threadIdx.x] = (float)shapes[2 * threadIdx.x + 1];
    }
    const auto ts = io.begin_tile(t, rpb, M, L, P, Lq, lev_h + kMaxLevels);
    tile_records(io, ts, shapes, starts, t, rpb, S, M, L, Lq, P,
                 [&](int i, int l, const unsigned (&off)[4], float lw, float lh, float a, bool on) {
                     (void)on;
                     rec_off[i] = make_int4((int)off[0], (int)off[1], (int)off[2], (int)off[3]);
                     rec_p[i] = make_float4(lw, lh, a, __int_as_float(l));
                 });
    __syncthreads();

    bwd_rows<T16>(gout, value, rec_off, rec_p, lev_w, lev_h, t, S, M, LP, LPP, Lq, rpb, gws);
    __syncthreads();

    // ---- coalesced write-back of the two small gradients, in the policy's form
    for (int s = threadIdx.x; s < rpb * LP; s += 256) {
        const int r = s / LP, k = s - r * LP;
        const int q = t.q0 + r;
        if (q >= Lq) continue;
        const int64_t row = ((int64_t)t.n * Lq + q) * M + t.m;
        const int l = k / P;
        io.store(ts, row, q, k, l, L, P, (int)lev_h[l], (int)lev_w[l], rec_p[r * LPP + k], rec_p + r * LPP);
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
struct Dims {
    int N, S, M, D, L, Lq, P;
};

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

// LDS of a fast kernel with `rows` query rows: the records (+ the backward's level table) + what the policy's softmax takes
template <typename IO>
size_t fast_lds(int rows, int LP, bool backward)
{
    return (size_t)rows * (LP + 1) * 32 + (backward ? 2 * kMaxLevels * sizeof(float) : 0) + IO::softmax_lds(rows, LP);
}

// `what`: the C-ABI entry, for the error texts
template <typename T16, typename IO>
int launch_fast_forward(hipStream_t st, const T16 *value, const int64_t *shapes, const int64_t *starts, const IO &io, const Dims &d,
                        T16 *out, const char *what)
{
    const int LP = d.L * d.P;
    int split = semidetr::pick_split(0, d.N, d.Lq, d.M);      // the fp32 forward's rule
    while (split < 4 && fast_lds<IO>(32 / split, LP, false) > 64 * 1024) split *= 2;      // wide rows: fewer per workgroup
    const int rpb = 32 / split;
    const int tiles = (d.Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)d.N * tiles * d.M < INT32_MAX, SEMIDETR_E_TOOLARGE, "%s: grid too large", what);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((int64_t)d.N * tiles * d.M)), dim3(256), fast_lds<IO>(rpb, LP, false), st, value, shapes,
                           starts, io, d.S, d.M, d.L, d.Lq, d.P, tiles, out);
    };
    if (split == 1) launch(&msda_fwd_h16<T16, IO, 1>);
    else if (split == 2) launch(&msda_fwd_h16<T16, IO, 2>);
    else launch(&msda_fwd_h16<T16, IO, 4>);
    g_last_kernels = IO::kFwd[split >> 1];
    return semidetr::launch_status(g_last_kernels);
}

template <typename T16, typename IO>
int launch_fast_backward(hipStream_t st, const T16 *gout, const T16 *value, const int64_t *shapes, const int64_t *starts, const IO &io,
                         const Dims &d, float *ws, const char *what)
{
    const int LP = d.L * d.P;
    // 32 query rows per workgroup, 8 when that would not fill the chip or 32 rows of records would not fit 64 KB of LDS
    const int rpb = ((int64_t)d.N * d.M * ((d.Lq + 31) / 32) >= 1024 && fast_lds<IO>(32, LP, true) <= 64 * 1024) ? 32 : 8;
    const int tiles = (d.Lq + rpb - 1) / rpb;
    SEMIDETR_REQUIRE((int64_t)d.N * tiles * d.M < INT32_MAX, SEMIDETR_E_TOOLARGE, "%s: grid too large", what);
    const size_t lds = fast_lds<IO>(rpb, LP, true);
    // (a grant is asked for only above 64 KB: L * P = 254 at 8 rows, which only the reference contract admits)
    if (int rc = semidetr::allow_big_lds(&msda_bwd_h16<T16, IO>, lds, what)) return rc;
    hipLaunchKernelGGL((msda_bwd_h16<T16, IO>), dim3((unsigned)((int64_t)d.N * tiles * d.M)), dim3(256), lds, st, gout, value, shapes, starts,
                       io, d.S, d.M, d.L, d.Lq, d.P, tiles, rpb, ws);
    return semidetr::launch_status(IO::kBwd);
}

// The backward's last launch: workspace -> grad_value.  `kernels`: what the whole backward reports as its last kernels.
template <typename T16>
int convert_grad_value(hipStream_t st, const float *ws, const Dims &d, T16 *gvalue, const char *kernels, const char *what)
{
    const int64_t count = (int64_t)d.N * d.S * d.M * d.D;
    const int64_t blocks = (count + 2047) / 2048;
    SEMIDETR_REQUIRE(blocks < INT32_MAX, SEMIDETR_E_TOOLARGE, "%s: grad_value too large", what);
    if ((((uintptr_t)ws | (uintptr_t)gvalue) & 15) == 0)
        hipLaunchKernelGGL((msda_h16_convert<T16, true>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    else
        hipLaunchKernelGGL((msda_h16_convert<T16, false>), dim3((unsigned)blocks), dim3(256), 0, st, ws, count, gvalue);
    g_last_kernels = kernels;
    return semidetr::launch_status("msda_h16_convert");
}

// ---- reference contract: the fast kernels where fast_ok, the generic ones otherwise
template <typename T16>
int forward_impl(hipStream_t st, const T16 *value, const int64_t *shapes, const int64_t *starts, const LocAttnIO16 &io, const Dims &d,
                 T16 *out)
{
    if (fast_ok(value, out, io.loc, d.S, d.M, d.D, d.L, d.P))
        return launch_fast_forward(st, value, shapes, starts, io, d, out, "msda_forward_h16");
    const int64_t rows = (int64_t)d.N * d.Lq * d.M;
    hipLaunchKernelGGL(msda_fwd_h16_generic<T16>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, value, shapes, starts, io.loc, io.attn,
                       d.N, d.S, d.M, d.D, d.L, d.Lq, d.P, out);
    g_last_kernels = "msda_fwd_h16_generic";
    return semidetr::launch_status("msda_fwd_h16_generic");
}

template <typename T16>
int backward_impl(hipStream_t st, const T16 *gout, const T16 *value, const int64_t *shapes, const int64_t *starts, const LocAttnIO16 &io,
                  const Dims &d, float *ws, T16 *gvalue)
{
    const char *name = LocAttnIO16::kBwd;
    if (fast_ok(value, gout, io.loc, d.S, d.M, d.D, d.L, d.P) && (((uintptr_t)io.gloc) & 7) == 0) {
        if (int rc = launch_fast_backward(st, gout, value, shapes, starts, io, d, ws, "msda_backward_h16")) return rc;
    } else {
        const int64_t rows = (int64_t)d.N * d.Lq * d.M;
        hipLaunchKernelGGL(msda_bwd_h16_generic<T16>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, gout, value, shapes, starts, io.loc,
                           io.attn, d.N, d.S, d.M, d.D, d.L, d.Lq, d.P, ws, io.gloc, io.gattn);
        name = "msda_bwd_h16_generic+msda_h16_convert";
        if (int rc = semidetr::launch_status(name)) return rc;
    }
    return convert_grad_value(st, ws, d, gvalue, name, "msda_backward_h16");
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
    Dims dims() const { return Dims{N, S, M, D, L, Lq, P}; }
    template <typename PT>
    RawIO16<PT> io(void *goff, void *glogit) const
    {
        return RawIO16<PT>{ref, static_cast<const PT *>(off), static_cast<const PT *>(logit), mask, ref_dim, static_cast<PT *>(goff),
                           static_cast<PT *>(glogit)};
    }
};

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

// The run-time dtype and prologue_type as types: f(Type<T16>, Type<PT>) with T16 = __half | __hip_bfloat16 and PT = float
// (SEMIDETR_ROW_F32) | T16.  Both checked by the caller; the reference-contract entries have no PT and pass SEMIDETR_ROW_F32.
template <typename T>
struct Type {
    using type = T;
};
template <typename F>
int with_types(int dtype, int prologue_type, F f)
{
    const bool f32 = prologue_type == SEMIDETR_ROW_F32;
    if (dtype == SEMIDETR_H16_FP16) return f32 ? f(Type<__half>{}, Type<float>{}) : f(Type<__half>{}, Type<__half>{});
    return f32 ? f(Type<__hip_bfloat16>{}, Type<float>{}) : f(Type<__hip_bfloat16>{}, Type<__hip_bfloat16>{});
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
    return with_types(dtype, prologue_type, [&](auto t16, auto pt) {
        using T16 = typename decltype(t16)::type;
        using PT = typename decltype(pt)::type;
        return launch_fast_forward(semidetr::as_stream(stream), static_cast<const T16 *>(value), spatial_shapes, level_start,
                                   a.io<PT>(nullptr, nullptr), a.dims(), static_cast<T16 *>(out), "msda_fused_forward_h16");
    });
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
    return with_types(dtype, prologue_type, [&](auto t16, auto pt) {
        using T16 = typename decltype(t16)::type;
        using PT = typename decltype(pt)::type;
        const hipStream_t st = semidetr::as_stream(stream);
        const RawIO16<PT> io = a.io<PT>(grad_sampling_offsets, grad_attn_logits);
        float *ws = static_cast<float *>(workspace);
        if (int rc = launch_fast_backward(st, static_cast<const T16 *>(grad_out), static_cast<const T16 *>(value), spatial_shapes,
                                          level_start, io, a.dims(), ws, "msda_fused_backward_h16"))
            return rc;
        return convert_grad_value(st, ws, a.dims(), static_cast<T16 *>(grad_value), RawIO16<PT>::kBwd, "msda_fused_backward_h16");
    });
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
    const Dims d = {batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
    return with_types(dtype, SEMIDETR_ROW_F32, [&](auto t16, auto) {
        using T16 = typename decltype(t16)::type;
        return forward_impl(semidetr::as_stream(stream), static_cast<const T16 *>(value), spatial_shapes, level_start,
                            LocAttnIO16{sampling_loc, attn_weight, nullptr, nullptr}, d, static_cast<T16 *>(out));
    });
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
    const Dims d = {batch, spatial_size, num_heads, channels, num_levels, num_query, num_point};
    return with_types(dtype, SEMIDETR_ROW_F32, [&](auto t16, auto) {
        using T16 = typename decltype(t16)::type;
        return backward_impl(semidetr::as_stream(stream), static_cast<const T16 *>(grad_out), static_cast<const T16 *>(value), spatial_shapes,
                             level_start, LocAttnIO16{sampling_loc, attn_weight, grad_sampling_loc, grad_attn_weight}, d,
                             static_cast<float *>(workspace), static_cast<T16 *>(grad_value));
    });
}

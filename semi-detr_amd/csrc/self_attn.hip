// Decoder self-attention core for gfx950: out = softmax(scale * Q K^T + mask) V, forward and backward, head dimension 32
// (DINOTransformerDecoderLayer.forward_sa, detr_od/models/utils/transformer.py:975-1039: the nn.MultiheadAttention call
// without its two projections, which stay GEMMs).  fp32 in, fp32 arithmetic on the fp32-input MFMA (v_mfma_f32_32x32x2_f32, an
// exact k-ordered fmaf chain), fp32 out.  The (Lq, Lk) scores never reach memory.
//
//   sattn_class_kernel   one wave per 32 x 32 tile of the byte mask: 0 = every in-range element blocked, 2 = none, 1 = mixed
//                        (self_attn_tiles.h, shared with the 16-bit arithmetic of self_attn_h16.hip)
//   sattn_q_kernel<0>    forward: workgroup = 2 waves = 64 queries of one (image, head), wave = 32 queries; key tiles of 32
//                        through LDS
//   sattn_q_kernel<1>    backward, same geometry: delta_i = sum_d dO_id O_id (written for the next launch), P = exp(s - lse), dQ
//   sattn_dkv_kernel     workgroup = 2 waves = 64 keys, wave = 32 keys; query tiles of 32 through LDS; dK and dV
// A key tile of class 0 for both waves of a workgroup is neither staged nor multiplied; a wave skips the matrix work of a tile
// of class 0 for its own 32 rows; a tile of class 2 reads no mask byte.  No float atomics, no memset, every sum in a fixed
// order: bitwise reproducible.
//
// Data flow (lane l: c = l & 31, h = l >> 5; register r of an accumulator is row R(r, h) = (r & 3) + 8 (r >> 2) + 4 h):
//   forward / dQ   S^T = K Qs^T  (A = K[key c][d = 2 s + h] from LDS, B = Qs[query c][2 s + h] in 16 registers, s = 0..15), so a
//                  lane owns one query and its registers are 16 keys: row maximum and row sum are in-lane plus one exchange
//                  with lane l ^ 32.  O^T = V^T P^T sums over S^T's register index: step r takes B = P^T register r and
//                  A = V[key R(r, h)][d = c].  dQ^T = K^T dS^T likewise with A = K[key R(r, h)][d = c].
//   dK, dV         S = Qs K^T with the key on the lane (A = Qs[query c][2 s + h] from LDS, B = K[key c][2 s + h] in registers),
//                  dP = dO V^T the same way; dV^T += dO^T P and dK^T += Qs^T dS take P / dS registers as B and
//                  A = dO / Qs[query R(r, h)][d = c].
// Arithmetic, in this order (tests/self_attn_ref64.py bounds it): Qs = q * scale (one rounding); s = fma chain over d = 0..31;
//   per key tile: m' = max(m, max_j s_j); p_j = exp2((s_j - m') * log2e) (v_exp_f32); l = l * exp2((m - m') * log2e) + sum_j p_j;
//   O = O * exp2((m - m') * log2e) then the fma chain over the tile's keys; out = O / l; lse = m + logf(l).
//   backward: p = exp2((s - lse) * log2e), dS = p * (dP - delta), dQ = (fma chain of dS k) * scale, dK = fma chain of dS Qs.
// A row whose every key is blocked gives NaN in `out` (torch's softmax of a row of -inf); its backward is outside the contract.
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

namespace {

#include "self_attn_tiles.h"

constexpr int kPad = kD + 1;                 // LDS row stride of an image read down a column of lanes (A = X[row c][d])

struct Launch : Tiles {
    semidetr_self_attn p;
    float *delta;              // (B, H, Lq)
};

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// A tile of 32 rows x 32 floats of `base` (row stride s0 elements, rows from row0, valid below `rows`) in the registers of the
// workgroup's 128 threads: two float4 per thread; rows past the end read as zeros.
struct TileRegs { float4 v[2]; };

__device__ __forceinline__ TileRegs tile_load(const float *base, int64_t s0, int row0, int rows)
{
    TileRegs t;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
        t.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < rows) t.v[i] = *reinterpret_cast<const float4 *>(base + (int64_t)(row0 + row) * s0 + 4 * c4);
    }
    return t;
}

__device__ __forceinline__ void tile_store(float *lds, const TileRegs &t, float mul)
{
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * kThreads, row = idx >> 3, c4 = idx & 7;
        float *d = lds + row * kPad + 4 * c4;
        d[0] = t.v[i].x * mul; d[1] = t.v[i].y * mul; d[2] = t.v[i].z * mul; d[3] = t.v[i].w * mul;
    }
}

// the 16 elements d = 2 s + h of a row, times mul
__device__ __forceinline__ void row_load(float (&dst)[16], const float *row, int h, float mul)
{
    #pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(row + 4 * i);
        dst[2 * i] = (h ? v.y : v.x) * mul;
        dst[2 * i + 1] = (h ? v.w : v.z) * mul;
    }
}

// S^T of a staged key tile: blocked elements (mask byte, key past the end) come back as -inf
__device__ __forceinline__ f32x16 scores_t(const Launch &L, const float *Ks, const float (&qreg)[16], int c, int h, int kt, int cls,
                                           int qc)
{
    f32x16 s = {0};
    #pragma unroll
    for (int i = 0; i < 16; ++i) s = mfma(Ks[c * kPad + 2 * i + h], qreg[i], s);
    const int Lk = L.p.len_k;
    if (cls == 1 || kt * kTile + kTile > Lk) {
        const uint8_t *mrow = (L.p.mask && cls == 1) ? L.p.mask + (int64_t)qc * Lk : nullptr;
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * kTile + row_of(r, h);
            bool blocked = key >= Lk;
            if (!blocked && mrow) blocked = mrow[key] != 0;
            if (blocked) s[r] = -INFINITY;
        }
    }
    return s;
}

// 16 accumulator registers (d = R(r, h)) of the lane's row -> four float4 at dst[8 g + 4 h]
__device__ __forceinline__ void row_store(float *dst, const f32x16 &o, int h)
{
    #pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4 *>(dst + 8 * g + 4 * h) = make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
}

template <bool BACKWARD>
__global__ __launch_bounds__(kThreads) void sattn_q_kernel(const Launch L)
{
    __shared__ float Ks[kTile * kPad], Vs[kTile * kPad];
    const semidetr_self_attn &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int qt0 = blockIdx.x * kWaves, qt = qt0 + wv;
    const int q = qt * kTile + c, qc = q < p.len_q ? q : p.len_q - 1;
    const int64_t lse_at = (int64_t)bh * p.len_q + qc;

    float qreg[16], dreg[16];
    row_load(qreg, p.q + qc * p.q_stride[0] + b * p.q_stride[1] + hd * kD, h, p.scale);
    float delta = 0.f, lse = 0.f;
    if (BACKWARD) {
        float oreg[16];
        const int64_t at = ((int64_t)qc * p.batch + b) * (p.heads * kD) + hd * kD;
        row_load(dreg, p.grad_out + at, h, 1.f);
        row_load(oreg, p.out + at, h, 1.f);
        #pragma unroll
        for (int i = 0; i < 16; ++i) delta += dreg[i] * oreg[i];
        delta += __shfl_xor(delta, 32, 64);
        lse = p.lse[lse_at];
        if (h == 0 && q < p.len_q) L.delta[lse_at] = delta;
        if (!p.grad_q) return;
    }

    const float *kbase = p.k + b * p.k_stride[1] + hd * kD, *vbase = p.v + b * p.v_stride[1] + hd * kD;
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
        tile_store(Ks, kr, 1.f);
        tile_store(Vs, vr, 1.f);
        __syncthreads();
        const int cls = scan.cls(kt);
        const int nxt = scan.next(L, kt + 1);
        if (nxt < L.nkt) {
            kr = tile_load(kbase, p.k_stride[0], nxt * kTile, p.len_k);
            vr = tile_load(vbase, p.v_stride[0], nxt * kTile, p.len_k);
        }
        if (cls) {
            f32x16 s = scores_t(L, Ks, qreg, c, h, kt, cls, qc);
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
                for (int r = 0; r < 16; ++r) acc = mfma(Vs[row_of(r, h) * kPad + c], s[r], acc);
            } else {
                f32x16 dp = {0};
                #pragma unroll
                for (int i = 0; i < 16; ++i) dp = mfma(Vs[c * kPad + 2 * i + h], dreg[i], dp);
                #pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = exp2_hw((s[r] - lse) * kLog2e) * (dp[r] - delta);
                #pragma unroll
                for (int r = 0; r < 16; ++r) acc = mfma(Ks[row_of(r, h) * kPad + c], s[r], acc);
            }
        }
        kt = nxt;
    }
    if (q >= p.len_q) return;
    if (!BACKWARD) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] / l;
        row_store(p.out + ((int64_t)q * p.batch + b) * (p.heads * kD) + hd * kD, acc, h);
        if (h == 0) p.lse[lse_at] = m + logf(l);
    } else {
        #pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= p.scale;
        row_store(p.grad_q + q * p.gq_stride[0] + b * p.gq_stride[1] + hd * kD, acc, h);
    }
}

__global__ __launch_bounds__(kThreads) void sattn_dkv_kernel(const Launch L)
{
    __shared__ float Qs[kTile * kPad], Gs[kTile * kPad], lse_s[kTile], delta_s[kTile];
    const semidetr_self_attn &p = L.p;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int bh = blockIdx.y, b = bh / p.heads, hd = bh - b * p.heads;
    const int kt0 = blockIdx.x * kWaves, kt = kt0 + wv;
    const int key = kt * kTile + c, kc = key < p.len_k ? key : p.len_k - 1;

    float kreg[16], vreg[16];
    row_load(kreg, p.k + kc * p.k_stride[0] + b * p.k_stride[1] + hd * kD, h, 1.f);
    row_load(vreg, p.v + kc * p.v_stride[0] + b * p.v_stride[1] + hd * kD, h, 1.f);
    const float *qbase = p.q + b * p.q_stride[1] + hd * kD;
    const float *gbase = p.grad_out + (int64_t)b * (p.heads * kD) + hd * kD;
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
        tile_store(Qs, qr, p.scale);
        tile_store(Gs, gr, 1.f);
        if (threadIdx.x < kTile) { lse_s[threadIdx.x] = lse_r; delta_s[threadIdx.x] = delta_r; }
        __syncthreads();
        const int cls = scan.cls(qt);
        const int nxt = scan.next(L, qt + 1);
        if (nxt < L.nqt) fetch(nxt);
        if (cls) {
            f32x16 s = {0}, dp = {0};
            #pragma unroll
            for (int i = 0; i < 16; ++i) s = mfma(Qs[c * kPad + 2 * i + h], kreg[i], s);
            #pragma unroll
            for (int i = 0; i < 16; ++i) dp = mfma(Gs[c * kPad + 2 * i + h], vreg[i], dp);
            const bool mixed = cls == 1 && p.mask && key < p.len_k;
            #pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qi = row_of(r, h), qq = qt * kTile + qi;
                float pr = exp2_hw((s[r] - lse_s[qi]) * kLog2e);
                if (mixed && qq < p.len_q && p.mask[(int64_t)qq * p.len_k + key]) pr = 0.f;
                s[r] = pr;
                dp[r] = pr * (dp[r] - delta_s[qi]);
            }
            #pragma unroll
            for (int r = 0; r < 16; ++r) dv = mfma(Gs[row_of(r, h) * kPad + c], s[r], dv);
            #pragma unroll
            for (int r = 0; r < 16; ++r) dk = mfma(Qs[row_of(r, h) * kPad + c], dp[r], dk);
        }
        qt = nxt;
    }
    if (key >= p.len_k) return;
    if (p.grad_k) row_store(p.grad_k + key * p.gk_stride[0] + b * p.gk_stride[1] + hd * kD, dk, h);
    if (p.grad_v) row_store(p.grad_v + key * p.gv_stride[0] + b * p.gv_stride[1] + hd * kD, dv, h);
}

bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }
bool rows_ok(const void *ptr, const int64_t *stride) { return aligned16(ptr) && stride[0] >= 0 && stride[1] >= 0 && stride[0] % 4 == 0 && stride[1] % 4 == 0; }

// Host-side check of the parameter block + launch geometry.  Returns SEMIDETR_OK or an error (message set).
int plan(const semidetr_self_attn *params, void *workspace, size_t workspace_bytes, Launch &L, int for_backward)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "self_attn: null pointer (parameter block)");
    const semidetr_self_attn &p = params[0];
    SEMIDETR_REQUIRE(p.head_dim == kD, SEMIDETR_E_BADARG, "self_attn: head dimension %d (only %d is built)", p.head_dim, kD);
    if (int rc = sizes_ok(p, "self_attn")) return rc;
    SEMIDETR_REQUIRE(p.q && p.k && p.v && p.out && p.lse, SEMIDETR_E_BADARG, "self_attn: null pointer (q / k / v / out / lse)");
    SEMIDETR_REQUIRE(rows_ok(p.q, p.q_stride) && rows_ok(p.k, p.k_stride) && rows_ok(p.v, p.v_stride) && aligned16(p.out),
                     SEMIDETR_E_BADARG, "self_attn: rows must be 16-byte aligned (base and strides) with non-negative strides");
    if (for_backward) {
        SEMIDETR_REQUIRE(p.grad_out && aligned16(p.grad_out), SEMIDETR_E_BADARG, "self_attn backward: null or misaligned grad_out");
        SEMIDETR_REQUIRE(p.grad_q || p.grad_k || p.grad_v, SEMIDETR_E_BADARG, "self_attn backward: no gradient asked for");
        SEMIDETR_REQUIRE((!p.grad_q || rows_ok(p.grad_q, p.gq_stride)) && (!p.grad_k || rows_ok(p.grad_k, p.gk_stride)) &&
                             (!p.grad_v || rows_ok(p.grad_v, p.gv_stride)),
                         SEMIDETR_E_BADARG, "self_attn backward: gradient rows must be 16-byte aligned (base and strides)");
    }
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) &&
                         workspace_bytes >= semidetr_self_attn_workspace_bytes(p.batch, p.heads, p.len_q, p.len_k),
                     SEMIDETR_E_BADARG, "self_attn: workspace null, misaligned or smaller than semidetr_self_attn_workspace_bytes()");
    L.p = p;
    carve(p, workspace, L, L.delta);
    return SEMIDETR_OK;
}

}  // namespace

extern "C" size_t semidetr_self_attn_workspace_bytes(int batch, int heads, int len_q, int len_k)
{
    if (batch < 1 || heads < 1 || len_q < 1 || len_k < 1) return 0;
    return delta_bytes(batch, heads, len_q) + (size_t)((len_q + kTile - 1) / kTile) * (size_t)((len_k + kTile - 1) / kTile);
}

extern "C" int semidetr_self_attn_forward_f32(void *stream, const semidetr_self_attn *params, void *workspace,
                                              size_t workspace_bytes)
{
    Launch L;
    if (int rc = plan(params, workspace, workspace_bytes, L, 0)) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    if (int rc = launch_class(st, L, L.p.mask, L.p.len_q, L.p.len_k)) return rc;
    const dim3 grid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL(sattn_q_kernel<false>, grid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status("sattn_q_kernel (forward)");
}

extern "C" int semidetr_self_attn_backward_f32(void *stream, const semidetr_self_attn *params, void *workspace,
                                               size_t workspace_bytes)
{
    Launch L;
    if (int rc = plan(params, workspace, workspace_bytes, L, 1)) return rc;
    hipStream_t st = semidetr::as_stream(stream);
    if (int rc = launch_class(st, L, L.p.mask, L.p.len_q, L.p.len_k)) return rc;
    const dim3 qgrid((L.nqt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL(sattn_q_kernel<true>, qgrid, dim3(kThreads), 0, st, L);
    if (int rc = semidetr::launch_status("sattn_q_kernel (backward)")) return rc;
    if (!L.p.grad_k && !L.p.grad_v) return SEMIDETR_OK;
    const dim3 kgrid((L.nkt + kWaves - 1) / kWaves, L.p.batch * L.p.heads);
    hipLaunchKernelGGL(sattn_dkv_kernel, kgrid, dim3(kThreads), 0, st, L);
    return semidetr::launch_status("sattn_dkv_kernel");
}

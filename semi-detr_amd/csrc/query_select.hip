// Two-stage query selection of DINO (include/semidetr_hip.h, "Two-stage query selection").
//
// Between the encoder and the decoder the reference runs ~40 small torch ops per level plus two masked_fill passes over the
// (N, S, d_model) memory, a max over the classes, torch.topk over all tokens and three gathers with expanded indices
// (detr_od/models/utils/transformer.py:525-575, 1315-1346, 1398).  Here:
//   qsel_proposals_kernel       anchors + masked copy of the memory + a valid byte per token, one read and one write of the
//                               memory at 16 bytes per lane (valid_H / valid_W counted per workgroup from the <= H + W mask
//                               bytes of the levels its tokens touch)
//   qsel_mask_rows_kernel       its backward
//   qsel_rowmax_kernel          key = max over the classes as an order-preserving 32-bit integer, spread over all CUs
//   qsel_topk_kernel            per image: radix select of the k largest keys out of LDS (out of the workspace for a large
//                               S), ties by the lower token index, bitonic sort of the k survivors, inverse map
//   qsel_gather_kernel          the three gathers and the two sigmoids
//   qsel_gather_bwd_kernel      dense gradients through the inverse map: every row written once, no memset, no atomics
// The order (key descending, token ascending) is total, so the selection is deterministic where torch.topk's is not: all
// padded tokens have bit-identical logits.
#include "common.h"
#include "select.h"

namespace {

using semidetr::kHistStride;
using semidetr::order_key;
using semidetr::sigmoidf_;

constexpr int kThreads = 256;
constexpr int kTile = 64;                     // tokens per workgroup of the streaming kernels
constexpr int kTopThreads = 1024;
constexpr int kHistCopies = 16;
constexpr size_t kLdsBudget = 160 * 1024 - 2048;      // dynamic LDS of the top-k kernel; the rest is its static part

struct Levels {
    int num;
    int h[SEMIDETR_QSEL_MAX_LEVELS], w[SEMIDETR_QSEL_MAX_LEVELS];
    const int64_t *dev;                       // (num, 2) int64 on the device, or null: h / w above hold
};

__device__ inline void level_hw(const Levels &lv, int l, int S, int &H, int &W)
{
    int64_t h = lv.dev ? lv.dev[2 * l] : lv.h[l], w = lv.dev ? lv.dev[2 * l + 1] : lv.w[l];
    if (h < 1 || w < 1 || h > S || w > S || h * w > S) h = w = 0;      // a level that cannot lie in S tokens: no tokens
    H = (int)h, W = (int)w;
}

// ---- anchors + masked memory.  grid (ceil(S / kTile), N)
__global__ __launch_bounds__(kThreads) void qsel_proposals_kernel(const float *__restrict__ memory,
                                                                 const unsigned char *__restrict__ mask, const Levels lv,
                                                                 int S, int D, int vec4, float *__restrict__ out_memory,
                                                                 float *__restrict__ proposals,
                                                                 unsigned char *__restrict__ valid)
{
    __shared__ int s_cnt[SEMIDETR_QSEL_MAX_LEVELS][2];
    __shared__ int s_start[SEMIDETR_QSEL_MAX_LEVELS + 1], s_H[SEMIDETR_QSEL_MAX_LEVELS], s_W[SEMIDETR_QSEL_MAX_LEVELS];
    __shared__ unsigned char s_valid[kTile];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int s0 = blockIdx.x * kTile;
    const int s1 = s0 + kTile < S ? s0 + kTile : S;
    const unsigned char *m = mask + (int64_t)n * S;
    if (tid == 0) {
        int at = 0;
        for (int l = 0; l < lv.num; ++l) {
            int H, W;
            level_hw(lv, l, S, H, W);
            if ((int64_t)at + (int64_t)H * W > S) H = W = 0;
            s_start[l] = at, s_H[l] = H, s_W[l] = W;
            at += H * W;
        }
        s_start[lv.num] = at;
    }
    if (tid < 2 * SEMIDETR_QSEL_MAX_LEVELS) s_cnt[tid >> 1][tid & 1] = 0;
    __syncthreads();
    // valid_H = unmasked entries of column 0, valid_W = of row 0 (transformer.py:542-543), for the levels of this tile
    for (int l = 0; l < lv.num; ++l) {
        const int a = s_start[l], b = s_start[l + 1];
        if (b <= s0 || a >= s1) continue;                              // uniform
        const int H = s_H[l], W = s_W[l];
        for (int i = tid; i < H + W; i += kThreads) {
            const int pos = i < H ? a + i * W : a + (i - H);
            if (pos < S && !m[pos]) atomicAdd(&s_cnt[l][i < H ? 0 : 1], 1);
        }
    }
    __syncthreads();
    if (tid < kTile && s0 + tid < S) {
        const int s = s0 + tid;
        int l = -1;
        for (int j = 0; j < lv.num; ++j)
            if (s >= s_start[j] && s < s_start[j + 1]) l = j;
        bool ok = false;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l >= 0) {
            const int W = s_W[l], local = s - s_start[l];
            const int y = local / W, x = local - y * W;
            // IEEE correctly rounded quotients: the flag below then equals the reference's fp32 run bit for bit
            const float px = __fdiv_rn((float)x + 0.5f, (float)s_cnt[l][1]);
            const float py = __fdiv_rn((float)y + 0.5f, (float)s_cnt[l][0]);
            const float wh = 0.05f * (float)(1 << l);
            ok = px > 0.01f && px < 0.99f && py > 0.01f && py < 0.99f && wh > 0.01f && wh < 0.99f && !m[s];
            if (ok) {
                const float lw = logf(__fdiv_rn(wh, 1.f - wh));
                q = make_float4(logf(__fdiv_rn(px, 1.f - px)), logf(__fdiv_rn(py, 1.f - py)), lw, lw);
            }
        }
        const float inf = __builtin_inff();
        if (!ok) q = make_float4(inf, inf, inf, inf);
        *reinterpret_cast<float4 *>(proposals + 4 * ((int64_t)n * S + s)) = q;
        valid[(int64_t)n * S + s] = ok;
        s_valid[tid] = ok;
    }
    __syncthreads();
    const int64_t base = ((int64_t)n * S + s0) * D;
    if (vec4) {
        const int q4 = D >> 2, total = (s1 - s0) * q4;
        const float4 *src = reinterpret_cast<const float4 *>(memory + base);
        float4 *dst = reinterpret_cast<float4 *>(out_memory + base);
        for (int e = tid; e < total; e += kThreads)
            dst[e] = s_valid[e / q4] ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const int total = (s1 - s0) * D;
        for (int e = tid; e < total; e += kThreads) out_memory[base + e] = s_valid[e / D] ? memory[base + e] : 0.f;
    }
}

// ---- grad_memory = valid ? grad_output_memory : 0.  grid ceil(rows / kTile)
__global__ __launch_bounds__(kThreads) void qsel_mask_rows_kernel(const float *__restrict__ grad, const unsigned char *__restrict__ valid,
                                                                 int64_t rows, int D, int vec4, float *__restrict__ out)
{
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kTile;
    const int nrow = rows - r0 < kTile ? (int)(rows - r0) : kTile;
    const int64_t base = r0 * D;
    if (vec4) {
        const int q4 = D >> 2, total = nrow * q4;
        const float4 *src = reinterpret_cast<const float4 *>(grad + base);
        float4 *dst = reinterpret_cast<float4 *>(out + base);
        for (int e = tid; e < total; e += kThreads)
            dst[e] = valid[r0 + e / q4] ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const int total = nrow * D;
        for (int e = tid; e < total; e += kThreads) out[base + e] = valid[r0 + e / D] ? grad[base + e] : 0.f;
    }
}

// ---- key = max over the classes, as the integer that orders like the float (order_key, select.h)
__device__ inline float max_nan(float m, float v) { return (m != m) ? m : ((v != v || v > m) ? v : m); }

// 16 lanes per row, four rows per wavefront and pass.  grid ceil(rows / 16)
__global__ __launch_bounds__(kThreads) void qsel_rowmax_kernel(const float *__restrict__ logits, int64_t rows, int C, int vec4,
                                                              unsigned *__restrict__ keys)
{
    const int sub = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / 16) + (threadIdx.x >> 4);
    float m = -__builtin_inff();
    if (row < rows) {
        const float *p = logits + row * C;
        if (vec4) {
            const float4 *p4 = reinterpret_cast<const float4 *>(p);
            for (int c = sub; c < (C >> 2); c += 16) {
                const float4 v = p4[c];
                m = max_nan(max_nan(max_nan(max_nan(m, v.x), v.y), v.z), v.w);
            }
        } else {
            for (int c = sub; c < C; c += 16) m = max_nan(m, p[c]);
        }
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) m = max_nan(m, __shfl_xor(m, d, 64));
    if (row < rows && sub == 0) keys[row] = order_key(m);
}

// ---- per image: the k largest keys sorted by (key descending, token ascending) + the inverse map.  grid N.
// dynamic LDS: sel[kcap] (64-bit), hist, then the S keys when they fit (in_lds).
__global__ __launch_bounds__(kTopThreads) void qsel_topk_kernel(const unsigned *__restrict__ keys_g, int S, int k, int kcap,
                                                               int in_lds, int64_t *__restrict__ indices,
                                                               int32_t *__restrict__ inverse)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long qsel_smem[];
    __shared__ int bins[256];
    __shared__ int s_wave[kTopThreads / 64];
    __shared__ int s_digit, s_remaining, s_fill, s_base;
    unsigned long long *sel = qsel_smem;
    int *hist = reinterpret_cast<int *>(sel + kcap);
    unsigned *keys_l = reinterpret_cast<unsigned *>(hist + kHistCopies * kHistStride);
    const int n = blockIdx.x, tid = threadIdx.x;
    const unsigned *kg = keys_g + (int64_t)n * S;
    int32_t *inv = inverse + (int64_t)n * S;
    for (int i = tid; i < S; i += kTopThreads) {
        if (in_lds) keys_l[i] = kg[i];
        inv[i] = -1;
    }
    for (int i = tid; i < kcap; i += kTopThreads) sel[i] = 0;
    if (tid == 0) { s_fill = 0; s_remaining = k; s_base = 0; }
    __syncthreads();
    const unsigned *keys = in_lds ? keys_l : kg;
    // radix select, most significant byte first: after four passes `prefix` is the k-th largest key and s_remaining the
    // number of tokens with exactly that key which belong to the selection
    unsigned prefix = 0, pmask = 0;
    for (int pass = 3; pass >= 0; --pass) {
        semidetr::histogram_pass<kTopThreads, kHistCopies>(hist, keys, S, prefix, pmask, pass);
        // 1 <= s_remaining <= words counted: it starts as k in [1, S] (launcher) against all S keys, and every pass leaves the
        // rank inside the chosen digit, whose keys are the next pass's
        semidetr::pick_digit<kTopThreads, kHistCopies>(hist, bins, &s_digit, &s_remaining);
        prefix |= (unsigned)s_digit << (8 * pass);
        pmask |= 0xFFu << (8 * pass);
    }
    const int ties = s_remaining;
    // every key above the k-th and the first `ties` tokens, in token order, that equal it; then the kcap slots sorted (the
    // unused ones are 0 and sink to the end)
    semidetr::collect_with_ties<kTopThreads>(keys, S, prefix, ties, s_wave, &s_base, [&](int i, unsigned u) {
        sel[atomicAdd(&s_fill, 1)] = ((unsigned long long)u << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
    });
    semidetr::bitonic_desc<kTopThreads>(sel, kcap);
    for (int r = tid; r < k; r += kTopThreads) {
        const unsigned i = 0xFFFFFFFFu - (unsigned)(sel[r] & 0xFFFFFFFFull);
        indices[(int64_t)n * k + r] = (int64_t)i;
        if (i < (unsigned)S) inv[i] = r;           // behind the barriers above: ordered after this workgroup's -1
    }
}

// ---- the gathers: one wavefront per (image, slot).  grid ceil(N * k / 4)
__global__ __launch_bounds__(kThreads) void qsel_gather_kernel(const int64_t *__restrict__ indices, const float *__restrict__ coord,
                                                              const float *__restrict__ proposals,
                                                              const float *__restrict__ memory, int rows, int S, int k, int D,
                                                              int vec4, float *__restrict__ refpoint,
                                                              float *__restrict__ init_box, float *__restrict__ tgt,
                                                              float *__restrict__ ref_enc)
{
    const int row = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int n = row / k;
    const int64_t s = indices[row];
    const bool ok = s >= 0 && s < S;
    const int64_t from = (int64_t)n * S + (ok ? s : 0);
    const float nan = __builtin_nanf("");
    if (tgt) {
        const float *src = memory + from * D;
        float *dst = tgt + (int64_t)row * D;
        if (vec4) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src);
            float4 *d4 = reinterpret_cast<float4 *>(dst);
            for (int c = lane; c < (D >> 2); c += 64) d4[c] = ok ? s4[c] : make_float4(nan, nan, nan, nan);
        } else {
            for (int c = lane; c < D; c += 64) dst[c] = ok ? src[c] : nan;
        }
    }
    if (lane < 4) {
        const float c = ok ? coord[from * 4 + lane] : nan;
        refpoint[(int64_t)row * 4 + lane] = c;
        ref_enc[(int64_t)row * 4 + lane] = sigmoidf_(c);
        init_box[(int64_t)row * 4 + lane] = sigmoidf_(ok ? proposals[from * 4 + lane] : nan);
    }
}

// ---- backward of the gathers.  grid (ceil(S / kTile), N); every row of both outputs written once
__global__ __launch_bounds__(kThreads) void qsel_gather_bwd_kernel(const int32_t *__restrict__ inverse,
                                                                  const float *__restrict__ g_refpoint,
                                                                  const float *__restrict__ g_tgt,
                                                                  const float *__restrict__ g_ref_enc,
                                                                  const float *__restrict__ ref_enc, int S, int k, int D,
                                                                  int vec4, float *__restrict__ grad_coord,
                                                                  float *__restrict__ grad_memory)
{
    __shared__ int s_slot[kTile];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int s0 = blockIdx.x * kTile;
    const int s1 = s0 + kTile < S ? s0 + kTile : S;
    if (tid < kTile) {
        int slot = -1;
        if (s0 + tid < S) {
            slot = inverse[(int64_t)n * S + s0 + tid];
            if (slot < 0 || slot >= k) slot = -1;
        }
        s_slot[tid] = slot;
    }
    __syncthreads();
    if (grad_coord) {
        const int t = tid >> 2, c = tid & 3;                 // kTile * 4 == kThreads
        if (s0 + t < S) {
            const int slot = s_slot[t];
            float g = 0.f;
            if (slot >= 0) {
                const int64_t at = ((int64_t)n * k + slot) * 4 + c;
                if (g_refpoint) g = g_refpoint[at];
                if (g_ref_enc) {
                    const float r = ref_enc[at];
                    g += g_ref_enc[at] * (r * (1.f - r));
                }
            }
            grad_coord[((int64_t)n * S + s0 + t) * 4 + c] = g;
        }
    }
    if (!grad_memory) return;
    const int64_t base = ((int64_t)n * S + s0) * D;
    if (vec4) {
        const int q4 = D >> 2, total = (s1 - s0) * q4;
        float4 *dst = reinterpret_cast<float4 *>(grad_memory + base);
        for (int e = tid; e < total; e += kThreads) {
            const int t = e / q4, slot = s_slot[t];
            dst[e] = (slot >= 0 && g_tgt)
                         ? reinterpret_cast<const float4 *>(g_tgt + ((int64_t)n * k + slot) * D)[e - t * q4]
                         : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const int total = (s1 - s0) * D;
        for (int e = tid; e < total; e += kThreads) {
            const int t = e / D, slot = s_slot[t];
            grad_memory[base + e] = (slot >= 0 && g_tgt) ? g_tgt[((int64_t)n * k + slot) * D + (e - t * D)] : 0.f;
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int check_sizes(const char *what, int N, int S, int D)
{
    SEMIDETR_REQUIRE(N >= 1 && S >= 1 && D >= 1, SEMIDETR_E_BADARG, "%s: bad sizes (N %d, S %d, channels %d)", what, N, S, D);
    SEMIDETR_REQUIRE(N <= 65535 && (int64_t)N * S * D < ((int64_t)1 << 40) && (int64_t)N * S < ((int64_t)1 << 31) - kTile * 16 &&
                         D <= (1 << 16),
                     SEMIDETR_E_TOOLARGE, "%s: too large (N %d, S %d, channels %d)", what, N, S, D);
    return SEMIDETR_OK;
}

size_t topk_lds_bytes(int S, int kcap, bool in_lds)
{
    return (size_t)kcap * 8 + (size_t)kHistCopies * kHistStride * 4 + (in_lds ? (size_t)S * 4 : 0);
}

}  // namespace

extern "C" int semidetr_qsel_proposals_f32(void *stream, const float *memory, const unsigned char *padding_mask,
                                           const int64_t *spatial_shapes_host, const int64_t *spatial_shapes_dev,
                                           int num_levels, int N, int S, int D, float *output_memory,
                                           float *output_proposals, unsigned char *valid)
{
    SEMIDETR_REQUIRE(memory && padding_mask && output_memory && output_proposals && valid, SEMIDETR_E_BADARG,
                     "query_select proposals: null pointer argument");
    SEMIDETR_REQUIRE(!spatial_shapes_host != !spatial_shapes_dev, SEMIDETR_E_BADARG,
                     "query_select proposals: exactly one of spatial_shapes_host / spatial_shapes_dev");
    SEMIDETR_REQUIRE(num_levels >= 1 && num_levels <= SEMIDETR_QSEL_MAX_LEVELS, SEMIDETR_E_BADARG,
                     "query_select proposals: %d levels (1..%d)", num_levels, SEMIDETR_QSEL_MAX_LEVELS);
    if (int rc = check_sizes("query_select proposals", N, S, D)) return rc;
    SEMIDETR_REQUIRE(aligned16(output_proposals), SEMIDETR_E_BADARG, "query_select proposals: output_proposals must be 16-byte aligned");
    Levels lv;
    lv.num = num_levels;
    lv.dev = spatial_shapes_dev;
    for (int l = 0; l < SEMIDETR_QSEL_MAX_LEVELS; ++l) lv.h[l] = lv.w[l] = 0;
    if (spatial_shapes_host) {
        int64_t total = 0;
        for (int l = 0; l < num_levels; ++l) {
            const int64_t h = spatial_shapes_host[2 * l], w = spatial_shapes_host[2 * l + 1];
            SEMIDETR_REQUIRE(h >= 1 && w >= 1 && h <= S && w <= S, SEMIDETR_E_BADARG,
                             "query_select proposals: level %d is %lld x %lld", l, (long long)h, (long long)w);
            lv.h[l] = (int)h, lv.w[l] = (int)w;
            total += h * w;
        }
        SEMIDETR_REQUIRE(total == S, SEMIDETR_E_BADARG, "query_select proposals: the levels hold %lld tokens, memory has %d",
                         (long long)total, S);
    }
    const int vec4 = D % 4 == 0 && aligned16(memory) && aligned16(output_memory);
    hipLaunchKernelGGL(qsel_proposals_kernel, dim3((S + kTile - 1) / kTile, N), dim3(kThreads), 0, semidetr::as_stream(stream),
                       memory, padding_mask, lv, S, D, vec4, output_memory, output_proposals, valid);
    return semidetr::launch_status("qsel_proposals_kernel");
}

extern "C" int semidetr_qsel_proposals_backward_f32(void *stream, const float *grad_output_memory, const unsigned char *valid,
                                                    int N, int S, int D, float *grad_memory)
{
    SEMIDETR_REQUIRE(grad_output_memory && valid && grad_memory, SEMIDETR_E_BADARG,
                     "query_select proposals backward: null pointer argument");
    if (int rc = check_sizes("query_select proposals backward", N, S, D)) return rc;
    const int64_t rows = (int64_t)N * S;
    const int vec4 = D % 4 == 0 && aligned16(grad_output_memory) && aligned16(grad_memory);
    hipLaunchKernelGGL(qsel_mask_rows_kernel, dim3((unsigned)((rows + kTile - 1) / kTile)), dim3(kThreads), 0,
                       semidetr::as_stream(stream), grad_output_memory, valid, rows, D, vec4, grad_memory);
    return semidetr::launch_status("qsel_mask_rows_kernel");
}

extern "C" size_t semidetr_qsel_topk_workspace_bytes(int N, int S)
{
    return N >= 1 && S >= 1 ? (size_t)N * S * sizeof(unsigned) : 0;
}

extern "C" int semidetr_qsel_topk_f32(void *stream, const float *logits, int N, int S, int C, int k, void *workspace,
                                      size_t workspace_bytes, int64_t *indices, int32_t *inverse)
{
    SEMIDETR_REQUIRE(logits && workspace && indices && inverse, SEMIDETR_E_BADARG, "query_select topk: null pointer argument");
    if (int rc = check_sizes("query_select topk", N, S, C)) return rc;
    SEMIDETR_REQUIRE(k >= 1 && k <= S, SEMIDETR_E_BADARG, "query_select topk: k %d out of range (1..S = %d)", k, S);
    SEMIDETR_REQUIRE(k <= SEMIDETR_QSEL_MAX_K, SEMIDETR_E_TOOLARGE, "query_select topk: k %d (at most %d)", k, SEMIDETR_QSEL_MAX_K);
    SEMIDETR_REQUIRE(workspace_bytes >= semidetr_qsel_topk_workspace_bytes(N, S) && ((uintptr_t)workspace & 3) == 0,
                     SEMIDETR_E_BADARG, "query_select topk: workspace of %zu bytes (need %zu, 4-byte aligned)", workspace_bytes,
                     semidetr_qsel_topk_workspace_bytes(N, S));
    const int64_t rows = (int64_t)N * S;
    unsigned *keys = static_cast<unsigned *>(workspace);
    const int kcap = semidetr::next_pow2(k);
    const bool in_lds = topk_lds_bytes(S, kcap, true) <= kLdsBudget;
    const size_t lds = topk_lds_bytes(S, kcap, in_lds);
    if (lds > 64 * 1024)       // the fixed budget, not `lds`: one grant per device covers every later shape
        if (int rc = semidetr::allow_big_lds(&qsel_topk_kernel, kLdsBudget, "query_select topk")) return rc;
    const int vec4 = C % 4 == 0 && aligned16(logits);
    hipLaunchKernelGGL(qsel_rowmax_kernel, dim3((unsigned)((rows + kThreads / 16 - 1) / (kThreads / 16))), dim3(kThreads), 0,
                       semidetr::as_stream(stream), logits, rows, C, vec4, keys);
    if (int rc = semidetr::launch_status("qsel_rowmax_kernel")) return rc;
    hipLaunchKernelGGL(qsel_topk_kernel, dim3(N), dim3(kTopThreads), lds, semidetr::as_stream(stream), keys, S, k, kcap,
                       (int)in_lds, indices, inverse);
    return semidetr::launch_status("qsel_topk_kernel");
}

extern "C" int semidetr_qsel_gather_f32(void *stream, const int64_t *indices, const float *coord, const float *proposals,
                                        const float *memory, int N, int S, int k, int D, float *refpoint, float *init_box,
                                        float *tgt, float *ref_enc)
{
    SEMIDETR_REQUIRE(indices && coord && proposals && memory && refpoint && init_box && tgt && ref_enc, SEMIDETR_E_BADARG,
                     "query_select gather: null pointer argument");
    if (int rc = check_sizes("query_select gather", N, S, D)) return rc;
    SEMIDETR_REQUIRE(k >= 1, SEMIDETR_E_BADARG, "query_select gather: k %d", k);
    SEMIDETR_REQUIRE((int64_t)N * k < ((int64_t)1 << 24), SEMIDETR_E_TOOLARGE, "query_select gather: N * k = %lld slots (below 2^24)",
                     (long long)N * k);
    const int rows = N * k;
    const int vec4 = D % 4 == 0 && aligned16(memory) && aligned16(tgt);
    hipLaunchKernelGGL(qsel_gather_kernel, dim3((rows + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0,
                       semidetr::as_stream(stream), indices, coord, proposals, memory, rows, S, k, D, vec4, refpoint, init_box,
                       tgt, ref_enc);
    return semidetr::launch_status("qsel_gather_kernel");
}

extern "C" int semidetr_qsel_gather_backward_f32(void *stream, const int32_t *inverse, const float *grad_refpoint,
                                                 const float *grad_tgt, const float *grad_ref_enc, const float *ref_enc, int N,
                                                 int S, int k, int D, float *grad_coord, float *grad_memory)
{
    SEMIDETR_REQUIRE(inverse && (grad_coord || grad_memory), SEMIDETR_E_BADARG, "query_select gather backward: null pointer argument");
    SEMIDETR_REQUIRE(!grad_ref_enc || ref_enc, SEMIDETR_E_BADARG, "query_select gather backward: grad_ref_enc without ref_enc");
    if (int rc = check_sizes("query_select gather backward", N, S, D)) return rc;
    SEMIDETR_REQUIRE(k >= 1, SEMIDETR_E_BADARG, "query_select gather backward: k %d", k);
    SEMIDETR_REQUIRE((int64_t)N * k < ((int64_t)1 << 24), SEMIDETR_E_TOOLARGE,
                     "query_select gather backward: N * k = %lld slots (below 2^24)", (long long)N * k);
    const int vec4 = D % 4 == 0 && aligned16(grad_memory) && aligned16(grad_tgt);
    hipLaunchKernelGGL(qsel_gather_bwd_kernel, dim3((S + kTile - 1) / kTile, N), dim3(kThreads), 0, semidetr::as_stream(stream),
                       inverse, grad_refpoint, grad_tgt, grad_ref_enc, ref_enc, S, k, D, vec4, grad_coord, grad_memory);
    return semidetr::launch_status("qsel_gather_bwd_kernel");
}

// Decoding detections at evaluation / inference time (include/semidetr_hip.h, "Detection decode").
//
// Per image the reference runs, in Python, a sigmoid over (Q, C), a flat topk(max_per_img) over the Q * C scores, % and // for
// the label and the query, a box gather, cxcywh -> xyxy, four strided scale / clamp ops, a division by scale_factor and a cat
// (detr_od/models/dense_heads/dino_detr_ssod_head.py:1316-1330, 1396-1413, dino_detr_head.py:1129-1137, 1143-1152), then
// mmdet's bbox2result: a .cpu() round trip and one boolean-mask selection per class (mmdet/core/bbox/transforms.py:100-117).
// Here, for the whole batch in two launches:
//   det_chunk_select_kernel   grid (chunks, B): a workgroup takes kChunk logits into LDS as order-preserving integer keys, radix
//                             selects its min(k, chunk) largest (ties by the lower flat index) and writes them to the workspace
//                             as 64-bit (key, ~index) words; unused slots of its row are written as 0, so no memset is needed
//   det_merge_decode_kernel   grid B: radix select of the k largest words among the chunks' survivors (all words differ, so
//                             there is no tie left to break), bitonic sort, decode of the k rows, and the class grouping: a
//                             second sort by (label, rank) -- stable by construction -- and a binary search per class offset
// Selection is on the LOGITS: sigmoid is monotone, so the k largest logits are k largest scores, the decision contains no
// arithmetic, and it is one valid resolution of every tie the reference's topk leaves open (equal logits as well as distinct
// logits whose fp32 sigmoids coincide).  Order: logit descending, flat index q * C + c ascending; NaN above +inf; -0 == +0.
// Integer LDS atomics only; no float atomics, no scratch.
#include "common.h"
#include "select.h"

namespace {

using semidetr::kHistStride;
using semidetr::order_key;
using semidetr::sigmoidf_;

constexpr int kThreads = 1024;
constexpr int kChunk = 8192;                          // logits per workgroup of the first stage: 32 KB of keys
constexpr int kHistCopies = 16;
constexpr size_t kLdsBudget = 160 * 1024 - 2048;      // dynamic LDS of the merge kernel; the rest is its static part

typedef unsigned long long u64;

// ---- stage 1: the min(k, chunk) largest keys of one chunk.  grid (chunks, B)
__global__ __launch_bounds__(kThreads) void det_chunk_select_kernel(const float *__restrict__ logits, int QC, int k, int kk,
                                                                   u64 *__restrict__ survivors)
{
    __shared__ unsigned keys[kChunk];
    __shared__ int hist[kHistCopies * kHistStride];
    __shared__ int bins[256];
    __shared__ int s_wave[kThreads / 64];
    __shared__ int s_digit, s_remaining, s_fill, s_base;
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int first = chunk * kChunk;                                  // < QC: the grid has ceil(QC / kChunk) chunks
    const int len = QC - first < kChunk ? QC - first : kChunk;
    const int want = k < len ? k : len;                                // <= kk
    const float *src = logits + (int64_t)b * QC + first;
    u64 *dst = survivors + ((int64_t)b * gridDim.x + chunk) * kk;
    for (int i = tid; i < len; i += kThreads) keys[i] = order_key(src[i]);
    if (tid == 0) { s_fill = 0; s_remaining = want; s_base = 0; }
    __syncthreads();
    unsigned prefix = 0, pmask = 0;
    for (int pass = 3; pass >= 0; --pass) {
        semidetr::histogram_pass<kThreads, kHistCopies>(hist, keys, len, prefix, pmask, pass);
        // 1 <= s_remaining <= words counted: it starts as want = min(k, len) with k >= 1 (launcher) and len >= 1 (grid), against
        // all len keys, and every pass leaves the rank inside the chosen digit, whose keys are the next pass's
        semidetr::pick_digit<kThreads, kHistCopies>(hist, bins, &s_digit, &s_remaining);
        prefix |= (unsigned)s_digit << (8 * pass);
        pmask |= 0xFFu << (8 * pass);
    }
    const int ties = s_remaining;
    // every key above the want-th, and the first `ties` positions, in index order, that equal it
    semidetr::collect_with_ties<kThreads>(keys, len, prefix, ties, s_wave, &s_base, [&](int i, unsigned u) {
        const int slot = atomicAdd(&s_fill, 1);
        if (slot < kk) dst[slot] = ((u64)u << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)(first + i));
    });
    for (int i = want + tid; i < kk; i += kThreads) dst[i] = 0;         // below every real word: the smallest key is ~(-inf) > 0
}

struct Row { float x1, y1, x2, y2, score; };

// one detection from its flat index, in the reference's operation order, every operation a single fp32 rounding
__device__ inline Row decode_row(const float *__restrict__ logits, const float *__restrict__ boxes, unsigned idx, int C, float H,
                                 float W, const float *__restrict__ sf)
{
    const unsigned q = idx / (unsigned)C;
    const float cx = boxes[4 * (int64_t)q], cy = boxes[4 * (int64_t)q + 1], w = boxes[4 * (int64_t)q + 2], h = boxes[4 * (int64_t)q + 3];
    const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
    float v[4] = {__fmul_rn(__fsub_rn(cx, hw), W), __fmul_rn(__fsub_rn(cy, hh), H), __fmul_rn(__fadd_rn(cx, hw), W),
                  __fmul_rn(__fadd_rn(cy, hh), H)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float top = (j & 1) ? H : W;
        v[j] = v[j] < 0.f ? 0.f : (v[j] > top ? top : v[j]);           // NaN stays NaN, as clamp_ leaves it
        if (sf) v[j] = __fdiv_rn(v[j], sf[j]);
    }
    Row r = {v[0], v[1], v[2], v[3], sigmoidf_(logits[idx])};
    return r;
}

__device__ inline void store_row(float *dst, const Row &r)
{
    dst[0] = r.x1, dst[1] = r.y1, dst[2] = r.x2, dst[3] = r.y2, dst[4] = r.score;
}

// ---- stage 2: per image, the k largest of the M survivors, sorted; decode; class grouping.  grid B.
// dynamic LDS: sel[kcap], hist, then the M words when they fit (in_lds).
__global__ __launch_bounds__(kThreads) void det_merge_decode_kernel(const u64 *__restrict__ survivors, int M, int in_lds,
                                                                   const float *__restrict__ logits,
                                                                   const float *__restrict__ bbox_pred,
                                                                   const float *__restrict__ img_hw,
                                                                   const float *__restrict__ scale_factor, int Q, int C, int k,
                                                                   int kcap, float *__restrict__ out_dets,
                                                                   int64_t *__restrict__ out_labels,
                                                                   float *__restrict__ out_by_class,
                                                                   int32_t *__restrict__ out_offsets)
{
    extern __shared__ __attribute__((aligned(16))) u64 det_smem[];
    __shared__ int bins[256];
    __shared__ int s_digit, s_remaining, s_fill;
    u64 *sel = det_smem;
    int *hist = reinterpret_cast<int *>(sel + kcap);                                      // 16 448 bytes: keeps 8-byte alignment
    unsigned *flat = reinterpret_cast<unsigned *>(hist + kHistCopies * kHistStride);       // flat index of every rank
    u64 *cand_l = reinterpret_cast<u64 *>(flat + kcap);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int QC = Q * C;
    const u64 *cg = survivors + (int64_t)b * M;
    if (in_lds)
        for (int i = tid; i < M; i += kThreads) cand_l[i] = cg[i];
    for (int i = tid; i < kcap; i += kThreads) sel[i] = 0;
    if (tid == 0) { s_fill = 0; s_remaining = k; }
    __syncthreads();
    const u64 *cand = in_lds ? cand_l : cg;
    // radix select over the 64-bit words, most significant byte first.  The real words are pairwise different (the index is
    // part of them) and there are at least k of them, so after eight passes `prefix` IS the k-th largest word.
    u64 prefix = 0, pmask = 0;
    for (int pass = 7; pass >= 0; --pass) {
        semidetr::histogram_pass<kThreads, kHistCopies>(hist, cand, M, prefix, pmask, pass);
        // 1 <= s_remaining <= words counted: it starts as k >= 1 against all M = chunks * kk words (zero tails included), and
        // k <= M because kk = k, or kk = kChunk and chunks * kChunk >= Q * C >= k (launcher); every pass leaves the rank inside
        // the chosen digit, whose words are the next pass's
        semidetr::pick_digit<kThreads, kHistCopies>(hist, bins, &s_digit, &s_remaining);
        prefix |= (u64)s_digit << (8 * pass);
        pmask |= (u64)0xFF << (8 * pass);
    }
    for (int i = tid; i < M; i += kThreads) {
        const u64 u = cand[i];
        if (u >= prefix && u != 0) {
            const int slot = atomicAdd(&s_fill, 1);
            if (slot < kcap) sel[slot] = u;
        }
    }
    semidetr::bitonic_desc<kThreads>(sel, kcap);
    const float H = img_hw[2 * b], W = img_hw[2 * b + 1];
    const float *sf = scale_factor ? scale_factor + 4 * b : nullptr;
    const float *lg = logits + (int64_t)b * QC, *bx = bbox_pred + (int64_t)b * Q * 4;
    // rank r -> flat index; a slot that was never filled (impossible for valid arguments) decodes index 0 instead of reading
    // out of bounds
    for (int r = tid; r < k; r += kThreads) {
        unsigned idx = 0xFFFFFFFFu - (unsigned)(sel[r] & 0xFFFFFFFFull);
        if (idx >= (unsigned)QC) idx = 0;
        flat[r] = idx;
        store_row(out_dets + ((int64_t)b * k + r) * 5, decode_row(lg, bx, idx, C, H, W, sf));
        out_labels[(int64_t)b * k + r] = (int64_t)(idx % (unsigned)C);
    }
    if (!out_by_class) return;
    __syncthreads();
    // bbox2result: the same rows ordered by (label ascending, rank ascending) -- stable because the rank is part of the word.
    // The sort is descending, so the words are complemented; the unused slots are 0 and sink to the end.
    for (int r = tid; r < kcap; r += kThreads) sel[r] = r < k ? ~(((u64)(flat[r] % (unsigned)C) << 32) | (unsigned)r) : 0;
    semidetr::bitonic_desc<kThreads>(sel, kcap);
    for (int j = tid; j < k; j += kThreads) {
        const int r = (int)((~sel[j]) & 0xFFFFFFFFull);
        store_row(out_by_class + ((int64_t)b * k + j) * 5, decode_row(lg, bx, flat[r < k ? r : 0], C, H, W, sf));
    }
    // offsets[c] = number of rows whose label is below c: the first position of the sorted words whose label is >= c
    for (int c = tid; c <= C; c += kThreads) {
        int lo = 0, hi = k;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)((~sel[mid]) >> 32) < (unsigned)c) lo = mid + 1; else hi = mid;
        }
        out_offsets[(int64_t)b * (C + 1) + c] = lo;
    }
}

inline int num_chunks(int64_t QC) { return (int)((QC + kChunk - 1) / kChunk); }

size_t merge_lds_bytes(int M, int kcap, bool in_lds)
{
    return (size_t)kcap * 12 + (size_t)kHistCopies * kHistStride * 4 + (in_lds ? (size_t)M * 8 : 0);
}

// the checks both entry points share; 0 when (batch, num_query, num_classes, k) is a problem the kernels take
int check_problem(int B, int Q, int C, int k, bool report)
{
    const int64_t QC = (int64_t)Q * C;
    if (!(B >= 1 && Q >= 1 && C >= 1 && k >= 1 && (int64_t)k <= QC))
        return report ? semidetr::fail(SEMIDETR_E_BADARG, "det_decode: bad sizes (batch %d, num_query %d, num_classes %d, k %d; "
                                       "1 <= k <= num_query * num_classes)", B, Q, C, k) : SEMIDETR_E_BADARG;
    if (!(k <= SEMIDETR_DET_MAX_K && QC < ((int64_t)1 << 31) && B <= 65535 && (int64_t)B * QC < ((int64_t)1 << 40)))
        return report ? semidetr::fail(SEMIDETR_E_TOOLARGE, "det_decode: too large (batch %d, num_query %d, num_classes %d, k %d; "
                                       "k <= %d, num_query * num_classes < 2^31, batch <= 65535)", B, Q, C, k, SEMIDETR_DET_MAX_K)
                      : SEMIDETR_E_TOOLARGE;
    return SEMIDETR_OK;
}

}  // namespace

extern "C" size_t semidetr_det_workspace_bytes(int batch, int num_query, int num_classes, int k)
{
    if (check_problem(batch, num_query, num_classes, k, false)) return 0;
    const int kk = k < kChunk ? k : kChunk;
    return (size_t)batch * num_chunks((int64_t)num_query * num_classes) * kk * sizeof(u64);
}

extern "C" int semidetr_det_decode_f32(void *stream, const float *cls_logits, const float *bbox_pred, const float *img_hw,
                                       const float *scale_factor, int batch, int num_query, int num_classes, int k,
                                       void *workspace, size_t workspace_bytes, float *out_dets, int64_t *out_labels,
                                       float *out_dets_by_class, int32_t *out_class_offsets)
{
    SEMIDETR_REQUIRE(cls_logits && bbox_pred && img_hw && workspace && out_dets && out_labels, SEMIDETR_E_BADARG,
                     "det_decode: null pointer argument");
    SEMIDETR_REQUIRE(!out_dets_by_class == !out_class_offsets, SEMIDETR_E_BADARG,
                     "det_decode: out_dets_by_class and out_class_offsets are given together or not at all");
    if (int rc = check_problem(batch, num_query, num_classes, k, true)) return rc;
    const size_t need = semidetr_det_workspace_bytes(batch, num_query, num_classes, k);
    SEMIDETR_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0, SEMIDETR_E_BADARG,
                     "det_decode: workspace of %zu bytes (need %zu, 8-byte aligned)", workspace_bytes, need);
    const int QC = num_query * num_classes;
    const int chunks = num_chunks(QC), kk = k < kChunk ? k : kChunk, kcap = semidetr::next_pow2(k);
    const int M = chunks * kk;
    const bool in_lds = merge_lds_bytes(M, kcap, true) <= kLdsBudget;
    const size_t lds = merge_lds_bytes(M, kcap, in_lds);
    if (lds > 64 * 1024)       // the fixed budget, not `lds`: one grant per device covers every later shape
        if (int rc = semidetr::allow_big_lds(&det_merge_decode_kernel, kLdsBudget, "det_decode")) return rc;
    u64 *survivors = static_cast<u64 *>(workspace);
    hipLaunchKernelGGL(det_chunk_select_kernel, dim3(chunks, batch), dim3(kThreads), 0, semidetr::as_stream(stream), cls_logits,
                       QC, k, kk, survivors);
    if (int rc = semidetr::launch_status("det_chunk_select_kernel")) return rc;
    hipLaunchKernelGGL(det_merge_decode_kernel, dim3(batch), dim3(kThreads), lds, semidetr::as_stream(stream), survivors, M,
                       (int)in_lds, cls_logits, bbox_pred, img_hw, scale_factor, num_query, num_classes, k, kcap, out_dets,
                       out_labels, out_dets_by_class, out_class_offsets);
    return semidetr::launch_status("det_merge_decode_kernel");
}

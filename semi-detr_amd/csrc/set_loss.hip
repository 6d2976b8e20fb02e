// Set-prediction losses of the DINO-DETR SSOD head for gfx950 (DINODETRSSODHead.loss / loss_single / loss_single_dn,
// detr_od/models/dense_heads/dino_detr_ssod_head.py:508-883): sigmoid focal (or task-aligned focal) classification, L1 on
// cxcywh (all four coordinates, xy, hw) and GIoU on image-scale xyxy, for every decoder layer, the encoder proposals and the
// dn queries of one loss() call.
//
//   setloss_fwd_kernel       one workgroup per (segment, layer, 64-row chunk): the rows' targets (read from the stacked
//                            matched targets, or built from the ground truths for dn rows), the focal sum over the chunk's
//                            logits, the box terms and the normaliser counts of the chunk -> kStats fp64 partial sums
//   setloss_reduce_kernel    ONE workgroup: per (segment, layer) the chunks' partials in a fixed order -> stats, the
//                            normaliser inputs and (one rank) the finalized losses and backward scales
//   setloss_finalize_kernel  ONE workgroup, several ranks only: the same finalize after the caller's all-reduce of the
//                            normaliser inputs
//   setloss_bwd_kernel       same decomposition as the forward: d loss / d logits and d loss / d boxes, recomputed from the
//                            inputs and scaled by upstream grad x loss_weight / normaliser (dense gradient tensors)
// No float atomics: every sum is taken in a fixed order, so a launch sequence is bitwise reproducible.
//
// Arithmetic (tests/set_loss_ref64.py restates it in numpy float64):
//   focal  (mmdet py_sigmoid_focal_loss, focal_loss.py:12-57) with z = t ? -x : x, a = t ? alpha : 1 - alpha:
//          loss = a * sigmoid(z)^gamma * softplus(z), softplus through log1p(exp(-|z|)) (no log(0) at any |x|),
//          d/dz = a * sigmoid(z)^gamma * (gamma * sigmoid(-z) * softplus(z) + sigmoid(z)); x row weight (label_weights)
//   TAL    (task_aligned_focal_loss.py:35-66, warm-up) as csrc/tal_loss.hip, sigmoid fused, no row weight
//   L1     sum_k w_k |b_k - t_k| over k = 0..3, k < 2, k >= 2;  d/db_k = w_k sign(b_k - t_k)
//   GIoU   1 - giou(xyxy(b) * f, xyxy(t) * f) (bbox_overlaps mode='giou', is_aligned, eps), weight mean_k(w_k); torch's
//          max / min tie rule in the backward (half to each side); zero when no bbox weight is > 0 (GIoULoss:372-376)
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kRows = 64;
constexpr int kStats = SEMIDETR_SET_LOSS_NUM_STATS, kTerms = SEMIDETR_SET_LOSS_NUM_TERMS;
constexpr int kMaxSegs = SEMIDETR_SET_LOSS_MAX_SEGMENTS, kMaxT = SEMIDETR_SET_LOSS_MAX_LAYERS;

struct Launch {
    semidetr_set_loss_segment seg[kMaxSegs];
    int nseg, vec4_mask;             // bit i: segment i's logits take the float4 path
    int block_begin[kMaxSegs + 1];     // first workgroup of each segment
    int t_begin[kMaxSegs + 1];         // first (segment, layer) index of each segment
    int chunks[kMaxSegs];              // 64-row chunks per layer
};

struct Row {
    int label;        // class index, num_classes = background
    float lw;         // row weight of the classification term (warm-up: the alignment metric)
    float tg[4], w[4];
    bool pos;
};

__device__ __forceinline__ void load_row(const semidetr_set_loss_segment &s, int layer, int b, int q, Row &r)
{
    const int64_t pr = ((int64_t)layer * s.num_images + b) * s.num_query + q;     // stacked target row
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
    if (s.kind == SEMIDETR_SET_LOSS_DN) {
        const int g0 = s.gt_offsets[b], G = s.gt_offsets[b + 1] - g0;
        const int j = q % s.single_pad;
        r.pos = j < G;
        r.label = r.pos ? (int)s.gt_labels[g0 + j] : s.num_classes;
        r.lw = G > 0 ? 1.f : 0.f;
        if (r.pos) {     // _get_target_single_dn: bbox_xyxy_to_cxcywh(gt / factor)
            const float fw = s.img_wh[2 * b], fh = s.img_wh[2 * b + 1];
            const float *g = s.gt_boxes + 4 * (int64_t)(g0 + j);
            const float x1 = g[0] / fw, y1 = g[1] / fh, x2 = g[2] / fw, y2 = g[3] / fh;
            t0 = (x1 + x2) / 2.f; t1 = (y1 + y2) / 2.f; t2 = x2 - x1; t3 = y2 - y1;
            w0 = w1 = w2 = w3 = 1.f;
        }
    } else {
        r.label = (int)s.labels[pr];
        r.pos = r.label >= 0 && r.label < s.num_classes;
        if (s.kind == SEMIDETR_SET_LOSS_WARMUP) r.lw = s.metrics[pr];
        else r.lw = s.label_weights ? s.label_weights[pr] : 1.f;
        if (s.bbox_targets) {
            const float *tp = s.bbox_targets + 4 * pr, *wp = s.bbox_weights + 4 * pr;
            t0 = tp[0]; t1 = tp[1]; t2 = tp[2]; t3 = tp[3];
            // warm-up: the box terms cover the positive rows only (dino_detr_ssod_head.py:719-745)
            if (s.kind != SEMIDETR_SET_LOSS_WARMUP || r.pos) { w0 = wp[0]; w1 = wp[1]; w2 = wp[2]; w3 = wp[3]; }
        }
    }
    r.tg[0] = t0; r.tg[1] = t1; r.tg[2] = t2; r.tg[3] = t3;
    r.w[0] = w0; r.w[1] = w1; r.w[2] = w2; r.w[3] = w3;
}

// loss of one logit; *dx = d loss / d x when dx != nullptr
__device__ __forceinline__ float focal_elem(float x, bool t, float alpha, float gamma, float *dx)
{
    const float z = t ? -x : x;
    const float a = t ? alpha : 1.f - alpha;
    const float ez = expf(-fabsf(z));
    const float s = z >= 0.f ? 1.f / (1.f + ez) : ez / (1.f + ez);          // sigmoid(z)
    const float oms = z >= 0.f ? ez / (1.f + ez) : 1.f / (1.f + ez);        // sigmoid(-z)
    const float sp = fmaxf(z, 0.f) + log1pf(ez);                            // softplus(z)
    const float sg = gamma == 2.f ? s * s : powf(s, gamma);
    if (dx) {
        const float dz = a * sg * (gamma * oms * sp + s);
        *dx = t ? -dz : dz;
    }
    return a * sg * sp;
}

__device__ __forceinline__ float tal_elem(float x, float st, float gamma, float *dx)
{
    const float p = 1.0f / (1.0f + expf(-x));
    const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(logf(1.0f - p), -100.f);
    const float ce = -(st * lp + (1.0f - st) * l1p);
    const float d = st - p, ad = fabsf(d);
    const float mod = gamma == 2.0f ? ad * ad : powf(ad, gamma);
    if (dx) {
        const float dmod = gamma == 2.0f ? -2.0f * d : (ad > 0.f ? -gamma * powf(ad, gamma - 1.0f) * (d > 0.f ? 1.f : -1.f) : 0.f);
        const float dce = (p - st) / fmaxf((1.0f - p) * p, 1e-12f);
        *dx = (dmod * ce + mod * dce) * (p * (1.0f - p));
    }
    return mod * ce;
}

__device__ __forceinline__ float cls_elem(const semidetr_set_loss_segment &s, float x, int c, const Row &r, float *dx)
{
    if (s.kind == SEMIDETR_SET_LOSS_WARMUP) return tal_elem(x, c == r.label ? r.lw : 0.f, s.gamma, dx);
    const float v = focal_elem(x, c == r.label, s.alpha, s.gamma, dx);
    if (dx) *dx *= r.lw;
    return v * r.lw;
}

// d max(a, b) / d a under torch's rule (ties: half to each side)
__device__ __forceinline__ float dmax_a(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
__device__ __forceinline__ float dmin_a(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

// 1 - giou of pred (cxcywh b) and target (cxcywh tg), both scaled by (fw, fh); grad (when non-null) += c * d/d b
__device__ __forceinline__ float giou_loss(const float b[4], const float tg[4], float fw, float fh, float eps, float c,
                                           float *grad)
{
    const float f[4] = {fw, fh, fw, fh};
    float p[4], g[4];
    p[0] = (b[0] - 0.5f * b[2]) * f[0]; p[1] = (b[1] - 0.5f * b[3]) * f[1];
    p[2] = (b[0] + 0.5f * b[2]) * f[2]; p[3] = (b[1] + 0.5f * b[3]) * f[3];
    g[0] = (tg[0] - 0.5f * tg[2]) * f[0]; g[1] = (tg[1] - 0.5f * tg[3]) * f[1];
    g[2] = (tg[0] + 0.5f * tg[2]) * f[2]; g[3] = (tg[1] + 0.5f * tg[3]) * f[3];
    const float a1 = (p[2] - p[0]) * (p[3] - p[1]), a2 = (g[2] - g[0]) * (g[3] - g[1]);
    float lt[2], rb[2], wh[2], elt[2], erb[2], ewh[2];
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
        lt[k] = fmaxf(p[k], g[k]); rb[k] = fminf(p[k + 2], g[k + 2]);
        wh[k] = fmaxf(rb[k] - lt[k], 0.f);
        elt[k] = fminf(p[k], g[k]); erb[k] = fmaxf(p[k + 2], g[k + 2]);
        ewh[k] = fmaxf(erb[k] - elt[k], 0.f);
    }
    const float ov = wh[0] * wh[1];
    const float uraw = a1 + a2 - ov, u = fmaxf(uraw, eps);
    const float eraw = ewh[0] * ewh[1], e = fmaxf(eraw, eps);
    const float giou = ov / u - (e - u) / e;
    if (grad) {
        // L = 1 - O/U + (E - U)/E
        const float dU = (ov / (u * u) - 1.f / e) * dmax_a(uraw, eps);
        const float dE = (u / (e * e)) * dmax_a(eraw, eps);
        const float dO = -1.f / u - dU;                 // union = a1 + a2 - O
        float dp[4] = {0.f, 0.f, 0.f, 0.f};
        // area1 = (p2 - p0)(p3 - p1)
        dp[2] += dU * (p[3] - p[1]); dp[0] -= dU * (p[3] - p[1]);
        dp[3] += dU * (p[2] - p[0]); dp[1] -= dU * (p[2] - p[0]);
        #pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float dwh = dO * wh[1 - k] * (rb[k] - lt[k] >= 0.f ? 1.f : 0.f);
            dp[k + 2] += dwh * dmin_a(p[k + 2], g[k + 2]);
            dp[k] -= dwh * dmax_a(p[k], g[k]);
            const float dewh = dE * ewh[1 - k] * (erb[k] - elt[k] >= 0.f ? 1.f : 0.f);
            dp[k + 2] += dewh * dmax_a(p[k + 2], g[k + 2]);
            dp[k] -= dewh * dmin_a(p[k], g[k]);
        }
        #pragma unroll
        for (int k = 0; k < 4; ++k) dp[k] *= f[k] * c;
        grad[0] += dp[0] + dp[2]; grad[1] += dp[1] + dp[3];
        grad[2] += 0.5f * (dp[2] - dp[0]); grad[3] += 0.5f * (dp[3] - dp[1]);
    }
    return 1.f - giou;
}

// block -> (segment, layer, chunk)
__device__ __forceinline__ void locate(const Launch &L, int blk, int &si, int &layer, int &chunk, int &t)
{
    si = 0;
    while (si + 1 < L.nseg && blk >= L.block_begin[si + 1]) ++si;
    const int local = blk - L.block_begin[si];
    layer = local / L.chunks[si];
    chunk = local - layer * L.chunks[si];
    t = L.t_begin[si] + layer;
}

template <int NV>
__device__ __forceinline__ void wave_sum(double (&v)[NV])
{
    for (int k = 0; k < NV; ++k)
        for (int sft = 32; sft > 0; sft >>= 1) v[k] += __shfl_xor(v[k], sft, 64);
}

__global__ __launch_bounds__(kThreads) void setloss_fwd_kernel(const Launch L, double *__restrict__ partial)
{
    __shared__ Row rows[kRows];
    __shared__ double red[kWaves][kStats];
    int si, layer, chunk, t;
    locate(L, blockIdx.x, si, layer, chunk, t);
    const semidetr_set_loss_segment &s = L.seg[si];
    const int nrows = s.num_images * s.num_query;
    const int r0 = chunk * kRows, nr = min(kRows, nrows - r0);
    double acc[kStats];
    for (int k = 0; k < kStats; ++k) acc[k] = 0.0;
    if (threadIdx.x < nr) {
        const int r = r0 + threadIdx.x, b = r / s.num_query, q = r - b * s.num_query;
        Row rw;
        load_row(s, layer, b, q, rw);
        rows[threadIdx.x] = rw;
        acc[5] = rw.pos ? 1.0 : 0.0;
        const float wsum = (rw.w[0] + rw.w[1]) + (rw.w[2] + rw.w[3]);
        acc[6] = wsum > 0.f ? 1.0 : 0.0;
        acc[7] = (rw.w[0] > 0.f || rw.w[1] > 0.f || rw.w[2] > 0.f || rw.w[3] > 0.f) ? 1.0 : 0.0;
        acc[8] = rw.pos ? (double)rw.w[0] : 0.0;
        acc[9] = s.kind == SEMIDETR_SET_LOSS_WARMUP ? (double)rw.lw : 0.0;
        if (s.boxes) {
            const float *bp = s.boxes + layer * s.box_stride[0] + b * s.box_stride[1] + q * s.box_stride[2];
            const float bb[4] = {bp[0], bp[1], bp[2], bp[3]};
            float l1[4];
            #pragma unroll
            for (int k = 0; k < 4; ++k) l1[k] = fabsf(bb[k] - rw.tg[k]) * rw.w[k];
            acc[1] = (double)l1[0] + l1[1] + l1[2] + l1[3];
            acc[2] = (double)l1[0] + l1[1];
            acc[3] = (double)l1[2] + l1[3];
            const float wm = wsum / 4.f;
            if (wm != 0.f)
                acc[4] = (double)(giou_loss(bb, rw.tg, s.img_wh[2 * b], s.img_wh[2 * b + 1], s.iou_eps, 0.f, nullptr) * wm);
        }
    }
    __syncthreads();
    const int C = s.num_classes;
    double cls = 0.0;
    if ((L.vec4_mask >> si) & 1) {
        const int C4 = C / 4, n = nr * C4;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int rr = i / C4, c0 = (i - rr * C4) * 4;
            const int r = r0 + rr, b = r / s.num_query, q = r - b * s.num_query;
            const float4 x = *reinterpret_cast<const float4 *>(s.logits + layer * s.logit_stride[0] +
                                                               b * s.logit_stride[1] + q * s.logit_stride[2] + c0);
            const Row &rw = rows[rr];
            cls += (double)((cls_elem(s, x.x, c0, rw, nullptr) + cls_elem(s, x.y, c0 + 1, rw, nullptr)) +
                            (cls_elem(s, x.z, c0 + 2, rw, nullptr) + cls_elem(s, x.w, c0 + 3, rw, nullptr)));
        }
    } else {
        const int n = nr * C;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int rr = i / C, c = i - rr * C;
            const int r = r0 + rr, b = r / s.num_query, q = r - b * s.num_query;
            const float x = s.logits[layer * s.logit_stride[0] + b * s.logit_stride[1] + q * s.logit_stride[2] + c];
            cls += (double)cls_elem(s, x, c, rows[rr], nullptr);
        }
    }
    acc[0] = cls;
    wave_sum(acc);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < kStats; ++k) red[wv][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < kStats)
        partial[(int64_t)blockIdx.x * kStats + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// normaliser inputs of one (segment, layer): [0] classification, [1] regression (before any cross-rank mean / clamp)
__device__ __forceinline__ void norm_inputs(const semidetr_set_loss_segment &s, const double *st, float *nin)
{
    const double rows = (double)s.num_images * s.num_query;
    if (s.kind == SEMIDETR_SET_LOSS_WARMUP) {
        nin[0] = (float)st[9];                   // sum of the normalised alignment metrics (head.py:688-689)
        nin[1] = (float)st[8];                   // sum of the positive rows' bbox_weights[:, 0] (head.py:726-727)
    } else if (s.kind == SEMIDETR_SET_LOSS_DN) {
        nin[0] = (float)(st[5] + st[5] * (double)s.bg_cls_weight);    // num_total_neg = num_total_pos (get_targets_dn)
        nin[1] = (float)st[5];
    } else {
        nin[0] = (float)(st[5] + (rows - st[5]) * (double)s.bg_cls_weight);
        nin[1] = (float)st[6];                   // rows with bbox_weights.sum(-1) > 0 (head.py:766)
    }
}

__device__ __forceinline__ void finalize_one(const semidetr_set_loss_segment &s, const double *st, const float *nloc,
                                             const float *nred, float *losses, float *scales)
{
    const bool red_cls = nred && (s.kind == SEMIDETR_SET_LOSS_WARMUP || s.sync_cls);
    const float ncls = fmaxf(red_cls ? nred[0] : nloc[0], 1.f);
    const float nreg = fmaxf(nred ? nred[1] : nloc[1], 1.f);
    float sc[kTerms];
    sc[0] = s.cls_weight / ncls;
    sc[1] = sc[3] = sc[4] = s.l1_weight / nreg;
    sc[2] = st[7] > 0.0 ? s.iou_weight / nreg : 0.f;        // GIoULoss: no weight > 0 -> 0 (and no gradient)
    const double sums[kTerms] = {st[0], st[1], st[4], st[2], st[3]};
    #pragma unroll
    for (int k = 0; k < kTerms; ++k) {
        scales[k] = sc[k];
        losses[k] = sc[k] == 0.f ? 0.f : (float)(sums[k] * (double)sc[k]);
    }
}

__device__ __forceinline__ const semidetr_set_loss_segment &seg_of_t(const Launch &L, int t)
{
    int si = 0;
    while (si + 1 < L.nseg && t >= L.t_begin[si + 1]) ++si;
    return L.seg[si];
}

__global__ __launch_bounds__(kThreads) void setloss_reduce_kernel(const Launch L, const double *__restrict__ partial,
                                                                  double *__restrict__ stats, float *__restrict__ norms,
                                                                  float *__restrict__ losses, float *__restrict__ scales)
{
    __shared__ double st[kMaxT][kStats];
    const int T = L.t_begin[L.nseg], wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = wv; t < T; t += kWaves) {       // wave wv owns (segment, layer) t: lanes stride its chunks, then a shuffle tree
        int si = 0;
        while (si + 1 < L.nseg && t >= L.t_begin[si + 1]) ++si;
        const int b0 = L.block_begin[si] + (t - L.t_begin[si]) * L.chunks[si], nb = L.chunks[si];
        double acc[kStats];
        for (int k = 0; k < kStats; ++k) acc[k] = 0.0;
        for (int i = lane; i < nb; i += 64)
            for (int k = 0; k < kStats; ++k) acc[k] += partial[(int64_t)(b0 + i) * kStats + k];
        wave_sum(acc);
        if (lane == 0)
            for (int k = 0; k < kStats; ++k) st[t][k] = acc[k];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T * kStats; i += kThreads) stats[i] = st[i / kStats][i % kStats];
    if (threadIdx.x < T) {
        const int t = threadIdx.x;
        const semidetr_set_loss_segment &s = seg_of_t(L, t);
        float nin[2];
        norm_inputs(s, st[t], nin);
        norms[2 * t] = nin[0];
        norms[2 * t + 1] = nin[1];
        if (losses) finalize_one(s, st[t], nin, nullptr, losses + kTerms * t, scales + kTerms * t);
    }
}

__global__ __launch_bounds__(64) void setloss_finalize_kernel(const Launch L, const double *__restrict__ stats,
                                                              const float *__restrict__ norms_local,
                                                              const float *__restrict__ norms_reduced,
                                                              float *__restrict__ losses, float *__restrict__ scales)
{
    const int T = L.t_begin[L.nseg];
    for (int t = threadIdx.x; t < T; t += 64)
        finalize_one(seg_of_t(L, t), stats + kStats * t, norms_local + 2 * t, norms_reduced + 2 * t, losses + kTerms * t,
                     scales + kTerms * t);
}

__global__ __launch_bounds__(kThreads) void setloss_bwd_kernel(const Launch L, const float *__restrict__ scales,
                                                               const float *__restrict__ grad_out)
{
    __shared__ Row rows[kRows];
    int si, layer, chunk, t;
    locate(L, blockIdx.x, si, layer, chunk, t);
    const semidetr_set_loss_segment &s = L.seg[si];
    const int nrows = s.num_images * s.num_query;
    const int r0 = chunk * kRows, nr = min(kRows, nrows - r0);
    float co[kTerms];
    #pragma unroll
    for (int k = 0; k < kTerms; ++k) co[k] = (scales ? scales[kTerms * t + k] : 1.f) * grad_out[kTerms * t + k];
    const int64_t lrow = (int64_t)layer * nrows;         // first dense gradient row of this layer
    if (threadIdx.x < nr) {
        const int r = r0 + threadIdx.x, b = r / s.num_query, q = r - b * s.num_query;
        Row rw;
        load_row(s, layer, b, q, rw);
        rows[threadIdx.x] = rw;
        if (s.boxes && s.grad_boxes) {
            const float *bp = s.boxes + layer * s.box_stride[0] + b * s.box_stride[1] + q * s.box_stride[2];
            const float bb[4] = {bp[0], bp[1], bp[2], bp[3]};
            float g[4];
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = bb[k] - rw.tg[k];
                const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                g[k] = rw.w[k] * sg * (co[1] + (k < 2 ? co[3] : co[4]));
            }
            const float wm = ((rw.w[0] + rw.w[1]) + (rw.w[2] + rw.w[3])) / 4.f;
            if (wm != 0.f && co[2] != 0.f)
                giou_loss(bb, rw.tg, s.img_wh[2 * b], s.img_wh[2 * b + 1], s.iou_eps, wm * co[2], g);
            *reinterpret_cast<float4 *>(s.grad_boxes + 4 * (lrow + r)) = make_float4(g[0], g[1], g[2], g[3]);
        }
    }
    __syncthreads();
    if (!s.grad_logits) return;
    const int C = s.num_classes;
    const float c0f = co[0];
    float *gl = s.grad_logits + lrow * C;
    if ((L.vec4_mask >> si) & 1) {
        const int C4 = C / 4, n = nr * C4;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int rr = i / C4, c0 = (i - rr * C4) * 4;
            const int r = r0 + rr, b = r / s.num_query, q = r - b * s.num_query;
            const float4 x = *reinterpret_cast<const float4 *>(s.logits + layer * s.logit_stride[0] +
                                                               b * s.logit_stride[1] + q * s.logit_stride[2] + c0);
            const Row &rw = rows[rr];
            float4 g;
            cls_elem(s, x.x, c0, rw, &g.x);
            cls_elem(s, x.y, c0 + 1, rw, &g.y);
            cls_elem(s, x.z, c0 + 2, rw, &g.z);
            cls_elem(s, x.w, c0 + 3, rw, &g.w);
            g.x *= c0f; g.y *= c0f; g.z *= c0f; g.w *= c0f;
            *reinterpret_cast<float4 *>(gl + (int64_t)r * C + c0) = g;
        }
    } else {
        const int n = nr * C;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int rr = i / C, c = i - rr * C;
            const int r = r0 + rr, b = r / s.num_query, q = r - b * s.num_query;
            const float x = s.logits[layer * s.logit_stride[0] + b * s.logit_stride[1] + q * s.logit_stride[2] + c];
            float g;
            cls_elem(s, x, c, rows[rr], &g);
            gl[(int64_t)r * C + c] = g * c0f;
        }
    }
}

// Host-side table check + launch geometry.  Returns SEMIDETR_OK or an error (message set).
int plan(const semidetr_set_loss_segment *segs, int nseg, Launch &L, int for_backward)
{
    SEMIDETR_REQUIRE(segs, SEMIDETR_E_BADARG, "set_loss: null segment table");
    SEMIDETR_REQUIRE(nseg >= 1 && nseg <= kMaxSegs, SEMIDETR_E_BADARG, "set_loss: %d segments (1..%d)", nseg, kMaxSegs);
    L.nseg = nseg;
    L.vec4_mask = 0;
    L.block_begin[0] = 0;
    L.t_begin[0] = 0;
    int64_t blocks = 0;
    int T = 0;
    for (int i = 0; i < nseg; ++i) {
        const semidetr_set_loss_segment &s = segs[i];
        L.seg[i] = s;
        SEMIDETR_REQUIRE(s.kind == SEMIDETR_SET_LOSS_MATCHED || s.kind == SEMIDETR_SET_LOSS_DN ||
                             s.kind == SEMIDETR_SET_LOSS_WARMUP,
                         SEMIDETR_E_BADARG, "set_loss: segment %d: unknown kind %d", i, s.kind);
        SEMIDETR_REQUIRE(s.num_layers > 0 && s.num_images > 0 && s.num_query > 0 && s.num_classes > 0, SEMIDETR_E_BADARG,
                         "set_loss: segment %d: bad sizes (nl=%d B=%d Q=%d C=%d)", i, s.num_layers, s.num_images,
                         s.num_query, s.num_classes);
        const int64_t rows = (int64_t)s.num_images * s.num_query;
        SEMIDETR_REQUIRE(rows * s.num_layers * s.num_classes < ((int64_t)1 << 31) && rows * s.num_layers < ((int64_t)1 << 29),
                         SEMIDETR_E_TOOLARGE, "set_loss: segment %d too large for 32-bit row indices", i);
        SEMIDETR_REQUIRE(s.logits, SEMIDETR_E_BADARG, "set_loss: segment %d: null logits", i);
        SEMIDETR_REQUIRE(s.logit_stride[0] >= 0 && s.logit_stride[1] >= 0 && s.logit_stride[2] >= s.num_classes &&
                             (s.num_images == 1 || s.logit_stride[1] >= s.num_query * s.logit_stride[2]) &&
                             (s.num_layers == 1 || s.logit_stride[0] >= s.num_images * s.logit_stride[1]),
                         SEMIDETR_E_BADARG, "set_loss: segment %d: overlapping logit strides", i);
        if (s.boxes)
            SEMIDETR_REQUIRE(s.box_stride[0] >= 0 && s.box_stride[1] >= 0 && s.box_stride[2] >= 4 && s.img_wh,
                             SEMIDETR_E_BADARG, "set_loss: segment %d: bad box strides or null img_wh", i);
        if (s.kind == SEMIDETR_SET_LOSS_DN) {
            SEMIDETR_REQUIRE(s.gt_offsets && s.gt_labels && s.gt_boxes && s.boxes && s.single_pad > 0 && s.dn_groups > 0 &&
                                 (int64_t)s.single_pad * s.dn_groups == s.num_query,
                             SEMIDETR_E_BADARG, "set_loss: dn segment %d: need gt_offsets / gt_labels / gt_boxes / boxes "
                             "and num_query == single_pad * dn_groups (%d != %d * %d)", i, s.num_query, s.single_pad,
                             s.dn_groups);
        } else {
            SEMIDETR_REQUIRE(s.labels, SEMIDETR_E_BADARG, "set_loss: segment %d: null labels", i);
            SEMIDETR_REQUIRE(!s.boxes || (s.bbox_targets && s.bbox_weights), SEMIDETR_E_BADARG,
                             "set_loss: segment %d: boxes without bbox_targets / bbox_weights", i);
            SEMIDETR_REQUIRE(s.kind != SEMIDETR_SET_LOSS_WARMUP || s.metrics, SEMIDETR_E_BADARG,
                             "set_loss: warm-up segment %d: null metrics", i);
        }
        SEMIDETR_REQUIRE(s.gamma >= 0.f && s.iou_eps > 0.f, SEMIDETR_E_BADARG, "set_loss: segment %d: gamma < 0 or eps <= 0", i);
        if (for_backward) {
            SEMIDETR_REQUIRE(!s.grad_boxes || s.boxes, SEMIDETR_E_BADARG, "set_loss: segment %d: grad_boxes without boxes", i);
            SEMIDETR_REQUIRE(((uintptr_t)s.grad_logits & 15) == 0 && ((uintptr_t)s.grad_boxes & 15) == 0, SEMIDETR_E_BADARG,
                             "set_loss: segment %d: gradient buffers must be 16-byte aligned", i);
        }
        const bool v4 = s.num_classes % 4 == 0 && s.logit_stride[0] % 4 == 0 && s.logit_stride[1] % 4 == 0 &&
                    s.logit_stride[2] % 4 == 0 && ((uintptr_t)s.logits & 15) == 0;
        L.vec4_mask |= (int)v4 << i;
        L.chunks[i] = (int)((rows + kRows - 1) / kRows);
        blocks += (int64_t)L.chunks[i] * s.num_layers;
        SEMIDETR_REQUIRE(blocks < (1 << 24), SEMIDETR_E_TOOLARGE, "set_loss: too many rows");
        T += s.num_layers;
        L.block_begin[i + 1] = (int)blocks;
        L.t_begin[i + 1] = T;
    }
    SEMIDETR_REQUIRE(T <= kMaxT, SEMIDETR_E_BADARG, "set_loss: %d (segment, layer) pairs > %d", T, kMaxT);
    return SEMIDETR_OK;
}

}  // namespace

extern "C" int64_t semidetr_set_loss_workspace_bytes(const semidetr_set_loss_segment *segs, int num_segments)
{
    Launch L;
    if (int rc = plan(segs, num_segments, L, 0)) return rc;
    return (int64_t)L.block_begin[L.nseg] * kStats * (int64_t)sizeof(double);
}

extern "C" int semidetr_set_loss_forward_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments,
                                             void *workspace, int64_t workspace_bytes, double *stats, float *norms,
                                             float *losses, float *scales)
{
    Launch L;
    if (int rc = plan(segs, num_segments, L, 0)) return rc;
    const int blocks = L.block_begin[L.nseg];
    SEMIDETR_REQUIRE(workspace && workspace_bytes >= (int64_t)blocks * kStats * (int64_t)sizeof(double), SEMIDETR_E_BADARG,
                     "set_loss: workspace null or smaller than semidetr_set_loss_workspace_bytes()");
    SEMIDETR_REQUIRE(stats && norms, SEMIDETR_E_BADARG, "set_loss: null stats / norms");
    SEMIDETR_REQUIRE(!losses == !scales, SEMIDETR_E_BADARG, "set_loss: losses and scales go together");
    hipStream_t st = semidetr::as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(setloss_fwd_kernel, dim3(blocks), dim3(kThreads), 0, st, L, partial);
    if (int rc = semidetr::launch_status("setloss_fwd_kernel")) return rc;
    hipLaunchKernelGGL(setloss_reduce_kernel, dim3(1), dim3(kThreads), 0, st, L, partial, stats, norms, losses, scales);
    return semidetr::launch_status("setloss_reduce_kernel");
}

extern "C" int semidetr_set_loss_finalize_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments,
                                              const double *stats, const float *norms_local, const float *norms_reduced,
                                              float *losses, float *scales)
{
    Launch L;
    if (int rc = plan(segs, num_segments, L, 0)) return rc;
    SEMIDETR_REQUIRE(stats && norms_local && norms_reduced && losses && scales, SEMIDETR_E_BADARG,
                     "set_loss finalize: null pointer argument");
    hipLaunchKernelGGL(setloss_finalize_kernel, dim3(1), dim3(64), 0, semidetr::as_stream(stream), L, stats, norms_local,
                       norms_reduced, losses, scales);
    return semidetr::launch_status("setloss_finalize_kernel");
}

extern "C" int semidetr_set_loss_backward_f32(void *stream, const semidetr_set_loss_segment *segs, int num_segments,
                                              const float *scales, const float *grad_out)
{
    Launch L;
    if (int rc = plan(segs, num_segments, L, 1)) return rc;
    SEMIDETR_REQUIRE(grad_out, SEMIDETR_E_BADARG, "set_loss backward: null grad_out");
    hipLaunchKernelGGL(setloss_bwd_kernel, dim3(L.block_begin[L.nseg]), dim3(kThreads), 0, semidetr::as_stream(stream), L,
                       scales, grad_out);
    return semidetr::launch_status("setloss_bwd_kernel");
}

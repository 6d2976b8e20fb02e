// Cost-GMM double filter of the unsupervised loss for gfx950 (DinoDetrSSOD.unsup_loss, dino_detr_ssod.py:243-353,
// _fit_gmm :832-890).  Three launches after the LSAP:
//   gmm_match_cost_kernel   one workgroup per image: cost[row, col] at the LSAP pairs -> this rank's segment of the padded
//                           cost buffer (pairs in image order, rows ascending within an image) + the segment's count
//   gmm_fit_kernel          ONE workgroup: a two-component, one-feature GaussianMixture fit in fp64 over every segment of the
//                           buffer (one segment per rank after an all_gather), predict + score_samples, the threshold pick
//   gmm_double_filter_kernel one workgroup per image: keep_base = {g : score >= base_thr}, keep_gmm = {col : cost <= thr},
//                           both compacted in ascending index order, nine outputs gathered into padded per-image slots
//
// The fit follows scikit-learn 1.7.2's arithmetic operation for operation (tests/gmm_ref64.py restates it in numpy):
//   * X is fp32: x * x is rounded to fp32 before it meets the fp64 parameters; the initial means are fp32 too (means_init
//     is an array of two float32 scalars), so the FIRST E-step squares them in fp32;
//   * weighted log prob (diag, one feature) = (-0.5 * (fp32(log 2pi) + ((m^2 p - 2 (x (m p))) + x^2 p)) + log pc) + log w,
//     p = pc^2, and logsumexp of the two terms = max + log1p(exp(min - max)) (scipy 1.15);
//   * M-step: nk = sum r + 10 eps, mean = sum r x / nk, cov = (sum r x^2 / nk - mean^2) + reg_covar, w = nk / (nk0 + nk1),
//     pc = 1 / sqrt(cov); lower bound = mean log_prob_norm of the E-step; stop when |change| < tol or after max_iter;
//   * a final E-step with the last parameters gives labels (argmax, ties -> component 0) and score_samples.
// The sums are taken in a fixed order (per-thread strides, then a shuffle tree, then the four waves in order), so a launch
// is deterministic; they differ from numpy's pairwise sums by a few ulps, which moves a discrete result only on a tie.
// Threshold: the cost of the component-0 point with the highest score; when no point is in component 0, the component-1
// point with the highest score.  TIE RULE: among equal scores the SMALLER cost wins (the reference sorts the costs
// ascending and takes torch.topk's first maximum).  No sorting is needed: the pick is an (argmax score, argmin cost) reduction.
//
// No FMA contraction anywhere in this file: every product and sum is rounded where numpy rounds it.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGt = 8192;                       // per-image gt flags in LDS (the teacher keeps <= max_per_img = 300)
constexpr double kEps10 = 10.0 * 2.220446049250313e-16;

// Sum of NV doubles over the workgroup; every thread gets the same totals (waves added in a fixed order).
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*red)[NV])
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += red[w][k];
        v[k] = t;
    }
}

// (score, cost) argmax with the tie rule: higher score, then smaller cost.  An empty candidate has score -inf and cost +inf.
__device__ __forceinline__ bool better(double s, float x, double bs, float bx)
{
    return s > bs || (s == bs && x < bx);
}

struct Comp {
    double A, B, P, logdet, logw;                  // m^2 p, m p, p, log pc, log w
};

__device__ __forceinline__ Comp make_comp(double msq, double m, double pc, double logw)
{
    Comp c;
    c.P = pc * pc;
    c.A = msq * c.P;
    c.B = m * c.P;
    c.logdet = log(pc);
    c.logw = logw;
    return c;
}

__device__ __forceinline__ double weighted_log_prob(const Comp &c, double x, double x2, double log2pi)
{
    const double lp = (c.A - 2.0 * (x * c.B)) + x2 * c.P;
    return (-0.5 * (log2pi + lp) + c.logdet) + c.logw;
}

__device__ __forceinline__ double lse2(double a, double b)
{
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    return hi + log1p(exp(lo - hi));
}

// Visits every point of the padded multi-segment buffer: thread tid takes points tid, tid + 256, ... of each segment;
// gi = the point's index in the concatenation of the segments.
template <typename F>
__device__ __forceinline__ void for_each_point(const float *__restrict__ values, int64_t value_stride,
                                               const int32_t *__restrict__ counts, int64_t count_stride, int num_segments,
                                               F &&f)
{
    int base = 0;
    for (int s = 0; s < num_segments; ++s) {
        const int c = counts[(int64_t)s * count_stride];
        const float *seg = values + (int64_t)s * value_stride;
        for (int j = threadIdx.x; j < c; j += kThreads) f(base + j, seg[j]);
        base += c;
    }
}

__global__ __launch_bounds__(kThreads) void gmm_fit_kernel(
    const float *__restrict__ values, int64_t value_stride, const int32_t *__restrict__ counts, int64_t count_stride,
    int num_segments, int capacity, double reg_covar, double tol, int max_iter, float *__restrict__ out_thr,
    int32_t *__restrict__ out_labels, double *__restrict__ out_scores, int32_t *__restrict__ out_info)
{
    __shared__ double red[kWaves][7];
    __shared__ float fred[kWaves][2];
    __shared__ double sred[kWaves][2];
    __shared__ float xred[kWaves][2];
    const int tid = threadIdx.x;
    // ---- point count; a segment count outside [0, capacity] is an error (reported, nothing is fitted)
    int n = 0, bad = 0;
    for (int s = 0; s < num_segments; ++s) {
        const int c = counts[(int64_t)s * count_stride];
        bad |= (c < 0 || c > capacity);
        n += (c < 0 || c > capacity) ? 0 : c;
    }
    if (bad) {
        if (tid == 0) {
            out_thr[0] = __builtin_nanf("");
            out_info[0] = 0; out_info[1] = 0; out_info[2] = 2; out_info[3] = n;
        }
        return;
    }
    if (n < 2) {                                   // _fit_gmm: 0 -> 0, one cost -> that cost (no fit)
        for_each_point(values, value_stride, counts, count_stride, num_segments, [&](int gi, float xf) {
            if (tid == 0) out_thr[0] = xf;
            if (out_labels) out_labels[gi] = 0;
            if (out_scores) out_scores[gi] = __builtin_nan("");
        });
        if (tid == 0) {
            if (n == 0) out_thr[0] = 0.f;
            out_info[0] = 0; out_info[1] = 0; out_info[2] = 0; out_info[3] = n;
        }
        return;
    }
    // ---- means_init = [min, max] (fp32)
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for_each_point(values, value_stride, counts, count_stride, num_segments, [&](int, float xf) {
        lo = fminf(lo, xf);
        hi = fmaxf(hi, xf);
    });
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, s, 64));
        hi = fmaxf(hi, __shfl_xor(hi, s, 64));
    }
    if ((tid & 63) == 0) { fred[tid >> 6][0] = lo; fred[tid >> 6][1] = hi; }
    __syncthreads();
    lo = fred[0][0]; hi = fred[0][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { lo = fminf(lo, fred[w][0]); hi = fmaxf(hi, fred[w][1]); }

    const double log2pi = (double)(float)1.8378770664093453;          // np.log(2 pi).astype(float32)
    const float lo2 = lo * lo, hi2 = hi * hi;                        // fp32 squares of the fp32 initial means
    Comp c0 = make_comp((double)lo2, (double)lo, 1.0, log(0.5));
    Comp c1 = make_comp((double)hi2, (double)hi, 1.0, log(0.5));
    double lower = -__builtin_inf();
    int n_iter = 0, converged = 0, err = 0;
    for (int it = 1; it <= max_iter; ++it) {
        n_iter = it;
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // r0, r1, r0 x, r1 x, r0 x^2, r1 x^2, log_prob_norm
        for_each_point(values, value_stride, counts, count_stride, num_segments, [&](int gi, float xf) {
            const float x2f = xf * xf;
            const double x = (double)xf, x2 = (double)x2f;
            const double w0 = weighted_log_prob(c0, x, x2, log2pi), w1 = weighted_log_prob(c1, x, x2, log2pi);
            const double lpn = lse2(w0, w1);
            const double r0 = exp(w0 - lpn), r1 = exp(w1 - lpn);
            acc[0] += r0; acc[1] += r1;
            acc[2] += r0 * x; acc[3] += r1 * x;
            acc[4] += r0 * x2; acc[5] += r1 * x2;
            acc[6] += lpn;
        });
        block_sum<7>(acc, red);
        const double nk0 = acc[0] + kEps10, nk1 = acc[1] + kEps10;
        const double m0 = acc[2] / nk0, m1 = acc[3] / nk1;
        const double v0 = (acc[4] / nk0 - m0 * m0) + reg_covar, v1 = (acc[5] / nk1 - m1 * m1) + reg_covar;
        if (!(v0 > 0.0) || !(v1 > 0.0)) { err = 1; break; }        // sklearn raises (ill-defined empirical covariance)
        const double wsum = nk0 + nk1;
        c0 = make_comp(m0 * m0, m0, 1.0 / sqrt(v0), log(nk0 / wsum));
        c1 = make_comp(m1 * m1, m1, 1.0 / sqrt(v1), log(nk1 / wsum));
        const double lb = acc[6] / (double)n;
        const double change = lb - lower;
        lower = lb;
        if (fabs(change) < tol) { converged = 1; break; }
    }
    if (err) {
        if (tid == 0) {
            out_thr[0] = __builtin_nanf("");
            out_info[0] = n_iter; out_info[1] = 0; out_info[2] = 1; out_info[3] = n;
        }
        return;
    }
    // ---- final E-step: labels, score_samples, the per-component best (score, cost)
    double bs0 = -__builtin_inf(), bs1 = -__builtin_inf();
    float bx0 = __builtin_inff(), bx1 = __builtin_inff();
    int has0 = 0;
    for_each_point(values, value_stride, counts, count_stride, num_segments, [&](int gi, float xf) {
        const float x2f = xf * xf;
        const double x = (double)xf, x2 = (double)x2f;
        const double w0 = weighted_log_prob(c0, x, x2, log2pi), w1 = weighted_log_prob(c1, x, x2, log2pi);
        const int lab = w1 > w0 ? 1 : 0;
        const double sc = lse2(w0, w1);
        if (out_labels) out_labels[gi] = lab;
        if (out_scores) out_scores[gi] = sc;
        // selects, not branches: a branch between the two candidates becomes a pointer select into scratch
        const bool t0 = lab == 0 && better(sc, xf, bs0, bx0), t1 = lab == 1 && better(sc, xf, bs1, bx1);
        has0 |= lab == 0;
        bs0 = t0 ? sc : bs0;
        bx0 = t0 ? xf : bx0;
        bs1 = t1 ? sc : bs1;
        bx1 = t1 ? xf : bx1;
    });
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double os0 = __shfl_xor(bs0, s, 64), os1 = __shfl_xor(bs1, s, 64);
        const float ox0 = __shfl_xor(bx0, s, 64), ox1 = __shfl_xor(bx1, s, 64);
        if (better(os0, ox0, bs0, bx0)) { bs0 = os0; bx0 = ox0; }
        if (better(os1, ox1, bs1, bx1)) { bs1 = os1; bx1 = ox1; }
    }
    has0 = __syncthreads_or(has0);
    if ((tid & 63) == 0) {
        sred[tid >> 6][0] = bs0; sred[tid >> 6][1] = bs1;
        xred[tid >> 6][0] = bx0; xred[tid >> 6][1] = bx1;
    }
    __syncthreads();
    if (tid == 0) {
        bs0 = sred[0][0]; bs1 = sred[0][1]; bx0 = xred[0][0]; bx1 = xred[0][1];
        for (int w = 1; w < kWaves; ++w) {
            if (better(sred[w][0], xred[w][0], bs0, bx0)) { bs0 = sred[w][0]; bx0 = xred[w][0]; }
            if (better(sred[w][1], xred[w][1], bs1, bx1)) { bs1 = sred[w][1]; bx1 = xred[w][1]; }
        }
        out_thr[0] = has0 ? bx0 : bx1;
        out_info[0] = n_iter; out_info[1] = converged; out_info[2] = 0; out_info[3] = n;
    }
}

// cost[row, col] of every LSAP pair -> seg[pair_offsets[b] + k]; block 0 also writes the segment's count.  A pair outside its
// problem (the LSAP reported a failure and left the pair lists unset) reads nothing and gives NaN.
__global__ __launch_bounds__(kThreads) void gmm_match_cost_kernel(
    const float *__restrict__ cost, const int32_t *__restrict__ gt_offsets, const int32_t *__restrict__ pair_offsets,
    const int64_t *__restrict__ rows, const int64_t *__restrict__ cols, int num_images, int Q, float *__restrict__ seg,
    int32_t *__restrict__ seg_count)
{
    const int b = blockIdx.x;
    const int g0 = gt_offsets[b], G = gt_offsets[b + 1] - g0;
    const int p0 = pair_offsets[b], np_ = pair_offsets[b + 1] - p0;
    const float *cb = cost + (int64_t)Q * g0;
    for (int k = threadIdx.x; k < np_; k += kThreads) {
        const int64_t r = rows[p0 + k], c = cols[p0 + k];
        seg[p0 + k] = (r >= 0 && r < Q && c >= 0 && c < G) ? cb[c * Q + r] : __builtin_nanf("");
    }
    if (b == 0 && threadIdx.x == 0) seg_count[0] = pair_offsets[num_images];
}

__global__ __launch_bounds__(kThreads) void gmm_double_filter_kernel(
    const float *__restrict__ seg, const int32_t *__restrict__ pair_offsets, const int64_t *__restrict__ cols,
    const float *__restrict__ thr_ptr, const float *__restrict__ gt_bboxes, const int64_t *__restrict__ gt_labels,
    const float *__restrict__ gt_scores, const float *__restrict__ det_bboxes, const int64_t *__restrict__ det_labels,
    const float *__restrict__ det_scores, const int32_t *__restrict__ gt_offsets, int num_images, float base_thr, int slot,
    float *__restrict__ ob_boxes, int64_t *__restrict__ ob_labels, float *__restrict__ ob_scores, float *__restrict__ og_boxes,
    int64_t *__restrict__ og_labels, float *__restrict__ og_scores, float *__restrict__ od_boxes, int64_t *__restrict__ od_labels,
    float *__restrict__ od_scores, int32_t *__restrict__ out_counts)
{
    __shared__ unsigned char gmm_keep[kMaxGt];
    __shared__ int wave_cnt[2][kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g0 = gt_offsets[b], G = gt_offsets[b + 1] - g0;
    const int p0 = pair_offsets[b], np_ = pair_offsets[b + 1] - p0;
    const float thr = thr_ptr[0];
    for (int g = tid; g < G; g += kThreads) gmm_keep[g] = 0;
    __syncthreads();
    for (int k = tid; k < np_; k += kThreads) {
        const int64_t c = cols[p0 + k];
        if (seg[p0 + k] <= thr && c >= 0 && c < G) gmm_keep[c] = 1;       // LSAP columns are distinct: one writer per flag
    }
    __syncthreads();
    int nb = 0, nu = 0;
    const int64_t o0 = (int64_t)b * slot;
    for (int i0 = 0; i0 < G; i0 += kThreads) {
        const int g = i0 + tid;
        bool kb = false, ku = false;
        if (g < G) {
            kb = gt_scores[g0 + g] >= base_thr;
            ku = kb || gmm_keep[g];
        }
        const unsigned long long mb = __ballot(kb), mu = __ballot(ku);
        const unsigned long long below = (1ull << lane) - 1ull;
        __syncthreads();
        if (lane == 0) { wave_cnt[0][wv] = __popcll(mb); wave_cnt[1][wv] = __popcll(mu); }
        __syncthreads();
        int wb = 0, wu = 0, tb = 0, tu = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wv) { wb += wave_cnt[0][w]; wu += wave_cnt[1][w]; }
            tb += wave_cnt[0][w]; tu += wave_cnt[1][w];
        }
        const int64_t src = g0 + g;
        if (kb) {
            const int64_t o = o0 + nb + wb + __popcll(mb & below);
            for (int j = 0; j < 4; ++j) ob_boxes[4 * o + j] = gt_bboxes[4 * src + j];
            ob_labels[o] = gt_labels[src];
            ob_scores[o] = gt_scores[src];
        }
        if (ku) {
            const int64_t o = o0 + nu + wu + __popcll(mu & below);
            for (int j = 0; j < 4; ++j) {
                og_boxes[4 * o + j] = gt_bboxes[4 * src + j];
                od_boxes[4 * o + j] = det_bboxes[4 * src + j];
            }
            og_labels[o] = gt_labels[src];
            og_scores[o] = gt_scores[src];
            od_labels[o] = det_labels[src];
            od_scores[o] = det_scores[src];
        }
        nb += tb;
        nu += tu;
    }
    if (tid == 0) { out_counts[b] = nb; out_counts[num_images + b] = nu; }
}

}  // namespace

extern "C" int semidetr_gmm_fit_f64(void *stream, const float *values, int64_t value_stride, const int32_t *counts,
                                    int64_t count_stride, int num_segments, int capacity, int covariance_type,
                                    double reg_covar, double tol, int max_iter, float *out_thr, int32_t *out_labels,
                                    double *out_scores, int32_t *out_info)
{
    SEMIDETR_REQUIRE(covariance_type == SEMIDETR_GMM_COVARIANCE_DIAG, SEMIDETR_E_BADARG,
                     "gmm_fit: covariance type %d is not supported (only SEMIDETR_GMM_COVARIANCE_DIAG = 'diag')",
                     covariance_type);
    SEMIDETR_REQUIRE(num_segments >= 1 && capacity >= 0, SEMIDETR_E_BADARG,
                     "gmm_fit: need num_segments >= 1 and capacity >= 0 (got %d, %d)", num_segments, capacity);
    SEMIDETR_REQUIRE(value_stride >= capacity && count_stride >= 1 && (int64_t)num_segments * capacity < (1ll << 31),
                     SEMIDETR_E_BADARG, "gmm_fit: bad segment strides (value_stride %lld < capacity %d or count_stride < 1)",
                     (long long)value_stride, capacity);
    SEMIDETR_REQUIRE(max_iter >= 1 && tol >= 0.0 && reg_covar >= 0.0, SEMIDETR_E_BADARG,
                     "gmm_fit: need max_iter >= 1, tol >= 0, reg_covar >= 0");
    SEMIDETR_REQUIRE((values || capacity == 0) && counts && out_thr && out_info, SEMIDETR_E_BADARG,
                     "gmm_fit: null pointer argument");
    hipLaunchKernelGGL(gmm_fit_kernel, dim3(1), dim3(kThreads), 0, semidetr::as_stream(stream), values, value_stride, counts,
                       count_stride, num_segments, capacity, reg_covar, tol, max_iter, out_thr, out_labels, out_scores,
                       out_info);
    return semidetr::launch_status("gmm_fit_kernel");
}

extern "C" int semidetr_gmm_match_costs_f32(void *stream, const float *cost, const int32_t *gt_offsets,
                                            const int32_t *pair_offsets, const int64_t *rows, const int64_t *cols,
                                            int num_images, int num_query, int num_pairs, int capacity, float *out_seg,
                                            int32_t *out_count)
{
    SEMIDETR_REQUIRE(num_images >= 0 && num_query >= 0 && num_pairs >= 0, SEMIDETR_E_BADARG,
                     "gmm_match_costs: negative size");
    SEMIDETR_REQUIRE(num_pairs <= capacity, SEMIDETR_E_BADARG,
                     "gmm_match_costs: %d matched pairs exceed the segment capacity %d", num_pairs, capacity);
    SEMIDETR_REQUIRE(out_count && (out_seg || capacity == 0), SEMIDETR_E_BADARG, "gmm_match_costs: null pointer argument");
    if (num_images == 0) {
        SEMIDETR_REQUIRE(num_pairs == 0, SEMIDETR_E_BADARG, "gmm_match_costs: pairs without images");
        return hipMemsetAsync(out_count, 0, sizeof(int32_t), semidetr::as_stream(stream)) == hipSuccess
                   ? SEMIDETR_OK : semidetr::fail(-1, "gmm_match_costs: hipMemsetAsync failed");
    }
    SEMIDETR_REQUIRE(gt_offsets && pair_offsets && (num_pairs == 0 || (cost && rows && cols)), SEMIDETR_E_BADARG,
                     "gmm_match_costs: null pointer argument");
    hipLaunchKernelGGL(gmm_match_cost_kernel, dim3(num_images), dim3(kThreads), 0, semidetr::as_stream(stream), cost,
                       gt_offsets, pair_offsets, rows, cols, num_images, num_query, out_seg, out_count);
    return semidetr::launch_status("gmm_match_cost_kernel");
}

extern "C" int semidetr_gmm_double_filter_f32(void *stream, const float *seg_costs, const int32_t *pair_offsets,
                                              const int64_t *cols, const float *thr, const float *gt_bboxes,
                                              const int64_t *gt_labels, const float *gt_scores, const float *det_bboxes,
                                              const int64_t *det_labels, const float *det_scores, const int32_t *gt_offsets,
                                              int num_images, int max_gt, float base_thr, int slot, float *out_base_boxes,
                                              int64_t *out_base_labels, float *out_base_scores, float *out_gmm_boxes,
                                              int64_t *out_gmm_labels, float *out_gmm_scores, float *out_det_boxes,
                                              int64_t *out_det_labels, float *out_det_scores, int32_t *out_counts)
{
    SEMIDETR_REQUIRE(num_images >= 0 && max_gt >= 0, SEMIDETR_E_BADARG, "gmm_double_filter: negative size");
    if (num_images == 0) return SEMIDETR_OK;
    SEMIDETR_REQUIRE(max_gt <= slot, SEMIDETR_E_BADARG,
                     "gmm_double_filter: %d pseudo boxes in an image exceed the output slot of %d", max_gt, slot);
    SEMIDETR_REQUIRE(max_gt <= kMaxGt, SEMIDETR_E_BADARG, "gmm_double_filter: %d pseudo boxes in an image (at most %d)",
                     max_gt, kMaxGt);
    SEMIDETR_REQUIRE(pair_offsets && gt_offsets && thr && out_counts, SEMIDETR_E_BADARG,
                     "gmm_double_filter: null pointer argument");
    SEMIDETR_REQUIRE(max_gt == 0 || (seg_costs && cols && gt_bboxes && gt_labels && gt_scores && det_bboxes && det_labels &&
                                     det_scores && out_base_boxes && out_base_labels && out_base_scores && out_gmm_boxes &&
                                     out_gmm_labels && out_gmm_scores && out_det_boxes && out_det_labels && out_det_scores),
                     SEMIDETR_E_BADARG, "gmm_double_filter: null pointer argument");
    hipLaunchKernelGGL(gmm_double_filter_kernel, dim3(num_images), dim3(kThreads), 0, semidetr::as_stream(stream), seg_costs,
                       pair_offsets, cols, thr, gt_bboxes, gt_labels, gt_scores, det_bboxes, det_labels, det_scores,
                       gt_offsets, num_images, base_thr, slot, out_base_boxes, out_base_labels, out_base_scores, out_gmm_boxes,
                       out_gmm_labels, out_gmm_scores, out_det_boxes, out_det_labels, out_det_scores, out_counts);
    return semidetr::launch_status("gmm_double_filter_kernel");
}

// De-noising and consistency queries of DINO / Semi-DETR (include/semidetr_hip.h, "De-noising and consistency queries").
//
// The reference builds them with a few hundred tiny torch ops and several host round trips per call
// (dn_components.py:6-274, dino_detr_ssod.py:484-760).  Every index in them is a closed form of the per-image list
// lengths, so here the lengths travel as kernel arguments and one launch writes every output: the de-noising rows (one
// wavefront per (image, slot) row: label flip, box noise, inverse sigmoid, embedding row copy), the scattered projector
// rows of the consistency part and the (tgt, tgt) attention mask (16 bytes per lane) run on disjoint workgroup ranges of
// the same grid.  The launches are latency-bound; what matters is that there are two of them, not occupancy.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaskBytesPerBlock = kThreads * 16;

__device__ inline int layout_pad(const semidetr_dn_layout &L) { return L.single_pad * L.groups; }

// (image, slot) row -> list row k; false for a padding slot
__device__ inline bool slot_row(const semidetr_dn_layout &L, int row, int &b, int &s, int &i, int &j, int &k)
{
    const int pad = layout_pad(L);
    b = row / pad;
    s = row - b * pad;
    i = s / L.single_pad;
    j = s - i * L.single_pad;
    const int o = L.offsets[b];
    k = i * L.offsets[L.num_images] + o + j;
    return j < L.offsets[b + 1] - o;
}

__device__ inline float inverse_sigmoid(float x)          // mmdet transformer.py:358, eps 1e-5
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

__device__ inline void copy_row(float *dst, const float *src, int H, bool vec4, int lane, bool nan_fill)
{
    const float fill = nan_fill ? __builtin_nanf("") : 0.f;
    if (vec4) {
        float4 *d = reinterpret_cast<float4 *>(dst);
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        for (int c = lane; c < H / 4; c += 64) d[c] = src ? s4[c] : make_float4(fill, fill, fill, fill);
    } else {
        for (int c = lane; c < H; c += 64) dst[c] = src ? src[c] : fill;
    }
}

struct BuildPlan {
    int rows_dn, rows_cons;            // (image, slot) rows of the two row jobs
    int blocks_dn, blocks_cons, blocks_mask;
    int pad1, pad2, tgt;
    int vec4;
};

__global__ __launch_bounds__(kThreads) void dn_build_kernel(const semidetr_dn_build p, const BuildPlan pl)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int blk = blockIdx.x;
    const int H = p.hidden_dim;
    if (blk < pl.blocks_dn) {
        const int row = blk * kWaves + wave;
        if (row >= pl.rows_dn) return;
        int b, s, i, j, k;
        const bool valid = slot_row(p.dn, row, b, s, i, j, k);
        const bool standin = p.src_counts[b] == 0;
        if (lane == 1 && p.pad_mask) p.pad_mask[row] = standin ? 1 : 0;
        float *ql = p.query_label + (int64_t)row * H;
        if (!valid) {
            copy_row(ql, nullptr, H, pl.vec4, lane, false);
            if (lane == 0) *reinterpret_cast<float4 *>(p.query_bbox + 4 * (int64_t)row) = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
        const float *u = p.noise + (int64_t)k * SEMIDETR_DN_NOISE_COLS;
        int64_t lab = standin ? (int64_t)(int)(p.image_noise[b] * 80.f) : p.labels[b][j];
        if (p.label_noise_threshold > 0.f && u[0] < p.label_noise_threshold) {
            const int nl = (int)(u[1] * (float)p.num_classes);
            lab = nl < p.num_classes - 1 ? nl : p.num_classes - 1;
        }
        const bool in_table = lab >= 0 && lab < p.num_embeddings;
        copy_row(ql, in_table ? p.label_weight + lab * H : nullptr, H, pl.vec4, lane, true);
        if (lane != 0) return;
        p.known_bid[k] = b;
        p.map_known_indice[k] = s;
        p.noised_labels[k] = lab;
        float cx = 0.5f, cy = 0.5f, w = 0.5f, h = 0.5f;
        if (!standin) {
            const float *bx = p.boxes[b] + (int64_t)j * p.box_stride;
            cx = bx[0], cy = bx[1], w = bx[2], h = bx[3];
        }
        if (p.box_noise_scale > 0.f) {
            const float hw = w * 0.5f, hh = h * 0.5f, sc = p.box_noise_scale;
            const float add = (i & 1) ? 1.f : 0.f;
            float c[4] = {cx - hw, cy - hh, cx + hw, cy + hh};
            const float d[4] = {hw, hh, hw, hh};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float r = (u[6 + e] + add) * (u[2 + e] >= 0.5f ? 1.f : -1.f);
                c[e] = fminf(fmaxf(c[e] + (r * d[e]) * sc, 0.f), 1.f);
            }
            cx = (c[0] + c[2]) * 0.5f, cy = (c[1] + c[3]) * 0.5f, w = c[2] - c[0], h = c[3] - c[1];
        }
        *reinterpret_cast<float4 *>(p.query_bbox + 4 * (int64_t)row) =
            make_float4(inverse_sigmoid(cx), inverse_sigmoid(cy), inverse_sigmoid(w), inverse_sigmoid(h));
        return;
    }
    blk -= pl.blocks_dn;
    if (blk < pl.blocks_cons) {
        const int row = blk * kWaves + wave;
        if (row >= pl.rows_cons) return;
        int b, s, i, j, k;
        const bool valid = slot_row(p.cons, row, b, s, i, j, k);
        copy_row(p.cons_label + (int64_t)row * H, valid ? p.cons_rows + (int64_t)k * H : nullptr, H, pl.vec4, lane, false);
        return;
    }
    blk -= pl.blocks_cons;
    // attention mask: 16 consecutive bytes of the flat (tgt, tgt) matrix per lane
    const int tgt = pl.tgt, P = pl.pad1 + pl.pad2;
    const int64_t total = (int64_t)tgt * tgt;
    const int64_t at = ((int64_t)blk * kThreads + threadIdx.x) * 16;
    if (at >= total) return;
    int r = (int)(at / tgt), c = (int)(at - (int64_t)r * tgt);
    const int n = total - at < 16 ? (int)(total - at) : 16;
    const int g2 = 2 * p.dn.single_pad;
    unsigned words[4] = {0u, 0u, 0u, 0u};
    int lo = 0, hi = 0, row_of = -1;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (row_of != r) {                 // the columns of r's own group stay visible
            row_of = r;
            if (r >= P) lo = hi = 0;
            else if (r < pl.pad1) lo = r / p.cons.single_pad * p.cons.single_pad, hi = lo + p.cons.single_pad;
            else lo = pl.pad1 + (r - pl.pad1) / g2 * g2, hi = lo + g2;
        }
        const unsigned m = c < P && !(c >= lo && c < hi);
        words[e >> 2] |= m << (8 * (e & 3));
        if (++c == tgt) c = 0, ++r;
    }
    if (n == 16) {
        *reinterpret_cast<uint4 *>(p.attn_mask + at) = make_uint4(words[0], words[1], words[2], words[3]);
    } else {                               // the last lane of the matrix
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e < n) p.attn_mask[at + e] = (unsigned char)((words[e >> 2] >> (8 * (e & 3))) & 1u);
    }
}

__global__ __launch_bounds__(kThreads) void dn_consistency_kernel(const semidetr_dn_consistency p, int rows)
{
    const int row = blockIdx.x * kThreads + threadIdx.x;
    if (row >= rows) return;
    int b, s, i, j, k;
    const bool valid = slot_row(p.cons, row, b, s, i, j, k);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        const bool sub = p.src_counts[b] == 0;
        const float W = p.tgt_wh[b][0], Hh = p.tgt_wh[b][1];
        float x1 = W * 0.25f, y1 = Hh * 0.25f, x2 = W * 0.75f, y2 = Hh * 0.75f;
        if (!sub) {
            const float *bx = p.pseudo_boxes[b] + (int64_t)j * p.pseudo_stride;
            x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
        }
        const float cx = (x1 + x2) / 2.f / W, cy = (y1 + y2) / 2.f / Hh, w = (x2 - x1) / W, h = (y2 - y1) / Hh;
        q = make_float4(inverse_sigmoid(cx), inverse_sigmoid(cy), inverse_sigmoid(w), inverse_sigmoid(h));
        p.known_bid[k] = (float)b;
        p.map_known_indice[k] = s;
        if (p.rois) {
            const float Ws = p.src_wh[b][0], Hs = p.src_wh[b][1];
            float r1 = Ws * 0.25f, r2 = Hs * 0.25f, r3 = Ws * 0.75f, r4 = Hs * 0.75f;
            if (!sub) {
                const float *dx = p.det_boxes[b] + (int64_t)j * p.det_stride;
                r1 = dx[0], r2 = dx[1], r3 = dx[2], r4 = dx[3];
            }
            float *ro = p.rois + 5 * (int64_t)k;
            ro[0] = (float)b, ro[1] = r1, ro[2] = r2, ro[3] = r3, ro[4] = r4;
        }
        if (p.loss_weights) p.loss_weights[k] = sub ? 0.f : p.loss_weight;
    }
    *reinterpret_cast<float4 *>(p.query_bbox + 4 * (int64_t)row) = q;
}

// One workgroup per embedding row, a lane per channel, the K noised labels walked in index order: a fixed summation order
// without float atomics.  Each wavefront finds its matches 64 labels at a time with a ballot.
__global__ __launch_bounds__(kThreads) void dn_label_bwd_kernel(const float *__restrict__ grad, const int64_t *__restrict__ bid,
                                                               const int64_t *__restrict__ map,
                                                               const int64_t *__restrict__ noised, int K, int B, int pad,
                                                               int H, float *__restrict__ grad_weight)
{
    const int e = blockIdx.x, lane = threadIdx.x & 63;
    for (int c0 = 0; c0 < H; c0 += kThreads) {
        const int c = c0 + threadIdx.x;
        float acc = 0.f;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int kk = k0 + lane;
            unsigned long long m = __ballot(kk < K && noised[kk] == e);
            while (m) {
                const int k = k0 + __builtin_ctzll(m);
                m &= m - 1;
                const int64_t bb = bid[k], ss = map[k];
                if (bb >= 0 && bb < B && ss >= 0 && ss < pad && c < H) acc += grad[(bb * pad + ss) * H + c];
            }
        }
        if (c < H) grad_weight[(int64_t)e * H + c] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void dn_gather_rows_kernel(const semidetr_dn_layout L, const float *__restrict__ grad,
                                                                 int H, int rows, int vec4, float *__restrict__ out)
{
    const int row = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= rows) return;
    int b, s, i, j, k;
    if (!slot_row(L, row, b, s, i, j, k)) return;
    copy_row(out + (int64_t)k * H, grad + (int64_t)row * H, H, vec4, threadIdx.x & 63, false);
}

// Host-side layout check.  `allow_empty`: groups == 0 means "no such part".
int check_layout(const semidetr_dn_layout &L, const char *what, bool allow_empty)
{
    if (allow_empty && L.groups == 0) return SEMIDETR_OK;
    SEMIDETR_REQUIRE(L.num_images >= 1 && L.num_images <= SEMIDETR_DN_MAX_IMAGES, SEMIDETR_E_BADARG,
                     "dn_query: %s: %d images (1..%d)", what, L.num_images, SEMIDETR_DN_MAX_IMAGES);
    SEMIDETR_REQUIRE(L.single_pad >= 1 && L.groups >= 1, SEMIDETR_E_BADARG, "dn_query: %s: single_pad %d / groups %d < 1", what,
                     L.single_pad, L.groups);
    SEMIDETR_REQUIRE(L.offsets[0] == 0, SEMIDETR_E_BADARG, "dn_query: %s: offsets[0] = %d", what, L.offsets[0]);
    for (int b = 0; b < L.num_images; ++b) {
        const int n = L.offsets[b + 1] - L.offsets[b];
        SEMIDETR_REQUIRE(n >= 0 && n <= L.single_pad, SEMIDETR_E_BADARG, "dn_query: %s: image %d has %d rows (0..single_pad %d)",
                         what, b, n, L.single_pad);
    }
    SEMIDETR_REQUIRE((int64_t)L.single_pad * L.groups * L.num_images < ((int64_t)1 << 22) &&
                         (int64_t)L.groups * L.offsets[L.num_images] < ((int64_t)1 << 24),
                     SEMIDETR_E_TOOLARGE, "dn_query: %s: too many slots for 32-bit indices", what);
    return SEMIDETR_OK;
}

}  // namespace

extern "C" int semidetr_dn_build_f32(void *stream, const semidetr_dn_build *params)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "dn_query build: null pointer argument");
    const semidetr_dn_build &p = *params;
    if (int rc = check_layout(p.dn, "dn layout", false)) return rc;
    if (int rc = check_layout(p.cons, "consistency layout", true)) return rc;
    const int B = p.dn.num_images, N = p.dn.offsets[B];
    SEMIDETR_REQUIRE(p.dn.groups % 2 == 0, SEMIDETR_E_BADARG, "dn_query build: dn groups %d must be even (positive + negative)",
                     p.dn.groups);
    SEMIDETR_REQUIRE(p.num_known == p.dn.groups * N, SEMIDETR_E_BADARG,
                     "dn_query build: num_known %d inconsistent with the offsets (%d groups x %d rows)", p.num_known,
                     p.dn.groups, N);
    SEMIDETR_REQUIRE(p.cons.groups == 0 || p.cons.num_images == B, SEMIDETR_E_BADARG,
                     "dn_query build: the two layouts disagree on the batch size (%d, %d)", B, p.cons.num_images);
    SEMIDETR_REQUIRE(p.hidden_dim >= 1 && p.hidden_dim <= 8192 && p.num_embeddings >= 1 && p.num_classes >= 1 &&
                         p.num_queries >= 0 && p.box_stride >= 4,
                     SEMIDETR_E_BADARG, "dn_query build: bad sizes (hidden %d, embeddings %d, classes %d, queries %d, stride %d)",
                     p.hidden_dim, p.num_embeddings, p.num_classes, p.num_queries, p.box_stride);
    SEMIDETR_REQUIRE(p.label_weight && p.noise && p.query_label && p.query_bbox && p.known_bid && p.map_known_indice &&
                         p.noised_labels,
                     SEMIDETR_E_BADARG, "dn_query build: null pointer argument");
    SEMIDETR_REQUIRE(((uintptr_t)p.query_bbox & 15) == 0 && ((uintptr_t)p.attn_mask & 15) == 0, SEMIDETR_E_BADARG,
                     "dn_query build: query_bbox / attn_mask must be 16-byte aligned");
    bool any_standin = false;
    for (int b = 0; b < B; ++b) {
        const int n = p.dn.offsets[b + 1] - p.dn.offsets[b];
        SEMIDETR_REQUIRE(p.src_counts[b] == n || (p.src_counts[b] == 0 && n == 1), SEMIDETR_E_BADARG,
                         "dn_query build: image %d: %d ground truths against %d layout rows", b, p.src_counts[b], n);
        SEMIDETR_REQUIRE(p.src_counts[b] == 0 || (p.labels[b] && p.boxes[b]), SEMIDETR_E_BADARG,
                         "dn_query build: image %d: null labels / boxes", b);
        any_standin |= p.src_counts[b] == 0 && n == 1;
    }
    SEMIDETR_REQUIRE(!any_standin || p.image_noise, SEMIDETR_E_BADARG, "dn_query build: stand-in image without image_noise");
    SEMIDETR_REQUIRE(!p.cons_rows == !p.cons_label && (!p.cons_rows || p.cons.groups > 0), SEMIDETR_E_BADARG,
                     "dn_query build: cons_rows, cons_label and the consistency layout go together");
    BuildPlan pl;
    pl.pad1 = p.cons.groups ? p.cons.single_pad * p.cons.groups : 0;
    pl.pad2 = p.dn.single_pad * p.dn.groups;
    pl.tgt = pl.pad1 + pl.pad2 + p.num_queries;
    SEMIDETR_REQUIRE(pl.tgt < (1 << 15), SEMIDETR_E_TOOLARGE, "dn_query build: %d queries in all", pl.tgt);
    pl.rows_dn = B * pl.pad2;
    pl.rows_cons = p.cons_rows ? B * pl.pad1 : 0;
    SEMIDETR_REQUIRE((int64_t)(pl.rows_dn + pl.rows_cons) * p.hidden_dim < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                     "dn_query build: outputs too large for 32-bit indices");
    pl.blocks_dn = (pl.rows_dn + kWaves - 1) / kWaves;
    pl.blocks_cons = (pl.rows_cons + kWaves - 1) / kWaves;
    pl.blocks_mask = p.attn_mask ? (int)(((int64_t)pl.tgt * pl.tgt + kMaskBytesPerBlock - 1) / kMaskBytesPerBlock) : 0;
    pl.vec4 = p.hidden_dim % 4 == 0 && ((uintptr_t)p.label_weight & 15) == 0 && ((uintptr_t)p.query_label & 15) == 0 &&
              ((uintptr_t)p.cons_rows & 15) == 0 && ((uintptr_t)p.cons_label & 15) == 0;
    hipLaunchKernelGGL(dn_build_kernel, dim3(pl.blocks_dn + pl.blocks_cons + pl.blocks_mask), dim3(kThreads), 0,
                       semidetr::as_stream(stream), p, pl);
    return semidetr::launch_status("dn_build_kernel");
}

extern "C" int semidetr_dn_consistency_f32(void *stream, const semidetr_dn_consistency *params)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "dn_query consistency: null pointer argument");
    const semidetr_dn_consistency &p = *params;
    if (int rc = check_layout(p.cons, "consistency layout", false)) return rc;
    const int B = p.cons.num_images;
    SEMIDETR_REQUIRE(p.num_known == p.cons.groups * p.cons.offsets[B], SEMIDETR_E_BADARG,
                     "dn_query consistency: num_known %d inconsistent with the offsets (%d groups x %d rows)", p.num_known,
                     p.cons.groups, p.cons.offsets[B]);
    SEMIDETR_REQUIRE(p.query_bbox && p.known_bid && p.map_known_indice, SEMIDETR_E_BADARG,
                     "dn_query consistency: null pointer argument");
    SEMIDETR_REQUIRE(((uintptr_t)p.query_bbox & 15) == 0 && p.pseudo_stride >= 4 && (!p.rois || p.det_stride >= 4),
                     SEMIDETR_E_BADARG, "dn_query consistency: query_bbox must be 16-byte aligned, box strides >= 4");
    for (int b = 0; b < B; ++b) {
        const int n = p.cons.offsets[b + 1] - p.cons.offsets[b];
        SEMIDETR_REQUIRE(p.src_counts[b] == n || (p.src_counts[b] == 0 && n == 1), SEMIDETR_E_BADARG,
                         "dn_query consistency: image %d: %d boxes against %d layout rows", b, p.src_counts[b], n);
        SEMIDETR_REQUIRE(p.src_counts[b] == 0 || (p.pseudo_boxes[b] && (!p.rois || p.det_boxes[b])), SEMIDETR_E_BADARG,
                         "dn_query consistency: image %d: null boxes", b);
        SEMIDETR_REQUIRE(p.tgt_wh[b][0] > 0.f && p.tgt_wh[b][1] > 0.f, SEMIDETR_E_BADARG,
                         "dn_query consistency: image %d: non-positive image size", b);
    }
    const int rows = B * p.cons.single_pad * p.cons.groups;
    hipLaunchKernelGGL(dn_consistency_kernel, dim3((rows + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       semidetr::as_stream(stream), p, rows);
    return semidetr::launch_status("dn_consistency_kernel");
}

extern "C" int semidetr_dn_label_backward_f32(void *stream, const float *grad_query_label, const int64_t *known_bid,
                                              const int64_t *map_known_indice, const int64_t *noised_labels, int num_known,
                                              int num_images, int pad_size, int hidden_dim, int num_embeddings,
                                              float *grad_weight)
{
    SEMIDETR_REQUIRE(grad_query_label && known_bid && map_known_indice && noised_labels && grad_weight, SEMIDETR_E_BADARG,
                     "dn_query label backward: null pointer argument");
    SEMIDETR_REQUIRE(num_known >= 1 && num_images >= 1 && pad_size >= 1 && hidden_dim >= 1 && num_embeddings >= 1,
                     SEMIDETR_E_BADARG, "dn_query label backward: bad sizes (K %d, B %d, pad %d, hidden %d, embeddings %d)",
                     num_known, num_images, pad_size, hidden_dim, num_embeddings);
    SEMIDETR_REQUIRE((int64_t)num_images * pad_size * hidden_dim < ((int64_t)1 << 31) && num_embeddings < (1 << 20),
                     SEMIDETR_E_TOOLARGE, "dn_query label backward: too large for 32-bit indices");
    hipLaunchKernelGGL(dn_label_bwd_kernel, dim3(num_embeddings), dim3(kThreads), 0, semidetr::as_stream(stream),
                       grad_query_label, known_bid, map_known_indice, noised_labels, num_known, num_images, pad_size,
                       hidden_dim, grad_weight);
    return semidetr::launch_status("dn_label_bwd_kernel");
}

extern "C" int semidetr_dn_gather_rows_f32(void *stream, const semidetr_dn_layout *layout, const float *grad_label,
                                           int hidden_dim, float *grad_rows)
{
    SEMIDETR_REQUIRE(layout && grad_label && grad_rows, SEMIDETR_E_BADARG, "dn_query gather: null pointer argument");
    if (int rc = check_layout(*layout, "layout", false)) return rc;
    SEMIDETR_REQUIRE(hidden_dim >= 1 && hidden_dim <= 8192, SEMIDETR_E_BADARG, "dn_query gather: hidden %d", hidden_dim);
    const int rows = layout->num_images * layout->single_pad * layout->groups;
    SEMIDETR_REQUIRE((int64_t)rows * hidden_dim < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                     "dn_query gather: too large for 32-bit indices");
    const int vec4 = hidden_dim % 4 == 0 && ((uintptr_t)grad_label & 15) == 0 && ((uintptr_t)grad_rows & 15) == 0;
    hipLaunchKernelGGL(dn_gather_rows_kernel, dim3((rows + kWaves - 1) / kWaves), dim3(kThreads), 0,
                       semidetr::as_stream(stream), *layout, grad_label, hidden_dim, rows, vec4, grad_rows);
    return semidetr::launch_status("dn_gather_rows_kernel");
}

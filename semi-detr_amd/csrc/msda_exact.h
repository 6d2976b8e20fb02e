// Exact backward of MSDA (semidetr_msda_backward_exact_f32; D == 32, fp32): grad_value[n, row, m, d] is the EXACT sum of its fp32
// contributions, rounded once -- its bits are a function of the SET of contributions, so they do not depend on launch order,
// on the kernel that produced the entries, on the image's position in the batch or on the order of queries / points.
// Included by msda.hip after msda_geom.h (sample_setup: the one copy of the skip test and the cells); the kernels live in
// namespace semidetr_exact and carry no IO policy (the reduce stage needs neither geometry nor policy: a fused or a 16-bit front
// end can feed it the same entries).
//
// A contribution is defined here, once: for a valid corner k of a sample with attention weight a,
//     w = fl(a * c_k),  c_k = fl(product of the two fp32 bilinear factors),  contribution[d] = fl(w * grad_out[n, q, m, d]).
// Every operation is a single individually rounded multiply or subtract (mul_rn / sub_rn: nothing to contract).
//
// Pipeline (integer atomics and plain stores only; no float atomic anywhere):
//   clear   count[(n * M + m) * S + row] = 0
//   count   one thread per sample (n, q, m, l, p): atomicAdd(count[row], 1) per valid corner
//   scan    per (n, m): start[row] = exclusive prefix of the S counts; count[] becomes the fill cursor (reset to 0).  Each (n, m)
//           owns a slice of Lq * L * P * 4 entries (its worst case), so nothing is scanned across (n, m)
//   fill    one thread per sample again: slot = start[row] + atomicAdd(cursor[row], 1), entry {grad_out row, w} (8 bytes).  The
//           slot order is run-dependent -- harmless, the sum does not depend on order
//   reduce  32 lanes (lane = channel) per destination row walk the row's entries: one 128-byte grad_out row load, one multiply
//           and one accumulator add per entry; the lanes round and store, a row without entries stores zeros.  grad_value is
//           written exactly once per element and needs no fill.  Rows longer than kSplitLen are shared by the workgroup's eight
//           lane groups and merged through LDS (the merge is exact)
#pragma once

#include "msda_exactsum.h"

namespace semidetr_exact {

constexpr int kChannels = 32;
constexpr int kReduceThreads = 256, kReduceGroups = kReduceThreads / kChannels;      // destination rows per workgroup
constexpr int kSplitLen = 256;      // a row with more entries than this is summed by all lane groups of its workgroup
constexpr int kScanThreads = 256;

// what semidetr_msda_last_kernels reports after the exact backward: the gather of the default route, then this header's kernels
constexpr const char *kLaunchedKernels = "msda_bwd_gather_d32+exact_clear+exact_count+exact_scan+exact_fill+exact_reduce";

struct Entry {
    unsigned grow;      // (n * Lq + q) * M + m: the grad_out row
    float w;            // fl(a * c_k)
};
static_assert(sizeof(Entry) == 8, "the workspace is sized with 8-byte entries");

// workspace layout: count / cursor words, start words (each padded to 256 bytes), then the entries
struct Workspace {
    size_t words;            // N * M * S
    size_t counts_bytes;     // padded
    size_t slice;            // entries per (n, m): Lq * L * P * 4
    size_t total_bytes;
};
inline Workspace workspace_layout(int N, int S, int M, int L, int Lq, int P)
{
    Workspace ws;
    ws.words = (size_t)N * M * S;
    ws.counts_bytes = (ws.words * 4 + 255) & ~(size_t)255;
    ws.slice = (size_t)Lq * L * P * 4;
    ws.total_bytes = 2 * ws.counts_bytes + (size_t)N * M * ws.slice * sizeof(Entry);
    return ws;
}

__global__ __launch_bounds__(256) void exact_clear(uint4 *__restrict__ p, int64_t n16)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// the sample of a thread: t = (((n * Lq + q) * M + m) * L + l) * P + p.  rows[k] = the corner's row inside the pyramid (or -1),
// w[k] = fl(a * c_k).  Returns false when the thread has no sample or the sample is skipped.
__device__ __forceinline__ bool sample_entries(int64_t t, int64_t total, const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                               const float *__restrict__ loc, const float *__restrict__ attn, int S, int M, int L, int P,
                                               bool want_w, int (&rows)[4], float (&w)[4], unsigned &grow, int &m)
{
    if (t >= total) return false;
    const int l = (int)((t / P) % L);
    grow = (unsigned)(t / ((int64_t)L * P));
    m = (int)(grow % (unsigned)M);
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)starts[l];
    const float2 xy = *reinterpret_cast<const float2 *>(loc + 2 * t);
    float lw, lh;
    if (!sample_setup(xy.x, xy.y, H, W, st, 1, rows, lw, lh)) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((unsigned)rows[k] >= (unsigned)S) rows[k] = -1;      // a level table that does not fit spatial_size writes nothing
    if (want_w) {
        const float a = attn[t];
        const float hh = sub_rn(1.f, lh), hw = sub_rn(1.f, lw);
        w[0] = mul_rn(a, mul_rn(hh, hw));
        w[1] = mul_rn(a, mul_rn(hh, lw));
        w[2] = mul_rn(a, mul_rn(lh, hw));
        w[3] = mul_rn(a, mul_rn(lh, lw));
    }
    return true;
}

__global__ __launch_bounds__(256) void exact_count(const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                   const float *__restrict__ loc, int S, int M, int L, int Lq, int P, int64_t total,
                                                   unsigned *__restrict__ count)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int rows[4], m;
    float w[4];
    unsigned grow;
    if (!sample_entries(t, total, shapes, starts, loc, nullptr, S, M, L, P, false, rows, w, grow, m)) return;
    const int64_t nm = (int64_t)(grow / ((unsigned)Lq * (unsigned)M)) * M + m;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (rows[k] >= 0) atomicAdd(count + nm * S + rows[k], 1u);
}

// one workgroup per (n, m): start = exclusive prefix of count, count = 0 (it is the fill's cursor from here on)
__global__ __launch_bounds__(kScanThreads) void exact_scan(unsigned *__restrict__ count, unsigned *__restrict__ start, int S)
{
    __shared__ unsigned part[kScanThreads];
    unsigned *c = count + (int64_t)blockIdx.x * S, *s = start + (int64_t)blockIdx.x * S;
    const int tid = threadIdx.x;
    const int per = (S + kScanThreads - 1) / kScanThreads;
    const int lo = min(tid * per, S), hi = min(lo + per, S);
    unsigned sum = 0;
    for (int i = lo; i < hi; ++i) sum += c[i];
    part[tid] = sum;
    __syncthreads();
    // inclusive scan of the 256 partial sums (Hillis-Steele)
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const unsigned v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned run = part[tid] - sum;
    for (int i = lo; i < hi; ++i) {
        const unsigned v = c[i];
        s[i] = run;
        c[i] = 0u;
        run += v;
    }
}

__global__ __launch_bounds__(256) void exact_fill(const int64_t *__restrict__ shapes, const int64_t *__restrict__ starts,
                                                  const float *__restrict__ loc, const float *__restrict__ attn, int S, int M, int L, int Lq,
                                                  int P, int64_t total, const unsigned *__restrict__ start, unsigned *__restrict__ cursor,
                                                  Entry *__restrict__ entries, unsigned slice)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int rows[4], m;
    float w[4];
    unsigned grow;
    if (!sample_entries(t, total, shapes, starts, loc, attn, S, M, L, P, true, rows, w, grow, m)) return;
    const int64_t nm = (int64_t)(grow / ((unsigned)Lq * (unsigned)M)) * M + m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (rows[k] < 0) continue;
        const unsigned slot = start[nm * S + rows[k]] + atomicAdd(cursor + nm * S + rows[k], 1u);
        if (slot < slice) entries[nm * (int64_t)slice + slot] = Entry{grow, w[k]};      // (always: the count saw the same corners)
    }
}

__device__ __forceinline__ void reduce_range(ExactSum &acc, const Entry *__restrict__ e, unsigned lo, unsigned hi, unsigned step,
                                             const float *__restrict__ gout, int lane)
{
    for (unsigned i = lo; i < hi; i += step) {
        const Entry en = e[i];
        acc.add(mul_rn(en.w, gout[(int64_t)en.grow * kChannels + lane]));
    }
}

// grid: N * M * ceil(S / kReduceGroups) workgroups; workgroup b owns rows r0 .. r0 + 7 of its (n, m), lane group g row r0 + g
__global__ __launch_bounds__(kReduceThreads) void exact_reduce(const float *__restrict__ gout, const unsigned *__restrict__ start,
                                                               const unsigned *__restrict__ len, const Entry *__restrict__ entries,
                                                               unsigned slice, int S, int M, int tiles, float *__restrict__ gvalue)
{
    __shared__ uint64_t sh_w[5][kReduceGroups][kChannels];
    __shared__ unsigned sh_f[kReduceGroups][kChannels];
    const int lane = threadIdx.x & (kChannels - 1), grp = threadIdx.x / kChannels;
    const int nm = (int)blockIdx.x / tiles, r0 = ((int)blockIdx.x % tiles) * kReduceGroups;
    const int n = nm / M, m = nm - n * M;
    const unsigned *st = start + (int64_t)nm * S, *ln = len + (int64_t)nm * S;
    const Entry *e = entries + (int64_t)nm * slice;
    // short rows: one lane group each
    {
        const int row = r0 + grp;
        if (row < S) {
            const unsigned cnt = ln[row];
            if (cnt <= (unsigned)kSplitLen) {
                ExactSum acc;
                acc.clear();
                const unsigned s0 = st[row];
                reduce_range(acc, e, s0, s0 + cnt, 1u, gout, lane);
                gvalue[(((int64_t)n * S + row) * M + m) * kChannels + lane] = acc.round_to_float();
            }
        }
    }
    // long rows: all lane groups on one row, entries interleaved, partial accumulators merged through LDS
    for (int j = 0; j < kReduceGroups; ++j) {
        const int row = r0 + j;
        if (row >= S) break;                                     // (workgroup-uniform)
        const unsigned cnt = ln[row];
        if (cnt <= (unsigned)kSplitLen) continue;                // (workgroup-uniform)
        ExactSum acc;
        acc.clear();
        const unsigned s0 = st[row];
        reduce_range(acc, e, s0 + (unsigned)grp, s0 + cnt, (unsigned)kReduceGroups, gout, lane);
        __syncthreads();                                         // (the previous long row's merge has read the LDS)
        sh_w[0][grp][lane] = acc.w[0];
        sh_w[1][grp][lane] = acc.w[1];
        sh_w[2][grp][lane] = acc.w[2];
        sh_w[3][grp][lane] = acc.w[3];
        sh_w[4][grp][lane] = acc.w[4];
        sh_f[grp][lane] = acc.flags;
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int g = 1; g < kReduceGroups; ++g) {
                ExactSum o;
                o.w[0] = sh_w[0][g][lane];
                o.w[1] = sh_w[1][g][lane];
                o.w[2] = sh_w[2][g][lane];
                o.w[3] = sh_w[3][g][lane];
                o.w[4] = sh_w[4][g][lane];
                o.flags = sh_f[g][lane];
                acc.merge(o);
            }
            gvalue[(((int64_t)n * S + row) * M + m) * kChannels + lane] = acc.round_to_float();
        }
    }
}

}  // namespace semidetr_exact

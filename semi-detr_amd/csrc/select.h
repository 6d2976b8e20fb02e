// Selection primitives shared by nms.hip, query_select.hip and detect.hip: "the k largest of n, ties by the
// lower index, sorted".  Device side only; every function is called by ALL threads of a workgroup of NT threads (NT a
// multiple of 64) under uniform control flow.  The kernels keep their own control flow and LDS; they hand the arrays in.
#pragma once
#include <hip/hip_runtime.h>

namespace semidetr {

// One rounded operation each: negate, expf, add, IEEE correctly rounded quotient (v_div_scale / v_div_fmas / v_div_fixup, the
// same sequence as a plain `1.0f / y`).  nms.hip includes this header behind its `#pragma clang fp contract(off)`, so that
// the sum is not contracted into expf's last operation there.
__device__ __forceinline__ float sigmoidf_(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

// The integer that orders like the float: NaN (either sign) above +inf, -0 == +0.
// (NMS once ordered a negative NaN below -inf instead.  Its results cannot tell: a candidate gets a key only behind
// `sigmoidf_(x) > score_thr`, which is false for a NaN, so no NaN is ever keyed there.)
__device__ __forceinline__ unsigned order_key(float v)
{
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.f) v = 0.f;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- 8-bit radix select, most significant byte first.  `prefix` / `mask` describe the words still tied with the wanted one.
// hist holds COPIES histograms of 256 bins at a stride of 257 ints: a thread counts into copy (tid % COPIES), and the odd
// stride puts one digit's copies into different LDS banks, so equal digits do not serialise on one address.
constexpr int kHistStride = 257;

// Clear hist, then count byte `pass` of the words among words[0 .. n) that match (prefix, mask).  `words` is an LDS array or
// a global pointer.  The counts are visible on return; the caller's writes to `words` must be behind a barrier already.
template <int NT, int COPIES, typename W>
__device__ __forceinline__ void histogram_pass(int *hist, const W *words, int n, W prefix, W mask, int pass)
{
    static_assert(COPIES <= 64 && (COPIES & (COPIES - 1)) == 0, "a power of two of at most one copy per lane");
    const int tid = threadIdx.x;
    for (int i = tid; i < COPIES * kHistStride; i += NT) hist[i] = 0;
    __syncthreads();
    int *mine = hist + (tid & (COPIES - 1)) * kHistStride;
    for (int i = tid; i < n; i += NT) {
        const W u = words[i];
        if ((u & mask) == prefix) atomicAdd(&mine[(int)((u >> (8 * pass)) & 255)], 1);
    }
    __syncthreads();
}

// hist -> *s_digit, the digit that holds the *s_remaining-th largest matching word; *s_remaining becomes its rank inside that
// digit and *s_matching (where given) the digit's population.  Thread d < 256 owns bin d: it sums the bin's copies, a suffix
// sum over the wavefront's lanes plus the totals of the higher wavefronts (through bins[0 .. 3]) gives the words above the
// bin, and the one thread whose bin the rank falls into publishes; visible on return.  (One thread walking down the bins
// with an early exit pays an LDS round trip per bin, ~10 us per pass; 256 threads that each read all the bins above their
// own made nms_topk_kernel 3 us slower than the walk.)
// `bins` is scratch of at least 4 ints; the callers hand in 256-int arrays, which keeps their static LDS at its recorded size.
// PRECONDITION: 1 <= *s_remaining <= number of words counted.  Otherwise no thread publishes and the old digit stays.
template <int NT, int COPIES>
__device__ __forceinline__ void pick_digit(const int *hist, int *bins, int *s_digit, int *s_remaining, int *s_matching = nullptr)
{
    static_assert(NT >= 256 && NT % 64 == 0, "thread d owns bin d: four whole wavefronts at least");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int v = 0, above = 0;
    if (tid < 256) {
        for (int cp = 0; cp < COPIES; ++cp) v += hist[cp * kHistStride + tid];
        int s = v;                                                     // -> sum over the lanes >= mine
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_down(s, d, 64);
            if (lane + d < 64) s += t;
        }
        above = s - v;
        if (lane == 0) bins[wave] = s;
    }
    __syncthreads();
    const int rem = *s_remaining;
    bool mine = false;
    if (tid < 256) {
        for (int w = wave + 1; w < 4; ++w) above += bins[w];
        mine = above < rem && rem <= above + v;
    }
    __syncthreads();                                                   // every thread has read s_remaining
    if (mine) {
        *s_digit = tid;
        *s_remaining = rem - above;
        if (s_matching) *s_matching = v;
    }
    __syncthreads();
}

// The tie rule.  Calls store(i, keys[i]) for every i < n whose key is above `kth`, and for the first `ties` positions, in
// index order, whose key equals it (ballot inside a wavefront, prefix over the wavefronts through s_wave[NT / 64], running
// total in *s_base).  *s_base must be 0 and visible on entry; the order of the store calls is unspecified.
template <int NT, typename Store>
__device__ __forceinline__ void collect_with_ties(const unsigned *keys, int n, unsigned kth, int ties, int *s_wave, int *s_base,
                                                  Store store)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i0 = 0; i0 < n; i0 += NT) {
        const int i = i0 + tid;
        const unsigned u = i < n ? keys[i] : 0u;
        const bool above = i < n && u > kth, tie = i < n && u == kth;
        const unsigned long long ballot = __ballot(tie);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = *s_base;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        const int rank = before + __popcll(ballot & ((1ull << lane) - 1ull));
        if (above || (tie && rank < ties)) store(i, u);
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < NT / 64; ++w) t += s_wave[w];
            *s_base += t;
        }
        // (s_base / s_wave are rewritten only behind the next iteration's first barrier or read behind it)
        __syncthreads();
    }
}

// Bitonic sort, descending, of the n (a power of two >= 2) 64-bit words in LDS.  Barrier convention: a barrier BEFORE every
// step and one after the last.  So the caller's writes to `words` need no barrier of their own before the call, and the
// sorted words are visible to every thread on return.
template <int NT>
__device__ __forceinline__ void bitonic_desc(unsigned long long *words, int n)
{
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (n >> 1); t += NT) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;      // lo has bit `stride` clear
                const bool desc = (lo & size) == 0;
                const unsigned long long a = words[lo], c = words[hi];
                if ((a < c) == desc) { words[lo] = c; words[hi] = a; }
            }
        }
    }
    __syncthreads();
}

}  // namespace semidetr

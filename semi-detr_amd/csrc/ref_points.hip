// Reference-point chain of the decoder for gfx950: what DINOTransformerDecoder.forward does to the reference points between two
// layers (detr_od/models/utils/transformer.py:972-987, 1029-1036) -- sigmoid / box refinement through inverse_sigmoid (:435-451),
// the valid-ratio scaling, gen_sineembed_for_position (:467-493) -- and the head's coordinate loop
// (dino_detr_ssod_head.py:393-398), forward and backward.  One parameter block with a table of row segments (semidetr_ref_points)
// serves every launch; a launch covers all segments.
//
//   ref_points_fwd_kernel<W>  workgroup = one wave = kRows = 8 consecutive rows of a segment.  Lane (row r = lane / W, coordinate
//                             c = lane % W) reads delta and ref in their type, refines, rounds once to out_type, stores new_ref,
//                             multiplies the rounded value by the image's valid ratios and stores its element of every level of
//                             ref_input.  Then the wave walks its rows: the level-0 coordinates come over __shfl, and each lane
//                             writes 16 bytes of each 128-column block pair (columns 4 * lane and 256 + 4 * lane) of the embed row;
//                             the lane's four dim_t entries stay in registers over the rows.
//   ref_points_bwd_kernel<W>  the same map.  The wave walks its rows first: each lane forms its four terms per block, adds them in
//                             index order, a xor butterfly (16 .. 1) adds the 32 lanes of a block, and the row's lanes pick the
//                             sums of their coordinates.  Then lane (r, c) adds the levels' g_ref_input * vr in level order and
//                             applies the refine derivative.
// No LDS, no scratch, no float atomics, no memset, no workspace; the grid and every order depend on the row counts alone: two runs
// are bitwise equal.
//
// Arithmetic (tests/ref_points_ref64.py bounds it), every operation rounded on its own (contraction off), precise sinf / cosf /
// expf / logf and correctly rounded division:
//   sigmoid(t) = 1 / (1 + expf(-t));  inverse_sigmoid(x) = logf(max(clamp(x, 0, 1), eps) / max(1 - clamp(x, 0, 1), eps));
//   arg = (coord * fp32(2 pi)) / dim_t[t];  backward term = (g * cosf(arg)) / dim_t[t]  or  (g * -sinf(arg)) / dim_t[t].
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"

constexpr int kMaxSegments = SEMIDETR_REF_MAX_SEGMENTS, kMaxLevels = SEMIDETR_REF_MAX_LEVELS;
constexpr int kRows = 8;                             // rows of a wave (= of a workgroup)
constexpr int kBlock = 128;                          // columns of one coordinate's block of the embed
constexpr float kTwoPi = 6.283185307179586f;         // fp32(2 * math.pi)

struct Plan {
    int first[kMaxSegments + 1];                     // first workgroup of a segment
};

__device__ __forceinline__ int segment_of(const int *first, int segments, int block)
{
    int s = 0;
    while (s + 1 < segments && block >= first[s + 1]) ++s;
    return s;
}

// ---- elements in their type (SEMIDETR_ROW_*): the branch is one scalar branch of the whole wave --------------------------------
__device__ __forceinline__ float ld1(const void *base, int type, int64_t i)
{
    if (type == SEMIDETR_ROW_F32) return static_cast<const float *>(base)[i];
    const unsigned bits = static_cast<const unsigned short *>(base)[i];
    return type == SEMIDETR_ROW_FP16 ? Cvt<__half>::up(bits) : Cvt<__hip_bfloat16>::up(bits);
}

__device__ __forceinline__ void st1(void *base, int type, int64_t i, float v)
{
    if (type == SEMIDETR_ROW_F32) static_cast<float *>(base)[i] = v;
    else static_cast<unsigned short *>(base)[i] =
        (unsigned short)(type == SEMIDETR_ROW_FP16 ? Cvt<__half>::down(v) : Cvt<__hip_bfloat16>::down(v));
}

// v as an element of `type` holds it
__device__ __forceinline__ float rounded(float v, int type)
{
    if (type == SEMIDETR_ROW_F32) return v;
    return type == SEMIDETR_ROW_FP16 ? Cvt<__half>::up(Cvt<__half>::down(v)) : Cvt<__hip_bfloat16>::up(Cvt<__hip_bfloat16>::down(v));
}

// ---- the arithmetic: the only statements of it ---------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid1(float t)
{
    #pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-t));
}

// comparisons, not fminf / fmaxf: a NaN stays a NaN, as torch's clamp keeps it
__device__ __forceinline__ float inverse_sigmoid1(float x, float eps)
{
    #pragma clang fp contract(off)
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    const float om = 1.0f - x;
    const float x1 = x < eps ? eps : x, x2 = om < eps ? eps : om;
    return logf(x1 / x2);
}

// d inverse_sigmoid / d x with torch's clamp rule: the gradient passes where min <= x <= max, equality included
__device__ __forceinline__ float inverse_sigmoid_slope(float x, float eps)
{
    #pragma clang fp contract(off)
    if (!(x >= 0.0f && x <= 1.0f)) return 0.0f;
    const float om = 1.0f - x;
    float t = 0.0f;
    if (x >= eps) t = 1.0f / x;
    if (om >= eps) t += 1.0f / om;
    return t;
}

__device__ __forceinline__ float sigmoid_grad(float g, float y)
{
    #pragma clang fp contract(off)
    return (g * (1.0f - y)) * y;
}

__device__ __forceinline__ float4 embed4(float coord, const float4 &d)
{
    #pragma clang fp contract(off)
    const float m = coord * kTwoPi;
    return make_float4(sinf(m / d.x), cosf(m / d.y), sinf(m / d.z), cosf(m / d.w));
}

// the lane's four terms of d embed / d coord (without the factor 2 pi), added in index order
__device__ __forceinline__ float embed_grad4(float coord, const float4 &d, const float4 &g)
{
    #pragma clang fp contract(off)
    const float m = coord * kTwoPi;
    const float t0 = (g.x * cosf(m / d.x)) / d.x, t1 = (g.y * -sinf(m / d.y)) / d.y;
    const float t2 = (g.z * cosf(m / d.z)) / d.z, t3 = (g.w * -sinf(m / d.w)) / d.w;
    return ((t0 + t1) + t2) + t3;
}

// the 32 lanes of a half wave, fixed order; every lane of the half gets the same bits
__device__ __forceinline__ float half_wave_sum(float v)
{
    #pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// lanes 0 .. 31 write the blocks of (y, w) = coordinates (1, 2), lanes 32 .. 63 those of (x, h) = coordinates (0, 3)
__device__ __forceinline__ int first_coord(int lane) { return lane < 32 ? 1 : 0; }
__device__ __forceinline__ int second_coord(int lane) { return lane < 32 ? 2 : 3; }

template <int W>
__global__ __launch_bounds__(64) void ref_points_fwd_kernel(const semidetr_ref_points p, const Plan pl)
{
    const int lane = threadIdx.x;
    const int s = segment_of(pl.first, p.num_segments, blockIdx.x);
    const semidetr_ref_segment &sg = p.segment[s];
    const int total = sg.rows0 * sg.rows1, row0 = (blockIdx.x - pl.first[s]) * kRows;
    const int r = lane / W, c = lane % W, row = row0 + r;
    const bool active = r < kRows && row < total;
    const int i = active ? row / sg.rows1 : 0, j = active ? row - i * sg.rows1 : 0;
    float y = 0.0f;
    if (active) {
        const float x = ld1(sg.ref, p.ref_type, i * sg.ref_stride[0] + j * sg.ref_stride[1] + c);
        if (p.mode == SEMIDETR_REF_NONE) {
            y = x;
        } else if (p.mode == SEMIDETR_REF_SIGMOID) {
            y = rounded(sigmoid1(x), p.out_type);
        } else {
            const float d = ld1(sg.delta, p.delta_type, i * sg.delta_stride[0] + j * sg.delta_stride[1] + c);
            y = rounded(sigmoid1(d + inverse_sigmoid1(x, p.eps)), p.out_type);
        }
        if (sg.new_ref) st1(sg.new_ref, p.out_type, i * sg.new_ref_stride[0] + j * sg.new_ref_stride[1] + c, y);
    }
    if (!p.valid_ratios) return;                     // the same for the whole launch
    float coord = 0.0f;                              // the level-0 element of ref_input
    if (active) {
        const float *vr = p.valid_ratios + (int64_t)j * p.levels * 2 + (c & 1);
        float *out = p.ref_input + ((int64_t)j * sg.rows0 + i) * p.levels * W + c;
        for (int l = 0; l < p.levels; ++l) {
            const float v = y * vr[2 * l];
            out[l * W] = v;
            if (l == 0) coord = v;
        }
    }
    if (!p.embed) return;
    const float4 d = *reinterpret_cast<const float4 *>(p.dim_t + ((4 * lane) & (kBlock - 1)));
    const int rows = min(kRows, total - row0);
    float *erow = p.embed + (int64_t)row0 * kBlock * W + 4 * lane;
    for (int rr = 0; rr < rows; ++rr, erow += kBlock * W) {
        const float a = __shfl(coord, rr * W + first_coord(lane));
        *reinterpret_cast<float4 *>(erow) = embed4(a, d);
        if (W == 4) {
            const float b = __shfl(coord, rr * W + second_coord(lane));
            *reinterpret_cast<float4 *>(erow + 2 * kBlock) = embed4(b, d);
        }
    }
}

template <int W>
__global__ __launch_bounds__(64) void ref_points_bwd_kernel(const semidetr_ref_points p, const Plan pl)
{
    const int lane = threadIdx.x;
    const int s = segment_of(pl.first, p.num_segments, blockIdx.x);
    const semidetr_ref_segment &sg = p.segment[s];
    const int total = sg.rows0 * sg.rows1, row0 = (blockIdx.x - pl.first[s]) * kRows;
    const int r = lane / W, c = lane % W, row = row0 + r;
    const bool active = r < kRows && row < total;
    const int i = active ? row / sg.rows1 : 0, j = active ? row - i * sg.rows1 : 0;
    float x = 0.0f, y = 0.0f;
    if (active) {
        x = ld1(sg.ref, p.ref_type, i * sg.ref_stride[0] + j * sg.ref_stride[1] + c);
        y = p.mode == SEMIDETR_REF_NONE ? x : ld1(sg.new_ref, p.out_type, i * sg.new_ref_stride[0] + j * sg.new_ref_stride[1] + c);
    }
    float g = 0.0f;
    bool have = false;                               // g holds a term: the first one is taken, not added to a zero
    if (active && sg.g_new) {
        g = ld1(sg.g_new, p.out_type, i * sg.g_new_stride[0] + j * sg.g_new_stride[1] + c);
        have = true;
    }
    if (p.valid_ratios) {                            // the same for the whole launch
        const float *vr = p.valid_ratios + (int64_t)j * p.levels * 2 + (c & 1);
        if (active && p.g_ref_input) {
            #pragma clang fp contract(off)
            const float *gin = p.g_ref_input + ((int64_t)j * sg.rows0 + i) * p.levels * W + c;
            for (int l = 0; l < p.levels; ++l) {
                const float t = gin[l * W] * vr[2 * l];
                g = have ? g + t : t;
                have = true;
            }
        }
        if (p.g_embed) {
            #pragma clang fp contract(off)
            const float coord = active ? y * vr[0] : 0.0f;
            const float4 d = *reinterpret_cast<const float4 *>(p.dim_t + ((4 * lane) & (kBlock - 1)));
            const int rows = min(kRows, total - row0);
            const float *grow = p.g_embed + (int64_t)row0 * kBlock * W + 4 * lane;
            float mine = 0.0f;
            for (int rr = 0; rr < rows; ++rr, grow += kBlock * W) {
                const float a = __shfl(coord, rr * W + first_coord(lane));
                const float sa = half_wave_sum(embed_grad4(a, d, *reinterpret_cast<const float4 *>(grow)));
                const float of_y = __shfl(sa, 0), of_x = __shfl(sa, 32);
                float of_w = 0.0f, of_h = 0.0f;
                if (W == 4) {
                    const float b = __shfl(coord, rr * W + second_coord(lane));
                    const float sb = half_wave_sum(embed_grad4(b, d, *reinterpret_cast<const float4 *>(grow + 2 * kBlock)));
                    of_w = __shfl(sb, 0);
                    of_h = __shfl(sb, 32);
                }
                if (r == rr) mine = c == 0 ? of_x : (c == 1 ? of_y : (c == 2 ? of_w : of_h));
            }
            if (active) {
                const float t = (mine * kTwoPi) * vr[0];
                g = have ? g + t : t;
                have = true;
            }
        }
    }
    if (!active) return;
    const int64_t at = (int64_t)row * W + c;
    if (p.mode == SEMIDETR_REF_NONE) {
        if (sg.g_ref) st1(sg.g_ref, p.ref_type, at, g);
    } else if (p.mode == SEMIDETR_REF_SIGMOID) {
        if (sg.g_ref) st1(sg.g_ref, p.ref_type, at, sigmoid_grad(g, y));
    } else {
        #pragma clang fp contract(off)
        const float gd = sigmoid_grad(g, y);
        if (sg.g_delta) st1(sg.g_delta, p.delta_type, at, gd);
        if (sg.g_ref) st1(sg.g_ref, p.ref_type, at, gd * inverse_sigmoid_slope(x, p.eps));
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
bool known_type(int type) { return type == SEMIDETR_ROW_F32 || type == SEMIDETR_ROW_FP16 || type == SEMIDETR_ROW_BF16; }
bool aligned(const void *ptr, int type) { return ((uintptr_t)ptr & (type == SEMIDETR_ROW_F32 ? 3 : 1)) == 0; }
bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

int rows_check(const char *what, int s, const void *ptr, int type, const int64_t *stride)
{
    SEMIDETR_REQUIRE(ptr, SEMIDETR_E_BADARG, "ref_points: null pointer (%s of segment %d)", what, s);
    SEMIDETR_REQUIRE(aligned(ptr, type) && stride[0] >= 0 && stride[1] >= 0, SEMIDETR_E_BADARG,
                     "ref_points: %s of segment %d must be aligned to its element, with non-negative strides", what, s);
    return SEMIDETR_OK;
}

// Host-side check of the parameter block and the grid.
int plan(const semidetr_ref_points *params, int for_backward, Plan &pl)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "ref_points: null pointer (parameter block)");
    const semidetr_ref_points &p = params[0];
    SEMIDETR_REQUIRE(p.width == 2 || p.width == 4, SEMIDETR_E_BADARG, "ref_points: width %d (2 and 4 are built)", p.width);
    SEMIDETR_REQUIRE(p.mode == SEMIDETR_REF_NONE || p.mode == SEMIDETR_REF_SIGMOID || p.mode == SEMIDETR_REF_REFINE, SEMIDETR_E_BADARG,
                     "ref_points: unknown mode %d (SEMIDETR_REF_NONE / _SIGMOID / _REFINE)", p.mode);
    SEMIDETR_REQUIRE(p.num_segments >= 1 && p.num_segments <= kMaxSegments, SEMIDETR_E_BADARG,
                     "ref_points: %d segments (1 .. %d)", p.num_segments, kMaxSegments);
    SEMIDETR_REQUIRE(p.eps >= 0.0f, SEMIDETR_E_BADARG, "ref_points: eps is NaN or negative");
    const bool refine = p.mode == SEMIDETR_REF_REFINE;
    SEMIDETR_REQUIRE(known_type(p.ref_type) && known_type(p.out_type) && (!refine || known_type(p.delta_type)), SEMIDETR_E_BADARG,
                     "ref_points: unknown type code (delta_type=%d ref_type=%d out_type=%d; SEMIDETR_ROW_F32 / _FP16 / _BF16)",
                     p.delta_type, p.ref_type, p.out_type);
    const int promoted = !refine || p.delta_type == p.ref_type ? p.ref_type : SEMIDETR_ROW_F32;
    SEMIDETR_REQUIRE(p.out_type == promoted || (p.out_type == SEMIDETR_ROW_F32 && p.mode != SEMIDETR_REF_NONE), SEMIDETR_E_BADARG,
                     "ref_points: out_type %d is neither fp32 nor the operands' common type %d", p.out_type, promoted);
    if (p.valid_ratios) {
        SEMIDETR_REQUIRE(p.num_segments == 1, SEMIDETR_E_BADARG, "ref_points: scale and embed take one segment, not %d", p.num_segments);
        SEMIDETR_REQUIRE(p.levels >= 1 && p.levels <= kMaxLevels, SEMIDETR_E_BADARG, "ref_points: %d levels (1 .. %d)", p.levels, kMaxLevels);
        SEMIDETR_REQUIRE(aligned(p.valid_ratios, SEMIDETR_ROW_F32), SEMIDETR_E_BADARG, "ref_points: valid_ratios misaligned");
        if (!for_backward) {
            SEMIDETR_REQUIRE(p.ref_input && aligned(p.ref_input, SEMIDETR_ROW_F32), SEMIDETR_E_BADARG,
                             "ref_points forward: ref_input null or misaligned");
            SEMIDETR_REQUIRE(!p.embed || (aligned16(p.embed) && p.dim_t && aligned16(p.dim_t)), SEMIDETR_E_BADARG,
                             "ref_points forward: embed needs dim_t, both 16-byte aligned");
        } else {
            SEMIDETR_REQUIRE(!p.g_ref_input || aligned(p.g_ref_input, SEMIDETR_ROW_F32), SEMIDETR_E_BADARG,
                             "ref_points backward: g_ref_input misaligned");
            SEMIDETR_REQUIRE(!p.g_embed || (aligned16(p.g_embed) && p.dim_t && aligned16(p.dim_t)), SEMIDETR_E_BADARG,
                             "ref_points backward: g_embed needs dim_t, both 16-byte aligned");
        }
    } else {
        SEMIDETR_REQUIRE(p.levels == 0 && !p.embed && !p.ref_input && !p.g_embed && !p.g_ref_input, SEMIDETR_E_BADARG,
                         "ref_points: levels, ref_input, embed and their gradients need valid_ratios");
    }
    pl.first[0] = 0;
    for (int s = 0; s < kMaxSegments; ++s) {
        int groups = 0;
        if (s < p.num_segments) {
            const semidetr_ref_segment &sg = p.segment[s];
            SEMIDETR_REQUIRE(sg.rows0 >= 1 && sg.rows1 >= 1, SEMIDETR_E_BADARG,
                             "ref_points: bad sizes (segment %d: rows0=%d rows1=%d)", s, sg.rows0, sg.rows1);
            const int64_t total = (int64_t)sg.rows0 * sg.rows1;
            SEMIDETR_REQUIRE(total * kBlock * p.width < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE,
                             "ref_points: too large (segment %d: rows0 * rows1 * 128 * width < 2^31)", s);
            if (int rc = rows_check("ref", s, sg.ref, p.ref_type, sg.ref_stride)) return rc;
            if (refine) if (int rc = rows_check("delta", s, sg.delta, p.delta_type, sg.delta_stride)) return rc;
            if (for_backward ? p.mode != SEMIDETR_REF_NONE : (sg.new_ref || p.mode != SEMIDETR_REF_NONE || !p.valid_ratios))
                if (int rc = rows_check("new_ref", s, sg.new_ref, p.out_type, sg.new_ref_stride)) return rc;
            if (for_backward) {
                if (sg.g_new) if (int rc = rows_check("g_new", s, sg.g_new, p.out_type, sg.g_new_stride)) return rc;
                SEMIDETR_REQUIRE(sg.g_new || p.g_ref_input || p.g_embed, SEMIDETR_E_BADARG,
                                 "ref_points backward: null pointer (no upstream gradient for segment %d)", s);
                SEMIDETR_REQUIRE(sg.g_ref || (refine && sg.g_delta), SEMIDETR_E_BADARG,
                                 "ref_points backward: null pointer (no gradient wanted from segment %d)", s);
                SEMIDETR_REQUIRE((!sg.g_ref || aligned(sg.g_ref, p.ref_type)) && (!refine || !sg.g_delta || aligned(sg.g_delta, p.delta_type)),
                                 SEMIDETR_E_BADARG, "ref_points backward: g_ref or g_delta of segment %d misaligned", s);
            }
            groups = (int)((total + kRows - 1) / kRows);
        }
        SEMIDETR_REQUIRE((int64_t)pl.first[s] + groups < ((int64_t)1 << 31), SEMIDETR_E_TOOLARGE, "ref_points: too many rows in all");
        pl.first[s + 1] = pl.first[s] + groups;
    }
    return SEMIDETR_OK;
}

}  // namespace

extern "C" int semidetr_ref_points_forward(void *stream, const semidetr_ref_points *params)
{
    Plan pl;
    if (int rc = plan(params, 0, pl)) return rc;
    const semidetr_ref_points &p = params[0];
    hipStream_t st = semidetr::as_stream(stream);
    if (p.width == 4) hipLaunchKernelGGL(ref_points_fwd_kernel<4>, dim3(pl.first[p.num_segments]), dim3(64), 0, st, p, pl);
    else hipLaunchKernelGGL(ref_points_fwd_kernel<2>, dim3(pl.first[p.num_segments]), dim3(64), 0, st, p, pl);
    return semidetr::launch_status("ref_points_fwd_kernel");
}

extern "C" int semidetr_ref_points_backward(void *stream, const semidetr_ref_points *params)
{
    Plan pl;
    if (int rc = plan(params, 1, pl)) return rc;
    const semidetr_ref_points &p = params[0];
    hipStream_t st = semidetr::as_stream(stream);
    if (p.width == 4) hipLaunchKernelGGL(ref_points_bwd_kernel<4>, dim3(pl.first[p.num_segments]), dim3(64), 0, st, p, pl);
    else hipLaunchKernelGGL(ref_points_bwd_kernel<2>, dim3(pl.first[p.num_segments]), dim3(64), 0, st, p, pl);
    return semidetr::launch_status("ref_points_bwd_kernel");
}

// Pyramid inputs of the transformer for gfx950: the level masks (from the image sizes, by F.interpolate's nearest rule, or given),
// SinePositionalEncodingHW of every level (detr_od/models/utils/positional_encoding.py:57-99) with the level_embed row added,
// flattened and concatenated into complete (N, S, 256) token rows (transformer.py:1271-1289), mask_flatten, get_valid_ratio
// (:1237-1244, 1292) and the encoder's get_reference_points (:676-691); backward: the gradient of level_embed.  One parameter block
// with a level table and the image sizes by value (semidetr_pyramid_inputs) serves every launch; a launch covers the whole pyramid
// and batch.
//
//   pyramid_scan_kernel      workgroup = one wave = 64 columns (or 64 rows) of an (image, level).  A lane walks its column down
//                            (its row along): evaluates or reads the mask, writes the mask byte (column walk only) and the
//                            inclusive count of valid pixels so far as 16 bits into the workspace (cnt_y | cnt_x, each N * S).
//                            The lane of column 0 / row 0 writes the valid ratio from its total.
//   pyramid_emit_kernel      workgroup = 4 waves = kTile = 32 consecutive token rows of an (image, level).  Lane k of a wave holds
//                            channels 4k .. 4k + 3: lanes 0 .. 31 the y half, 32 .. 63 the x half, the lane's four divisors and
//                            four level_embed values in registers.  Per row: the pixel's count and its column's (row's) total --
//                            the count at the last row (column) -- come from the workspace, the wave stores the whole 1 KB row
//                            (16 bytes per lane; 8 for 16-bit rows), lanes 0 .. 2 L - 1 the row's reference points.
//   pyramid_grad_rows_kernel workgroup = kUnit = 256 rows of an (image, level): wave v adds rows v, v + 4, ... in that order, the
//                            four waves combine through LDS in wave order into one slot of 256 floats.
//   pyramid_grad_sum_kernel  workgroup = level: 4 parts x 256 channels add the level's slots in slot order in fp64, the parts in
//                            part order, one rounding.
// No float atomics, no memset; every grid, map and order depends on batch, levels, h[] and w[] alone: two runs are bitwise equal.
//
// Arithmetic (tests/pyramid_inputs_ref64.py bounds it), every operation rounded on its own (contraction off), precise sinf / cosf
// and correctly rounded division:
//   y = ((cnt_y + offset) / (tot_y + eps)) * scale  (normalize), else cnt_y;  pos[c] = sinf | cosf (y / dim_ty[c]) + level_embed[l][c];
//   vr = ((float)tot_x(row 0) * (1.0f / w), (float)tot_y(column 0) * (1.0f / h)): what torch's division of a GPU tensor by a host
//   number computes;  ref = ((j + 0.5f) / (vr[l].x * w)) * vr[l'].x, likewise y.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"

namespace {

#include "cvt16.h"

constexpr int kC = 256, kBlock = 128;                // channels of a token row; channels of one coordinate's half
constexpr int kMaxLevels = SEMIDETR_PYR_MAX_LEVELS, kMaxBatch = SEMIDETR_PYR_MAX_BATCH;
constexpr int kWaves = 4, kThreads = 64 * kWaves;
constexpr int kTile = 32;                            // token rows of an emit workgroup
constexpr int kUnit = 256;                           // token rows of one backward slot
constexpr int kParts = 4;

// The grids: level-major, then image, then the part of the level.
struct Plan {
    int sfirst[kMaxLevels + 1], cchunks[kMaxLevels], rchunks[kMaxLevels];   // scan: 64-column chunks, then 64-row chunks
    int tfirst[kMaxLevels + 1], tiles[kMaxLevels];                          // emit tiles per image
    int ufirst[kMaxLevels + 1], units[kMaxLevels];                          // backward units (= slots) per image
};

__device__ __forceinline__ int level_of(const int *first, int levels, int block)
{
    int l = 0;
    while (l + 1 < levels && block >= first[l + 1]) ++l;
    return l;
}

// ---- elements in their type (SEMIDETR_ROW_*): the branch is one scalar branch of the whole wave --------------------------------
__device__ __forceinline__ float4 ld4(const void *base, int type, int64_t i)
{
    if (type == SEMIDETR_ROW_F32) return *reinterpret_cast<const float4 *>(static_cast<const float *>(base) + i);
    const float2 r = *reinterpret_cast<const float2 *>(static_cast<const unsigned short *>(base) + i);
    return type == SEMIDETR_ROW_FP16 ? unpack4<__half>(r) : unpack4<__hip_bfloat16>(r);
}

__device__ __forceinline__ void st4(void *base, int type, int64_t i, const float4 &v)
{
    if (type == SEMIDETR_ROW_F32) {
        *reinterpret_cast<float4 *>(static_cast<float *>(base) + i) = v;
        return;
    }
    uint2 bits;
    if (type == SEMIDETR_ROW_FP16) bits = make_uint2(pack2<__half>(v.x, v.y), pack2<__half>(v.z, v.w));
    else bits = make_uint2(pack2<__hip_bfloat16>(v.x, v.y), pack2<__hip_bfloat16>(v.z, v.w));
    *reinterpret_cast<uint2 *>(static_cast<unsigned short *>(base) + i) = bits;
}

__device__ __forceinline__ void st1(void *base, int type, int64_t i, float v)
{
    if (type == SEMIDETR_ROW_F32) static_cast<float *>(base)[i] = v;
    else static_cast<unsigned short *>(base)[i] =
        (unsigned short)(type == SEMIDETR_ROW_FP16 ? Cvt<__half>::down(v) : Cvt<__hip_bfloat16>::down(v));
}

// ---- the arithmetic: the only statements of it ---------------------------------------------------------------------------------
// F.interpolate's nearest source index of destination index d; ratio = (float)in / (float)out
__device__ __forceinline__ int nearest_src(int d, float ratio, int in)
{
    return min((int)floorf((float)d * ratio), in - 1);
}

__device__ __forceinline__ float coordinate(const semidetr_pyramid_inputs &p, unsigned cnt, unsigned tot)
{
    #pragma clang fp contract(off)
    if (!p.normalize) return (float)cnt;
    return (((float)cnt + p.offset) / ((float)tot + p.eps)) * p.scale;
}

__device__ __forceinline__ float4 embed4(float v, const float4 &d)
{
    #pragma clang fp contract(off)
    return make_float4(sinf(v / d.x), cosf(v / d.y), sinf(v / d.z), cosf(v / d.w));
}

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// torch divides a GPU tensor by a host number by multiplying with the number's fp32 reciprocal; get_valid_ratio does exactly that
__device__ __forceinline__ float valid_ratio(unsigned valid, int size)
{
    #pragma clang fp contract(off)
    return (float)valid * (1.0f / (float)size);
}

__device__ __forceinline__ float ref_point(float index, float own_ratio, float size, float other_ratio)
{
    #pragma clang fp contract(off)
    return ((index + 0.5f) / (own_ratio * size)) * other_ratio;
}

// ---- 1. masks, counts, valid ratios ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void pyramid_scan_kernel(const semidetr_pyramid_inputs p, const Plan pl, unsigned short *counts)
{
    const int lane = threadIdx.x;
    const int l = level_of(pl.sfirst, p.levels, blockIdx.x);
    const int per = pl.cchunks[l] + pl.rchunks[l];
    const int r = blockIdx.x - pl.sfirst[l], n = r / per, k = r - n * per;
    const int h = p.h[l], w = p.w[l];
    const int64_t base = (int64_t)n * p.tokens_per_image + p.start[l];
    const unsigned char *given = p.from_sizes ? nullptr : static_cast<const unsigned char *>(p.masks[l]) + (int64_t)n * h * w;
    const float ry = (float)p.input_h / (float)h, rx = (float)p.input_w / (float)w;
    const int img_h = p.from_sizes ? p.img_h[n] : 0, img_w = p.from_sizes ? p.img_w[n] : 0;
    unsigned char *mask = static_cast<unsigned char *>(p.mask_flatten);
    if (k < pl.cchunks[l]) {                         // the same for the whole workgroup: columns
        const int j = k * 64 + lane;
        if (j >= w) return;
        unsigned short *cy = counts + base;
        const bool col_out = p.from_sizes && nearest_src(j, rx, p.input_w) >= img_w;
        unsigned cnt = 0;
        for (int i = 0; i < h; ++i) {
            const int at = i * w + j;
            const bool m = p.from_sizes ? (col_out || nearest_src(i, ry, p.input_h) >= img_h) : given[at] != 0;
            mask[base + at] = m ? 1 : 0;
            cnt += m ? 0u : 1u;
            cy[at] = (unsigned short)cnt;
        }
        if (j == 0) p.valid_ratios[((int64_t)n * p.levels + l) * 2 + 1] = valid_ratio(cnt, h);
    } else {
        const int i = (k - pl.cchunks[l]) * 64 + lane;
        if (i >= h) return;
        unsigned short *cx = counts + (int64_t)p.batch * p.tokens_per_image + base;
        const bool row_out = p.from_sizes && nearest_src(i, ry, p.input_h) >= img_h;
        unsigned cnt = 0;
        for (int j = 0; j < w; ++j) {
            const int at = i * w + j;
            const bool m = p.from_sizes ? (row_out || nearest_src(j, rx, p.input_w) >= img_w) : given[at] != 0;
            cnt += m ? 0u : 1u;
            cx[at] = (unsigned short)cnt;
        }
        if (i == 0) p.valid_ratios[((int64_t)n * p.levels + l) * 2] = valid_ratio(cnt, w);
    }
}

// ---- 2. token rows -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pyramid_emit_kernel(const semidetr_pyramid_inputs p, const Plan pl, const unsigned short *counts)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.tfirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.tfirst[l], T = pl.tiles[l];
    const int n = r / T, p0 = (r - n * T) * kTile;
    const int h = p.h[l], w = p.w[l], hw = h * w, npix = min(kTile, hw - p0);
    const bool xhalf = lane >= 32;
    const int64_t base = (int64_t)n * p.tokens_per_image + p.start[l];
    const unsigned short *cnt = counts + (xhalf ? (int64_t)p.batch * p.tokens_per_image : 0) + base;
    const float4 d = *reinterpret_cast<const float4 *>((xhalf ? p.dim_tx : p.dim_ty) + ((4 * lane) & (kBlock - 1)));
    float4 le = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.level_embed) le = ld4(p.level_embed, p.level_embed_type, (int64_t)l * kC + 4 * lane);
    // reference points: lane k < 2 L holds coordinate k & 1 (0: x, 1: y) towards level k >> 1
    const bool ref_lane = p.reference_points && lane < 2 * p.levels;
    const float *vr = p.valid_ratios + (int64_t)n * p.levels * 2;
    const int c = lane & 1;
    const float own = ref_lane ? vr[2 * l + c] : 0.f, other = ref_lane ? vr[lane] : 0.f, size = c ? (float)h : (float)w;
    for (int pp = wave; pp < npix; pp += kWaves) {
        const int pix = p0 + pp, i = pix / w, j = pix - i * w;
        const unsigned here = cnt[pix], total = cnt[xhalf ? i * w + (w - 1) : (h - 1) * w + j];
        float4 e = embed4(coordinate(p, here, total), d);
        if (p.level_embed) e = add4(e, le);
        st4(p.pos, p.pos_type, (base + pix) * kC + 4 * lane, e);
        if (ref_lane) p.reference_points[(base + pix) * (2 * p.levels) + lane] = ref_point((float)(c ? i : j), own, size, other);
    }
}

// ---- 3. backward: rows -> slots ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pyramid_grad_rows_kernel(const semidetr_pyramid_inputs p, const Plan pl, float *slots)
{
    __shared__ __attribute__((aligned(16))) float part[kWaves][kC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l = level_of(pl.ufirst, p.levels, blockIdx.x);
    const int r = blockIdx.x - pl.ufirst[l], U = pl.units[l];
    const int n = r / U, u0 = (r - n * U) * kUnit;
    const int rows = min(kUnit, p.h[l] * p.w[l] - u0);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int rr = wave; rr < rows; rr += kWaves)
        acc = add4(acc, ld4(p.g, p.g_type, n * p.g_stride[0] + (p.start[l] + u0 + rr) * p.g_stride[1] + 4 * lane));
    reinterpret_cast<float4 *>(part[wave])[lane] = acc;
    __syncthreads();
    slots[(int64_t)blockIdx.x * kC + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

// ---- 4. backward: slots -> level_embed gradient ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kC * kParts) void pyramid_grad_sum_kernel(const semidetr_pyramid_inputs p, const Plan pl, const float *slots)
{
    __shared__ double part[kParts][kC];
    const int col = threadIdx.x & (kC - 1), k = threadIdx.x / kC, l = blockIdx.x;
    const int num = pl.ufirst[l + 1] - pl.ufirst[l];
    const float *base = slots + (int64_t)pl.ufirst[l] * kC + col;
    const int chunk = (num + kParts - 1) / kParts;
    const int first = min(k * chunk, num), last = min(first + chunk, num);
    double acc = 0.0;
    for (int sl = first; sl < last; ++sl) acc += (double)base[(int64_t)sl * kC];
    part[k][col] = acc;
    __syncthreads();
    if (k == 0) {
        #pragma unroll
        for (int j = 1; j < kParts; ++j) acc += part[j][col];
        st1(p.grad_level_embed, p.level_embed_type, (int64_t)l * kC + col, (float)acc);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
bool known_type(int type) { return type == SEMIDETR_ROW_F32 || type == SEMIDETR_ROW_FP16 || type == SEMIDETR_ROW_BF16; }
bool aligned(const void *ptr, int type) { return ((uintptr_t)ptr & (type == SEMIDETR_ROW_F32 ? 15 : 7)) == 0; }
bool aligned16(const void *ptr) { return ((uintptr_t)ptr & 15) == 0; }

// The sizes of the block alone (what the workspace query needs) and the grids.
int plan_sizes(const semidetr_pyramid_inputs &p, Plan &pl)
{
    SEMIDETR_REQUIRE(p.levels >= 1 && p.levels <= kMaxLevels, SEMIDETR_E_BADARG, "pyramid_inputs: %d levels (1 .. %d)", p.levels, kMaxLevels);
    SEMIDETR_REQUIRE(p.batch >= 1 && p.batch <= kMaxBatch, SEMIDETR_E_BADARG,
                     "pyramid_inputs: %d images (1 .. %d: the image sizes travel by value)", p.batch, kMaxBatch);
    SEMIDETR_REQUIRE(p.tokens_per_image >= 1, SEMIDETR_E_BADARG, "pyramid_inputs: bad sizes (tokens_per_image=%lld)",
                     (long long)p.tokens_per_image);
    SEMIDETR_REQUIRE(p.tokens_per_image < ((int64_t)1 << 31) && (int64_t)p.batch * p.tokens_per_image * kC < ((int64_t)1 << 31),
                     SEMIDETR_E_TOOLARGE, "pyramid_inputs: too large (batch * tokens_per_image * 256 < 2^31)");
    int64_t end = 0;
    pl.sfirst[0] = pl.tfirst[0] = pl.ufirst[0] = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        int64_t hw = 0;
        pl.cchunks[l] = pl.rchunks[l] = 0;
        if (l < p.levels) {
            SEMIDETR_REQUIRE(p.h[l] >= 1 && p.w[l] >= 1 && p.h[l] < 65536 && p.w[l] < 65536, SEMIDETR_E_BADARG,
                             "pyramid_inputs: level %d is (%d, %d); 1 .. 65535 each (16-bit counts)", l, p.h[l], p.w[l]);
            hw = (int64_t)p.h[l] * p.w[l];
            SEMIDETR_REQUIRE(p.start[l] >= end && hw <= p.tokens_per_image - p.start[l], SEMIDETR_E_BADARG,
                             "pyramid_inputs: rows [%lld, %lld + %lld) of level %d overlap the level before it or pass tokens_per_image=%lld",
                             (long long)p.start[l], (long long)p.start[l], (long long)hw, l, (long long)p.tokens_per_image);
            end = p.start[l] + hw;
            pl.cchunks[l] = (p.w[l] + 63) / 64;
            pl.rchunks[l] = (p.h[l] + 63) / 64;
        }
        pl.tiles[l] = (int)((hw + kTile - 1) / kTile);
        pl.units[l] = (int)((hw + kUnit - 1) / kUnit);
        pl.sfirst[l + 1] = pl.sfirst[l] + p.batch * (pl.cchunks[l] + pl.rchunks[l]);
        pl.tfirst[l + 1] = pl.tfirst[l] + p.batch * pl.tiles[l];
        pl.ufirst[l + 1] = pl.ufirst[l] + p.batch * pl.units[l];
    }
    return SEMIDETR_OK;
}

size_t workspace_bytes(const semidetr_pyramid_inputs &p, const Plan &pl, int for_backward)
{
    return for_backward ? (size_t)pl.ufirst[p.levels] * kC * sizeof(float)
                        : (size_t)2 * p.batch * p.tokens_per_image * sizeof(unsigned short);
}

// Host-side check of the parameter block and the workspace.
int plan(const semidetr_pyramid_inputs *params, int for_backward, const void *workspace, size_t bytes, Plan &pl)
{
    SEMIDETR_REQUIRE(params, SEMIDETR_E_BADARG, "pyramid_inputs: null pointer (parameter block)");
    const semidetr_pyramid_inputs &p = params[0];
    if (int rc = plan_sizes(p, pl)) return rc;
    SEMIDETR_REQUIRE(workspace && aligned16(workspace) && bytes >= workspace_bytes(p, pl, for_backward), SEMIDETR_E_BADARG,
                     "pyramid_inputs: workspace null, misaligned or smaller than semidetr_pyramid_inputs_workspace_bytes()");
    if (for_backward) {
        SEMIDETR_REQUIRE(known_type(p.g_type) && known_type(p.level_embed_type), SEMIDETR_E_BADARG,
                         "pyramid_inputs backward: unknown type code (g_type=%d level_embed_type=%d; SEMIDETR_ROW_F32 / _FP16 / _BF16)",
                         p.g_type, p.level_embed_type);
        SEMIDETR_REQUIRE(p.g && aligned(p.g, p.g_type) && p.g_stride[0] >= 0 && p.g_stride[1] >= 0 && p.g_stride[0] % 4 == 0 &&
                             p.g_stride[1] % 4 == 0, SEMIDETR_E_BADARG,
                         "pyramid_inputs backward: g null or its rows not %d-byte aligned (base; strides non-negative multiples of 4 elements)",
                         p.g_type == SEMIDETR_ROW_F32 ? 16 : 8);
        SEMIDETR_REQUIRE(p.grad_level_embed && aligned(p.grad_level_embed, p.level_embed_type), SEMIDETR_E_BADARG,
                         "pyramid_inputs backward: grad_level_embed null or misaligned");
        return SEMIDETR_OK;
    }
    if (p.from_sizes) {
        SEMIDETR_REQUIRE(p.input_h >= 1 && p.input_w >= 1, SEMIDETR_E_BADARG, "pyramid_inputs: bad input shape (%d, %d)", p.input_h, p.input_w);
        for (int n = 0; n < p.batch; ++n)
            SEMIDETR_REQUIRE(p.img_h[n] >= 0 && p.img_h[n] <= p.input_h && p.img_w[n] >= 0 && p.img_w[n] <= p.input_w, SEMIDETR_E_BADARG,
                             "pyramid_inputs: image %d is (%d, %d), outside the input shape (%d, %d)", n, p.img_h[n], p.img_w[n],
                             p.input_h, p.input_w);
    } else {
        for (int l = 0; l < p.levels; ++l)
            SEMIDETR_REQUIRE(p.masks[l], SEMIDETR_E_BADARG, "pyramid_inputs: null pointer (masks[%d]; from_sizes is 0)", l);
    }
    SEMIDETR_REQUIRE(p.offset == p.offset && p.eps == p.eps && p.scale == p.scale, SEMIDETR_E_BADARG, "pyramid_inputs: a NaN setting");
    SEMIDETR_REQUIRE(!p.normalize || p.eps > 0.0f, SEMIDETR_E_BADARG,
                     "pyramid_inputs: normalize needs eps > 0 (a column without a valid pixel divides by eps alone)");
    SEMIDETR_REQUIRE(known_type(p.pos_type) && (!p.level_embed || known_type(p.level_embed_type)), SEMIDETR_E_BADARG,
                     "pyramid_inputs: unknown type code (pos_type=%d level_embed_type=%d; SEMIDETR_ROW_F32 / _FP16 / _BF16)",
                     p.pos_type, p.level_embed_type);
    SEMIDETR_REQUIRE(p.dim_ty && p.dim_tx && aligned16(p.dim_ty) && aligned16(p.dim_tx), SEMIDETR_E_BADARG,
                     "pyramid_inputs: dim_ty / dim_tx null or not 16-byte aligned");
    SEMIDETR_REQUIRE(!p.level_embed || aligned(p.level_embed, p.level_embed_type), SEMIDETR_E_BADARG, "pyramid_inputs: level_embed misaligned");
    SEMIDETR_REQUIRE(p.pos && aligned(p.pos, p.pos_type), SEMIDETR_E_BADARG, "pyramid_inputs: pos null or misaligned");
    SEMIDETR_REQUIRE(p.mask_flatten && p.valid_ratios && ((uintptr_t)p.valid_ratios & 3) == 0, SEMIDETR_E_BADARG,
                     "pyramid_inputs: mask_flatten / valid_ratios null or misaligned");
    SEMIDETR_REQUIRE(((uintptr_t)p.reference_points & 3) == 0, SEMIDETR_E_BADARG, "pyramid_inputs: reference_points misaligned");
    return SEMIDETR_OK;
}

}  // namespace

extern "C" size_t semidetr_pyramid_inputs_workspace_bytes(const semidetr_pyramid_inputs *params, int for_backward)
{
    // sizes only: the pointers of the block are not looked at
    Plan pl;
    if (!params || plan_sizes(params[0], pl)) return 0;
    return workspace_bytes(params[0], pl, for_backward);
}

extern "C" int semidetr_pyramid_inputs_forward(void *stream, const semidetr_pyramid_inputs *params, void *workspace, size_t workspace_bytes)
{
    Plan pl;
    if (int rc = plan(params, 0, workspace, workspace_bytes, pl)) return rc;
    const semidetr_pyramid_inputs &p = params[0];
    hipStream_t st = semidetr::as_stream(stream);
    unsigned short *counts = static_cast<unsigned short *>(workspace);
    hipLaunchKernelGGL(pyramid_scan_kernel, dim3(pl.sfirst[p.levels]), dim3(64), 0, st, p, pl, counts);
    if (int rc = semidetr::launch_status("pyramid_scan_kernel")) return rc;
    hipLaunchKernelGGL(pyramid_emit_kernel, dim3(pl.tfirst[p.levels]), dim3(kThreads), 0, st, p, pl, counts);
    return semidetr::launch_status("pyramid_emit_kernel");
}

extern "C" int semidetr_pyramid_inputs_backward(void *stream, const semidetr_pyramid_inputs *params, void *workspace, size_t workspace_bytes)
{
    Plan pl;
    if (int rc = plan(params, 1, workspace, workspace_bytes, pl)) return rc;
    const semidetr_pyramid_inputs &p = params[0];
    hipStream_t st = semidetr::as_stream(stream);
    float *slots = static_cast<float *>(workspace);
    hipLaunchKernelGGL(pyramid_grad_rows_kernel, dim3(pl.ufirst[p.levels]), dim3(kThreads), 0, st, p, pl, slots);
    if (int rc = semidetr::launch_status("pyramid_grad_rows_kernel")) return rc;
    hipLaunchKernelGGL(pyramid_grad_sum_kernel, dim3(p.levels), dim3(kC * kParts), 0, st, p, pl, slots);
    return semidetr::launch_status("pyramid_grad_sum_kernel");
}

// Sample geometry and raw-buffer helpers shared by the MSDA translation units (msda.hip: fp32 / fp64, msda_h16.hip: fp16 / bf16
// value maps): the pixel mapping with its individually rounded multiply / subtract, the corner records in element and in byte
// form, and the bounds-checked buffer loads whose out-of-range result IS the op's zero padding.  Included INSIDE the including
// file's (anonymous) namespace, after <hip/hip_runtime.h>; both files sample with this one copy, so a 16-bit value map selects
// exactly the cells the fp32 op selects.  (msda_lanes.h is the sibling header for what the two files' fast kernels share beyond
// the geometry: the DPP lane reductions and the workgroup -> tile mapping.)
#pragma once

// ---------------------------------------------------------------------------------------------
// sample geometry (ms_deform_im2col_cuda.cuh:285-288 pixel mapping, :56-78 corner validity)
// ---------------------------------------------------------------------------------------------
// Individually rounded multiply / subtract.  HIP's __fmul_rn / __fsub_rn are plain operators that hipcc's default
// -ffp-contract=fast fuses into one fma(y, H, -0.5); the pixel coordinate (hence floor(), the bilinear cell)
// must round exactly like the oracle's two C operations, so contraction is switched off for these four.
template <typename T>
__device__ __forceinline__ T mul_rn(T a, T b)
{
#pragma clang fp contract(off)
    return a * b;
}
template <typename T>
__device__ __forceinline__ T sub_rn(T a, T b)
{
#pragma clang fp contract(off)
    return a - b;
}

// off[i] = element offset of corner i relative to (value + n*S*M*D + m*D), or -1 when the corner is
// outside the level (zero padding).  Returns false when the whole sample is skipped.
template <typename T>
__device__ __forceinline__ bool sample_setup(T x, T y, int H, int W, int start, int rowstride,
                                             int (&off)[4], T &lw, T &lh)
{
    const T h = sub_rn(mul_rn(y, (T)H), (T)0.5);
    const T w = sub_rn(mul_rn(x, (T)W), (T)0.5);
    off[0] = off[1] = off[2] = off[3] = -1;
    lw = lh = 0;
    if (!(h > (T)-1 && w > (T)-1 && h < (T)H && w < (T)W)) return false;
    const int h0 = (int)floor(h), w0 = (int)floor(w);
    lh = sub_rn(h, (T)h0);
    lw = sub_rn(w, (T)w0);
    const bool top = h0 >= 0, bot = h0 + 1 <= H - 1, lef = w0 >= 0, rig = w0 + 1 <= W - 1;
    const int base = (start + h0 * W + w0) * rowstride;
    if (top && lef) off[0] = base;
    if (top && rig) off[1] = base + rowstride;
    if (bot && lef) off[2] = base + W * rowstride;
    if (bot && rig) off[3] = base + (W + 1) * rowstride;
    return true;
}

// Same geometry for the fast-path kernels that LOAD the corners, in the form the buffer instructions want:
// off[i] = BYTE offset of corner i inside the image's value slice (head / channel offset not included), or
// kOob for a corner outside the level / a skipped sample.  The kernels read the value map through a raw buffer
// resource whose size is exactly one image slice: the hardware bounds check of buffer_load returns 0 for kOob,
// which IS the op's zero padding -- no per-corner exec-mask branches, no zero-initialised destination
// registers in the hot loop (they were 1/3 of its VALU instructions), and values elsewhere in memory can never
// leak into a sample (NaN-safe exactly like the reference).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOob = 0xFFFFF000u;       // + any in-row lane offset (< 4096) stays out of range, no wrap

__device__ __forceinline__ bool sample_setup_oob(float x, float y, int H, int W, int start, unsigned row_bytes,
                                                 unsigned (&off)[4], float &lw, float &lh)
{
    const float h = sub_rn(mul_rn(y, (float)H), 0.5f);
    const float w = sub_rn(mul_rn(x, (float)W), 0.5f);
    off[0] = off[1] = off[2] = off[3] = kOob;
    lw = lh = 0;
    if (!(h > -1.f && w > -1.f && h < (float)H && w < (float)W)) return false;
    const int h0 = (int)floorf(h), w0 = (int)floorf(w);
    lh = sub_rn(h, (float)h0);
    lw = sub_rn(w, (float)w0);
    const bool top = h0 >= 0, bot = h0 + 1 <= H - 1, lef = w0 >= 0, rig = w0 + 1 <= W - 1;
    const unsigned base = (unsigned)(start + h0 * W + w0) * row_bytes;     // may wrap for h0/w0 == -1: unused then
    if (top && lef) off[0] = base;
    if (top && rig) off[1] = base + row_bytes;
    if (bot && lef) off[2] = base + (unsigned)W * row_bytes;
    if (bot && rig) off[3] = base + (unsigned)(W + 1) * row_bytes;
    return true;
}

// ---------------------------------------------------------------------------------------------
// location arithmetic of the fused MSDeformAttn prologue (ms_deform_attn.py:102-108), shared by the fp32 kernels' RawIO
// (msda_fast.h) and the 16-bit kernels' RawIO16 (msda_h16.hip): loc = ref + off * scale, per coordinate
// ---------------------------------------------------------------------------------------------
// 1 / x as ONE v_rcp_f32 (1 ulp).  __frcp_rn is the correctly rounded reciprocal -- on gfx950 the full IEEE division
// sequence (v_div_scale / v_rcp / 4 fma / v_div_fmas / v_div_fixup), ten instructions where the fused prologue wants one.
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// scale = d loc / d offset: (1 / W, 1 / H) for 2-d points (:102-105), 0.5 / P x the box's (w, h) = r.zw for 4-d boxes (:106-108).
// x / W as x * rcp(W) (v_rcp_f32, 1 ulp): a true division is ~10 instructions per coordinate, and the location is
// compared with the reference's to 1e-4, not bit for bit (the oracle-exact path is LocAttnIO)
__device__ __forceinline__ float2 fused_loc_scale(const float4 r, int ref_dim, int P, int H, int W)
{
    const bool box = ref_dim == 4;
    const float ip = 0.5f * fast_rcp((float)P);
    return make_float2(box ? ip * r.z : fast_rcp((float)W), box ? ip * r.w : fast_rcp((float)H));
}
// o: the raw offset, r: the reference point {x, y[, w, h]}
__device__ __forceinline__ void fused_loc_xy(const float2 o, const float4 r, int ref_dim, int P, int H, int W, float &x, float &y)
{
    const float2 s = fused_loc_scale(r, ref_dim, P, H, W);
    x = r.x + o.x * s.x;
    y = r.y + o.y * s.y;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const float *image_base, unsigned image_bytes)
{
    // The descriptor is wave-uniform (it depends on blockIdx only) but the compiler cannot prove it and would
    // wrap every buffer op in a waterfall loop; readfirstlane of its inputs makes the uniformity explicit.
    const unsigned long long b = reinterpret_cast<unsigned long long>(image_base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    const unsigned nb = __builtin_amdgcn_readfirstlane(image_bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo), 0, nb,
                                             0x00020000);
}
__device__ __forceinline__ float4 buf_ld4(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float2 buf_ld2(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, byte_off, 0, 0));
}
__device__ __forceinline__ float buf_ld1(__amdgpu_buffer_rsrc_t r, unsigned byte_off)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

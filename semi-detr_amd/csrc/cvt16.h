// The two 16-bit storage types of the mixed-precision kernels (msda_h16.hip -- the value rows and, in RawIO16, the raw offsets /
// logits --, add_norm.hip, self_attn.hip, group_norm_tokens.hip, ref_points.hip): exact up-cast, one
// round-to-nearest-even down-cast (fp16 overflows to inf, as the conversion does), and the pack / unpack of four neighbouring
// elements = two dwords.  T16 = __half | __hip_bfloat16.  Included INSIDE the namespace of the file that uses it, after
// <hip/hip_runtime.h>, <hip/hip_fp16.h> and <hip/hip_bf16.h>.
#pragma once

template <typename T16>
struct Cvt;
template <>
struct Cvt<__half> {
    static __device__ __forceinline__ float up(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
    static __device__ __forceinline__ unsigned down(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
};
template <>
struct Cvt<__hip_bfloat16> {
    static __device__ __forceinline__ float up(unsigned bits) { return __uint_as_float(bits << 16); }
    static __device__ __forceinline__ unsigned down(float f)
    {
        return __builtin_bit_cast(unsigned short, __float2bfloat16(f));      // v_cvt_pk_bf16_f32 on gfx950
    }
};
// four channels of a row = two dwords (channel 0 in the low half of the first)
template <typename T16>
__device__ __forceinline__ float4 unpack4(float2 raw)
{
    const unsigned a = __float_as_uint(raw.x), b = __float_as_uint(raw.y);
    return make_float4(Cvt<T16>::up(a & 0xffffu), Cvt<T16>::up(a >> 16), Cvt<T16>::up(b & 0xffffu), Cvt<T16>::up(b >> 16));
}
template <typename T16>
__device__ __forceinline__ unsigned pack2(float lo, float hi)
{
    return Cvt<T16>::down(lo) | (Cvt<T16>::down(hi) << 16);
}
template <typename T16>
__device__ __forceinline__ float ld16(const T16 *p)
{
    return Cvt<T16>::up(*reinterpret_cast<const unsigned short *>(p));
}
template <typename T16>
__device__ __forceinline__ void st16(T16 *p, float f)
{
    *reinterpret_cast<unsigned short *>(p) = (unsigned short)Cvt<T16>::down(f);
}

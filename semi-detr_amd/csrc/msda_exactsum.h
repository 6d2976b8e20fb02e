// Exact, order-independent summation of fp32 numbers: a long fixed-point accumulator (the "superaccumulator" of Kulisch) sized
// for fp32.  Five 64-bit words, two's complement, bit 0 = 2^-149 (the smallest subnormal): a finite fp32 number occupies bits
// 0..276, so 320 bits hold any sum of up to 2^32 of them (277 + 32 bits + sign) without overflow, and every add is exact.  The
// sum is rounded ONCE, to nearest even, when it is read -- its bits are a function of the SET of addends, whatever the order
// and however the addends were split among accumulators (merge is exact too).
//
// Non-finite addends never enter the words: they set flags, and the result is what IEEE addition gives in EVERY order -- NaN if
// a NaN or both infinities were seen, otherwise the infinity seen, otherwise the rounded sum (which itself overflows to +-inf
// exactly when the exact sum rounds beyond FLT_MAX; a sequential fp32 sum may overflow earlier or not at all).
//
// Plain C++ on the host (tests/host/msda_exactsum_host_check.cpp builds it alone), __host__ __device__ under hipcc.  The word
// array is only ever indexed by constants: the addend is placed with selects and the carry chains are unrolled, so on the GPU
// the accumulator lives in registers (10 dwords + the flags), never in scratch.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SEMIDETR_EXACT_HD __host__ __device__ __forceinline__
#else
#define SEMIDETR_EXACT_HD inline
#endif

namespace semidetr_exact {

constexpr unsigned kSawNan = 1u, kSawPosInf = 2u, kSawNegInf = 4u;

SEMIDETR_EXACT_HD uint32_t float_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}
SEMIDETR_EXACT_HD float bits_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
SEMIDETR_EXACT_HD int top_bit64(uint64_t x)      // index of the highest set bit, x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)x);
#else
    return 63 - __builtin_clzll(x);
#endif
}

struct ExactSum {
    uint64_t w[5];       // two's complement, bit 0 = 2^-149
    uint32_t flags;      // kSawNan | kSawPosInf | kSawNegInf

    SEMIDETR_EXACT_HD void clear()
    {
        w[0] = w[1] = w[2] = w[3] = w[4] = 0;
        flags = 0;
    }

    // w += a (320 bits) + carry_in, the chain unrolled
    SEMIDETR_EXACT_HD void add_words(const uint64_t a0, const uint64_t a1, const uint64_t a2, const uint64_t a3, const uint64_t a4,
                                     uint64_t carry)
    {
#define SEMIDETR_EXACT_STEP(i, a)                       \
    {                                                   \
        const uint64_t t = w[i] + (a);                  \
        const uint64_t c1 = t < (a) ? 1u : 0u;          \
        const uint64_t u = t + carry;                   \
        const uint64_t c2 = u < t ? 1u : 0u;            \
        w[i] = u;                                       \
        carry = c1 | c2;                                \
    }
        SEMIDETR_EXACT_STEP(0, a0)
        SEMIDETR_EXACT_STEP(1, a1)
        SEMIDETR_EXACT_STEP(2, a2)
        SEMIDETR_EXACT_STEP(3, a3)
        SEMIDETR_EXACT_STEP(4, a4)
#undef SEMIDETR_EXACT_STEP
    }

    SEMIDETR_EXACT_HD void add(float f)
    {
        const uint32_t b = float_bits(f);
        const uint32_t e = (b >> 23) & 0xffu, m = b & 0x7fffffu;
        const bool neg = (b >> 31) != 0;
        if (e == 0xffu) {
            flags |= m ? kSawNan : (neg ? kSawNegInf : kSawPosInf);
            return;
        }
        // |f| = mant * 2^(sh - 149): subnormals have sh = 0 and no implicit bit
        const uint64_t mant = e ? (uint64_t)(m | 0x800000u) : (uint64_t)m;
        const uint32_t sh = e ? e - 1u : 0u;                   // 0..253
        const uint32_t wi = sh >> 6, bo = sh & 63u;            // first word 0..3, bit offset inside it
        const uint64_t lo = mant << bo;
        const uint64_t hi = (mant >> 1) >> (63u - bo);         // the bits that cross into the next word (bo > 40), else 0
        const uint64_t s = neg ? ~(uint64_t)0 : (uint64_t)0;   // a negative addend is added as ~a + 1
        const uint64_t a0 = (wi == 0 ? lo : 0) ^ s;
        const uint64_t a1 = ((wi == 1 ? lo : 0) | (wi == 0 ? hi : 0)) ^ s;
        const uint64_t a2 = ((wi == 2 ? lo : 0) | (wi == 1 ? hi : 0)) ^ s;
        const uint64_t a3 = ((wi == 3 ? lo : 0) | (wi == 2 ? hi : 0)) ^ s;
        const uint64_t a4 = (wi == 3 ? hi : 0) ^ s;
        add_words(a0, a1, a2, a3, a4, neg ? 1u : 0u);
    }

    SEMIDETR_EXACT_HD void merge(const ExactSum &o)
    {
        add_words(o.w[0], o.w[1], o.w[2], o.w[3], o.w[4], 0u);
        flags |= o.flags;
    }

    // one round-to-nearest-even of the exact sum
    SEMIDETR_EXACT_HD float round_to_float() const
    {
        if ((flags & kSawNan) || (flags & (kSawPosInf | kSawNegInf)) == (kSawPosInf | kSawNegInf)) return bits_float(0x7fc00000u);
        if (flags & kSawPosInf) return bits_float(0x7f800000u);
        if (flags & kSawNegInf) return bits_float(0xff800000u);
        const bool neg = (w[4] >> 63) != 0;
        // magnitude: ~w + 1 for a negative sum
        const uint64_t s = neg ? ~(uint64_t)0 : (uint64_t)0;
        uint64_t m0 = w[0] ^ s, m1 = w[1] ^ s, m2 = w[2] ^ s, m3 = w[3] ^ s, m4 = w[4] ^ s;
        uint64_t c = neg ? 1u : 0u;
        m0 += c; c = (c && m0 == 0) ? 1u : 0u;
        m1 += c; c = (c && m1 == 0) ? 1u : 0u;
        m2 += c; c = (c && m2 == 0) ? 1u : 0u;
        m3 += c; c = (c && m3 == 0) ? 1u : 0u;
        m4 += c;
        const uint32_t sign = neg ? 0x80000000u : 0u;
        // the highest non-zero word `hi` (index t), the word below it `lo`, and whether anything is set below that one
        int t;
        uint64_t hi, lo;
        bool below;
        if (m4) { t = 4; hi = m4; lo = m3; below = (m2 | m1 | m0) != 0; }
        else if (m3) { t = 3; hi = m3; lo = m2; below = (m1 | m0) != 0; }
        else if (m2) { t = 2; hi = m2; lo = m1; below = m0 != 0; }
        else if (m1) { t = 1; hi = m1; lo = m0; below = false; }
        else { t = 0; hi = m0; lo = 0; below = false; }
        if (t == 0 && hi < (1u << 24)) return bits_float(sign | (uint32_t)hi);      // zero, subnormals and the first binade: exact
        const int hb = top_bit64(hi);
        const int h = 64 * t + hb;                         // the sum's leading bit: |sum| in [2^(h-149), 2^(h-148))
        if (h >= 277) return bits_float(sign | 0x7f800000u);                         // >= 2^128
        // the 128 bits hi:lo shifted so that the leading bit is bit 63 of x
        const uint64_t x = (hi << (63 - hb)) | ((lo >> 1) >> hb);
        const uint64_t y = lo << (63 - hb);
        const uint32_t mant = (uint32_t)(x >> 40);         // 24 bits, the implicit one included
        const bool half = ((x >> 39) & 1u) != 0;
        const bool sticky = (x & (((uint64_t)1 << 39) - 1)) != 0 || y != 0 || below;
        // exponent field h - 22; mant's implicit bit adds the 1, and a carry out of the mantissa moves on into the exponent
        uint32_t r = ((uint32_t)(h - 23) << 23) + mant;
        if (half && (sticky || (mant & 1u))) r += 1u;
        if (r >= 0x7f800000u) r = 0x7f800000u;
        return bits_float(sign | r);
    }
};

}  // namespace semidetr_exact

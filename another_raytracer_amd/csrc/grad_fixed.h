// grad_fixed.h — the exact accumulator of rt_radiance_grad: an f64 contribution as a 192-bit two's-complement integer
// count of quanta of 2^-96, three 64-bit limbs (w[0] the least significant).  Integer sums commute, so a sum of such
// integers does not depend on the order of its terms; it is rounded to f64 once (to nearest, ties to even) at the end.
//   fix_from_double  x -> trunc(x * 2^96): the magnitude is truncated towards zero (|x| < 2^-96 gives 0, and so do
//                    +-0 and every subnormal); false for a non-finite x and for |x| >= 2^56, which no accumulator holds
//                    (the caller marks the sum NaN).  2^39 terms of the largest magnitude cannot overflow the 191
//                    value bits: more than a call's 2^31 paths add to a row at 255 vertices each.
//   fix_add          a += b, modulo 2^192
//   fix_to_double    the correctly rounded f64 of an accumulator; +0.0 for zero
// Host and device: tests/native/grad_fixed_check.cpp drives it on the CPU, radiance_grad.hip on the GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ART_FX_HD __host__ __device__ inline
#else
#define ART_FX_HD inline
#endif

namespace art {

constexpr int kFixFracBits = 96;   // the quantum is 2^-96
constexpr int kFixLimitExp = 56;   // |x| < 2^56

struct Fix192 {
    uint64_t w[3];
};

ART_FX_HD uint64_t fix_bits(double x) {
    uint64_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = static_cast<uint64_t>(__double_as_longlong(x));
#else
    __builtin_memcpy(&b, &x, sizeof b);
#endif
    return b;
}
ART_FX_HD double fix_double(uint64_t b) {
    double x;
#if defined(__HIP_DEVICE_COMPILE__)
    x = __longlong_as_double(static_cast<long long>(b));
#else
    __builtin_memcpy(&x, &b, sizeof x);
#endif
    return x;
}

ART_FX_HD void fix_negate(Fix192& a) {
    a.w[0] = ~a.w[0] + 1u;
    const uint64_t c0 = a.w[0] == 0 ? 1u : 0u;
    a.w[1] = ~a.w[1] + c0;
    const uint64_t c1 = (c0 && a.w[1] == 0) ? 1u : 0u;
    a.w[2] = ~a.w[2] + c1;
}

ART_FX_HD bool fix_from_double(double x, Fix192& out) {
    const uint64_t b = fix_bits(x);
    const int e = static_cast<int>((b >> 52) & 0x7ffu);
    out.w[0] = out.w[1] = out.w[2] = 0;
    if (e == 0x7ff || e >= 1023 + kFixLimitExp) return false;  // inf, NaN, |x| >= 2^56
    if (e == 0) return true;                                   // +-0, subnormals: below the quantum
    const uint64_t mant = (b & 0xfffffffffffffull) | (1ull << 52);
    // x = mant * 2^(e - 1075): mant * 2^(e - 1075 + 96) quanta
    const int s = e - 1075 + kFixFracBits;  // <= 99
    if (s <= -53) return true;
    if (s < 0) {
        out.w[0] = mant >> (-s);
    } else {
        const int bit = s & 63;
        const uint64_t lo = mant << bit, hi = bit ? mant >> (64 - bit) : 0;
        if (s < 64) out.w[0] = lo, out.w[1] = hi;
        else out.w[1] = lo, out.w[2] = hi;
    }
    if ((b >> 63) && (out.w[0] | out.w[1] | out.w[2])) fix_negate(out);
    return true;
}

ART_FX_HD void fix_add(Fix192& a, const Fix192& b) {
    const uint64_t s0 = a.w[0] + b.w[0];
    const uint64_t c0 = s0 < b.w[0] ? 1u : 0u;
    const uint64_t t1 = a.w[1] + b.w[1];
    const uint64_t s1 = t1 + c0;
    const uint64_t c1 = (t1 < b.w[1] || s1 < c0) ? 1u : 0u;
    a.w[0] = s0, a.w[1] = s1, a.w[2] = a.w[2] + b.w[2] + c1;
}

ART_FX_HD int fix_clz64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll(static_cast<long long>(v));
#else
    return __builtin_clzll(v);
#endif
}

ART_FX_HD double fix_to_double(Fix192 a) {
    const bool neg = (a.w[2] >> 63) != 0;
    if (neg) fix_negate(a);
    if ((a.w[0] | a.w[1] | a.w[2]) == 0) return 0.0;
    // p: the position of the magnitude's leading bit
    const int top = a.w[2] ? 2 : (a.w[1] ? 1 : 0);
    const int p = 64 * top + 63 - fix_clz64(a.w[top]);
    uint64_t mant;
    if (p <= 52) {
        mant = a.w[0] << (52 - p);  // exact
    } else {
        // the 53 bits [p - 52, p], the guard bit p - 53 and whether any bit below it is set
        const int lo = p - 52;  // >= 1
        auto bits_from = [&](int at) -> uint64_t {  // the 64 bits [at, at + 63] of the magnitude, at >= 0
            const int word = at >> 6, bit = at & 63;
            uint64_t v = a.w[word] >> bit;
            if (bit && word < 2) v |= a.w[word + 1] << (64 - bit);
            return v;
        };
        mant = bits_from(lo) & ((1ull << 53) - 1);
        const int g = lo - 1;
        const bool guard = ((a.w[g >> 6] >> (g & 63)) & 1u) != 0;
        bool sticky = false;
        for (int word = 0; word < 3; ++word) {
            const int below = g - 64 * word;  // bits of this word under the guard bit
            if (below >= 64) sticky = sticky || a.w[word] != 0;
            else if (below > 0) sticky = sticky || (a.w[word] & ((1ull << below) - 1)) != 0;
        }
        if (guard && (sticky || (mant & 1u))) ++mant;  // 2^53 carries into the exponent below
    }
    const uint64_t expo = static_cast<uint64_t>(p - kFixFracBits + 1023);
    const uint64_t bits = (expo << 52) + (mant - (1ull << 52));
    return fix_double(bits | (neg ? 1ull << 63 : 0ull));
}

}  // namespace art

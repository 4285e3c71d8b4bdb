// s2k_text_dev.h -- decimal text on the device, for the kernels that format lines (s2k_gaf.hip): how many digits a
// value takes, by one comparison against a table of powers of ten, and the digits themselves, by multiply-high.  No division: a
// 64-bit division is a subroutine of some forty instructions on this target, and a line of GAF holds a dozen numbers.
#pragma once
#include <stdint.h>

#include "s2k_dev.h"

namespace s2k {
namespace {

__device__ const uint64_t POW10_64[20] = {1ull,
                                          10ull,
                                          100ull,
                                          1000ull,
                                          10000ull,
                                          100000ull,
                                          1000000ull,
                                          10000000ull,
                                          100000000ull,
                                          1000000000ull,
                                          10000000000ull,
                                          100000000000ull,
                                          1000000000000ull,
                                          10000000000000ull,
                                          100000000000000ull,
                                          1000000000000000ull,
                                          10000000000000000ull,
                                          100000000000000000ull,
                                          1000000000000000000ull,
                                          10000000000000000000ull};
__device__ const uint32_t POW10_32[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

// The decimal digits of v, 1 for 0.  With b the bits of v | 1, t = b * 1233 >> 12 is floor(log10(v)) or one above it (1233 / 4096 is
// log10(2) from above, and exact enough up to 64 bits); the table decides.  v | 1 compares as v does: 10^t is even for t >= 1.
__device__ __forceinline__ uint32_t dec_digits(uint64_t v) {
    const uint64_t x = v | 1u;
    const uint32_t t = ((64u - (uint32_t)__clzll((long long)x)) * 1233u) >> 12;
    return t + 1u - (x < POW10_64[t] ? 1u : 0u);
}
__device__ __forceinline__ uint32_t dec_digits(uint32_t v) {
    const uint32_t x = v | 1u;
    const uint32_t t = ((32u - (uint32_t)__clz((int)x)) * 1233u) >> 12;
    return t + 1u - (x < POW10_32[t] ? 1u : 0u);
}

// v as nd = dec_digits(v) bytes at p, the last digit first: v / 10 = mulhi(v, ceil(2^(w + 3) / 10)) >> 3 for every w-bit v; the loop
// goes on in 32 bits as soon as the value fits
__device__ __forceinline__ void put_dec(uint8_t *__restrict__ p, uint64_t v, uint32_t nd) {
    while (v >> 32) {
        const uint64_t q = __umul64hi(v, 0xCCCCCCCCCCCCCCCDull) >> 3;
        p[--nd] = (uint8_t)('0' + (uint32_t)(v - q * 10u));
        v = q;
    }
    uint32_t x = (uint32_t)v;
    while (nd) {
        const uint32_t q = __umulhi(x, 0xCCCCCCCDu) >> 3;
        p[--nd] = (uint8_t)('0' + (x - q * 10u));
        x = q;
    }
}

// `text` (n bytes, no terminator) at p
__device__ __forceinline__ void put_text(uint8_t *__restrict__ p, const char *text, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) p[i] = (uint8_t)text[i];
}

} // namespace
} // namespace s2k

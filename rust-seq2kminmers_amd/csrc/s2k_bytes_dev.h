// s2k_bytes_dev.h -- sixteen bytes in two register pairs: what the output-ordered byte copies share (s2k_seq.hip, the stitch, DESIGN.md
// §3.11; s2k_align.hip, the walk targets, §3.20): the fetch from aligned words, the byte shifts, and the reverse complement in
// registers.
#pragma once
#include <cstdint>

#include "s2k_dev.h"

namespace s2k {
namespace {

constexpr uint64_t B01 = 0x0101010101010101ull;

// ---- 16 bytes in two registers pairs --------------------------------------------------------------------------------------------
// bytes [p, p + 16) of memory in (lo, hi), little endian, of which the first n (1 .. 16) are wanted: only the aligned 8-byte words
// that hold a wanted byte are loaded, so nothing outside the words of [p, p + n) is touched; bytes past n are undefined
__device__ __forceinline__ void fetch16(const uint8_t *p, uint32_t n, uint64_t &lo, uint64_t &hi) {
    const uint64_t a = (uint64_t)p, last = (a + n - 1) & ~7ull;
    const uint64_t *w = (const uint64_t *)(a & ~7ull);
    const uint32_t s = (uint32_t)(a & 7u) * 8u;
    const uint64_t w0 = w[0];
    const uint64_t w1 = (uint64_t)(w + 1) <= last ? w[1] : 0ull;
    const uint64_t w2 = (uint64_t)(w + 2) <= last ? w[2] : 0ull;
    lo = s ? (w0 >> s) | (w1 << (64u - s)) : w0;
    hi = s ? (w1 >> s) | (w2 << (64u - s)) : w1;
}
// keep the low n bytes (1 .. 16)
__device__ __forceinline__ void keep_low(uint32_t n, uint64_t &lo, uint64_t &hi) {
    if (n >= 16) return;
    if (n >= 8) hi = n == 8 ? 0ull : hi & ((1ull << ((n - 8) * 8)) - 1ull);
    else {
        hi = 0;
        lo &= (1ull << (n * 8)) - 1ull;
    }
}
__device__ __forceinline__ void shl_bytes(uint32_t b, uint64_t &lo, uint64_t &hi) { // b in 0 .. 15
    if (b == 0) return;
    if (b < 8) {
        hi = (hi << (b * 8)) | (lo >> (64 - b * 8));
        lo <<= b * 8;
    } else {
        hi = lo << ((b - 8) * 8);
        lo = 0;
    }
}
__device__ __forceinline__ void shr_bytes(uint32_t b, uint64_t &lo, uint64_t &hi) { // b in 0 .. 15
    if (b == 0) return;
    if (b < 8) {
        lo = (lo >> (b * 8)) | (hi << (64 - b * 8));
        hi >>= b * 8;
    } else {
        lo = hi >> ((b - 8) * 8);
        hi = 0;
    }
}
// 0x80 in every byte of y that is zero, 0 elsewhere (exact: no carry leaves a byte)
__device__ __forceinline__ uint64_t zero_bytes(uint64_t y) { return ~(((y & (0x7F * B01)) + 0x7F * B01) | y | (0x7F * B01)); }
// ACGTacgt -> TGCAtgca in every byte, every other byte as it is: A ^ T == 0x15, C ^ G == 0x04, the case bit stays
__device__ __forceinline__ uint64_t comp8(uint64_t x) {
    const uint64_t f = x & (0xDF * B01);
    const uint64_t at = zero_bytes(f ^ (0x41 * B01)) | zero_bytes(f ^ (0x54 * B01));
    const uint64_t cg = zero_bytes((f ^ (0x43 * B01)) & (0xFB * B01)); // 0x43 and 0x47
    return x ^ ((at >> 7) * 0x15) ^ ((cg >> 7) * 0x04);
}
// the low n bytes (1 .. 16) of (lo, hi) reversed and complemented, in the low n bytes; zeros above
__device__ __forceinline__ void revcomp_low(uint32_t n, uint64_t &lo, uint64_t &hi) {
    uint64_t a = __builtin_bswap64(hi), b = __builtin_bswap64(lo);
    shr_bytes(16 - n, a, b);
    lo = comp8(a);
    hi = comp8(b);
}

} // namespace
} // namespace s2k

// s2k_table_dev.h -- the count table's device view and its fused look-ups, shared by the translation units that search a table
// (s2k_table.hip: look-up, filter, edges; s2k_seq.hip: representatives, node sequences; s2k_thread.hip: read paths), and the searches
// of km_off that map an item to its read and a tile to the reads that start in it.  The tile geometry (TB_THREADS, TB_Q, TB_TILE, TB_WORDS) comes from s2k_compact_dev.h.  DESIGN.md §3.8.
#pragma once
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"

namespace s2k {
namespace {

constexpr uint64_t TB_KEYS_PER_BUCKET = 4; // B = floor(log2(n / 4)): 4-7 keys per bucket on average
constexpr uint32_t TB_MAX_BITS = 26;

struct TableView {
    const uint64_t *keys;
    const uint32_t *counts; // NULL: membership table (count 1)
    const uint32_t *dir;    // 2^bits + 1 entries
    uint32_t n;
    uint32_t shift;         // 64 - bits
};

// c[r] = count of q[r] in the table (0 if absent); with POS also rank[r] = its index in the table (0 if absent).  The look-up and
// the filter use POS = false, the instantiation that compiles to the code they had before the ranks existed.
template <bool POS>
__device__ inline void lookup_many(const TableView &tv, const uint64_t (&q)[TB_Q], uint32_t (&c)[TB_Q], uint32_t *rank) {
    if (tv.n == 0) {
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            c[r] = 0;
            if (POS) rank[r] = 0;
        }
        return;
    }
    uint32_t lo[TB_Q], hi[TB_Q], pos[TB_Q];
    bool hit[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) { // every directory load in flight before the first use
        const uint64_t p = q[r] >> tv.shift;
        lo[r] = tv.dir[p];
        hi[r] = tv.dir[p + 1];
    }
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hit[r] = false;
        pos[r] = 0;
    }
    for (;;) { // TB_Q searches side by side; a finished one reloads its last key (a cache hit) instead of branching around the load
        uint64_t kv[TB_Q];
        uint32_t mid[TB_Q];
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            mid[r] = (lo[r] + hi[r]) >> 1;
            kv[r] = tv.keys[std::min<uint32_t>(mid[r], tv.n - 1)];
        }
        bool more = false;
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            if (lo[r] < hi[r]) {
                if (kv[r] < q[r]) lo[r] = mid[r] + 1;
                else if (kv[r] > q[r]) hi[r] = mid[r];
                else { // keys are strictly ascending: the one match
                    hit[r] = true;
                    pos[r] = mid[r];
                    lo[r] = hi[r];
                }
                more |= lo[r] < hi[r];
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (int r = 0; r < TB_Q; r++) c[r] = hit[r] ? (tv.counts ? tv.counts[pos[r]] : 1u) : 0u;
    if (POS) {
#pragma unroll
        for (int r = 0; r < TB_Q; r++) rank[r] = pos[r];
    }
}

// one query (the edge kernel's halo item): *c its count, *pos its index (both 0 if absent)
__device__ inline void lookup_one(const TableView &tv, uint64_t q, uint32_t *c, uint32_t *pos) {
    *c = *pos = 0;
    if (tv.n == 0) return;
    const uint64_t p = q >> tv.shift;
    uint32_t lo = tv.dir[p], hi = tv.dir[p + 1];
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t k = tv.keys[mid];
        if (k < q) lo = mid + 1;
        else if (k > q) hi = mid;
        else {
            *c = tv.counts ? tv.counts[mid] : 1u;
            *pos = mid;
            return;
        }
    }
}

// the last read r in [lo, hi] with km_off[r] <= j (km_off[lo] <= j holds)
__device__ inline uint64_t read_of(const uint64_t *__restrict__ km_off, uint64_t lo, uint64_t hi, uint64_t j) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (km_off[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the first r in [0, n_reads] with km_off[r] > x (n_reads + 1 if there is none)
__device__ inline uint64_t reads_upto(const uint64_t *__restrict__ km_off, uint64_t n_reads, uint64_t x) {
    uint64_t lo = 0, hi = n_reads + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (km_off[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

} // namespace
} // namespace s2k

struct s2k_table {
    s2k_ctx *ctx;
    const uint64_t *keys;
    const uint32_t *counts;
    uint64_t n;
    uint32_t bits;
    uint32_t *dir; // 2^bits + 1 entries, then the validation flag
    s2k::TableView view() const { return s2k::TableView{keys, counts, dir, (uint32_t)n, 64u - bits}; }
};

// s2k_graph_dev.h -- what the kernel families that walk oriented ids grid-stride share (s2k_unitig.hip, DESIGN.md §3.10;
// s2k_simplify.hip, §3.12): the launch shape, the block sum behind their counters, the rules of a CSR row and the search of one (also s2k_span_dev.h, s2k_untangle.hip).
#pragma once
#include <algorithm>

#include "s2k_dev.h"

namespace s2k {
namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int UT = 256;           // threads per block
constexpr unsigned UB_MAX = 4096; // blocks of a grid-stride launch (one counter atomic per block and counter)

__host__ inline unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + UT - 1) / UT, UB_MAX); }

// the sums of v[0 .. N) over the block, each added to its word by one lane (nothing when it is 0)
template <int N, typename T>
__device__ __forceinline__ void block_add(T (&v)[N], unsigned long long *words) {
    __shared__ T part[UT / 64][N];
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += __shfl_down(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        unsigned long long s = 0;
        for (int w = 0; w < UT / 64; w++) s += part[w][threadIdx.x];
        if (s) atomicAdd(words + threadIdx.x, s);
    }
}
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long *word) {
    unsigned long long one[1] = {v};
    block_add(one, word);
}

// row u of a CSR of n_ids rows over n_edges entries: *a, *b = its bounds; false when they break the rules (row_off[0] == 0,
// non-decreasing, nothing past n_edges, the last row ends there) -- then nothing may be read through them
__device__ __forceinline__ bool csr_row_ok(const uint64_t *__restrict__ row_off, uint64_t u, uint64_t n_ids, uint64_t n_edges, uint64_t *a,
                                           uint64_t *b) {
    *a = row_off[u], *b = row_off[u + 1];
    return !((u == 0 && *a != 0) || (u == n_ids - 1 && *b != n_edges) || *a > *b || *b > n_edges);
}

struct Csr {
    const uint64_t *row_off;
    const uint32_t *dst;
};

// the index of B in the row of A (strictly ascending), NONE if it is not there; both bounds are loaded before the first probe
__device__ __forceinline__ uint32_t find_edge(const Csr &g, uint32_t A, uint32_t B) {
    uint64_t lo = g.row_off[A], hi = g.row_off[A + 1];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint32_t v = g.dst[mid];
        if (v < B) lo = mid + 1;
        else if (v > B) hi = mid;
        else return (uint32_t)mid;
    }
    return NONE;
}

// the CSR rules of s2k_graph_simplify_mask for row u
__device__ __forceinline__ bool csr_ids_ok(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst, uint64_t u, uint64_t n_ids,
                                           uint64_t n_edges) {
    uint64_t a, b;
    if (!csr_row_ok(row_off, u, n_ids, n_edges, &a, &b)) return false;
    bool ok = true;
    for (uint64_t e = a; e < b; e++)
        if (dst[e] >= n_ids) ok = false;
    return ok;
}

} // namespace
} // namespace s2k

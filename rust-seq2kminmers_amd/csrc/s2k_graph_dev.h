// s2k_graph_dev.h -- what the kernel families that walk oriented ids grid-stride share (s2k_unitig.hip, DESIGN.md §3.10;
// s2k_simplify.hip, §3.12): the launch shape, the block sum behind their counters and the rule of a CSR row.
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

} // namespace
} // namespace s2k

// s2k_targets_dev.h -- what the calls that walk a read walk's stitched path share (s2k_align.hip, the walk targets, DESIGN.md §3.20;
// s2k_pileup.hip, the pile-up, §3.21): the inputs, the check pass, the per-step advance and broken-junction pass, the per-walk
// length pass and the search of a non-decreasing prefix.
#pragma once
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"

namespace s2k {
namespace {

constexpr int TG_T = 256; // threads per block of the per-step and per-walk passes

// the last i in [lo, hi] with off[i] <= x (off[lo] <= x holds)
__device__ inline uint64_t last_le(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct TgIn {
    const uint64_t *first_step, *path_start, *path_end;
    const uint32_t *n_steps, *flags, *unitig;
    const uint64_t *out_off;
    const uint8_t *out;
    const uint32_t *overlap;
    uint64_t n_walks, n_all_steps, n_unitigs, n_bases;
};

__device__ __forceinline__ uint64_t unitig_len(const TgIn &in, uint32_t U) { return in.out_off[(U >> 1) + 1] - in.out_off[U >> 1]; }

__global__ __launch_bounds__(UT) void tg_check_kernel(TgIn in, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t g = i0; g < in.n_all_steps; g += stride)
        if (in.unitig[g] >= 2 * in.n_unitigs) ok = false;
    for (uint64_t t = i0; t < in.n_unitigs; t += stride) {
        const uint64_t a = in.out_off[t], b = in.out_off[t + 1];
        if (a > b || b > in.n_bases || b - a >= (1ull << 32)) ok = false;
    }
    for (uint64_t w = i0; w < in.n_walks; w += stride) {
        const uint64_t f = in.first_step[w];
        if (f > in.n_all_steps || in.n_steps[w] > in.n_all_steps - f) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(TG_T) void tg_steps_kernel(TgIn in, uint32_t *__restrict__ adv, uint32_t *__restrict__ broken) {
    const uint64_t g = (uint64_t)blockIdx.x * TG_T + threadIdx.x;
    if (g >= in.n_all_steps) return;
    const uint32_t U = in.unitig[g];
    const uint64_t L = unitig_len(in, U); // the check pass: below 2^32
    adv[g] = (uint32_t)(L - std::min<uint64_t>(in.overlap[U], L));
    uint32_t b = 0;
    if (g) {
        const uint32_t P = in.unitig[g - 1];
        b = in.overlap[P] > std::min(unitig_len(in, P), L);
    }
    broken[g] = b;
}

__global__ __launch_bounds__(TG_T) void tg_len_kernel(TgIn in, const uint64_t *__restrict__ G, const uint64_t *__restrict__ J, uint32_t *__restrict__ len,
                                                      uint8_t *__restrict__ bad8, uint32_t *__restrict__ bad) {
    const uint64_t w = (uint64_t)blockIdx.x * TG_T + threadIdx.x;
    if (w >= in.n_walks) return;
    const uint64_t f = in.first_step[w], n = in.n_steps[w], ps = in.path_start[w], pe = in.path_end[w];
    bool b = ps > pe;
    if (in.flags[w] & S2K_WALK_CIRCULAR) b = b || n == 0 || unitig_len(in, in.unitig[f]) == 0;
    else {
        const uint64_t total = n ? G[f + n - 1] - G[f] + unitig_len(in, in.unitig[f + n - 1]) : 0;
        b = b || pe > total || (n > 1 && J[f + n] != J[f + 1]);
    }
    const uint64_t l = b ? 0 : pe - ps;
    if (l >= (1ull << 32)) atomicOr(bad, 2u);
    len[w] = (uint32_t)l;
    bad8[w] = b ? 1 : 0;
}

} // namespace
} // namespace s2k

// s2k_targets_dev.h -- what the calls that walk a read walk's stitched path share (s2k_align.hip, the walk targets, DESIGN.md §3.20;
// s2k_pileup.hip, the pile-up, §3.21; s2k_segment.hip, the segments, §3.22): the inputs, the check pass, the per-step advance and
// broken-junction pass, the per-walk length pass, the search of a non-decreasing prefix, the step cursor (which step owns byte X of
// a walk's path) and the host side of the prelude: its pieces of the workspace and its launches.
#pragma once
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
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

// ---- the step cursor ------------------------------------------------------------------------------------------------------------------
// (the pile-up's; tg_copy_kernel of s2k_align.hip keeps its own copy of the search, which measured faster there, and
// tests/test_pileup.py holds the two to one answer)
// A walk and the prefix entry of its first step: step j's string starts at byte G[f + j] - g0 of the walk's stitched path.
struct Walk {
    uint64_t f, n, ps, pe, g0;
    bool circ;
};
__device__ __forceinline__ Walk walk_of(const TgIn &in, const uint64_t *__restrict__ G, uint64_t w) {
    const uint64_t f = in.first_step[w];
    return Walk{f, in.n_steps[w], in.path_start[w], in.path_end[w], G[f], (in.flags[w] & S2K_WALK_CIRCULAR) != 0};
}
// the end of step j's string on the stitched path
__device__ __forceinline__ uint64_t end_of(const TgIn &in, const uint64_t *__restrict__ G, const Walk &k, uint64_t j) {
    return G[k.f + j] - k.g0 + unitig_len(in, in.unitig[k.f + j]);
}
// the step that owns byte X of a walk's path that is not circular: the last j with j == 0 or the end of step j - 1 <= X
__device__ __forceinline__ uint64_t owner_step(const TgIn &in, const uint64_t *__restrict__ G, const Walk &k, uint64_t X) {
    uint64_t j = 0;
    for (uint64_t b = k.n - 1; j < b;) {
        const uint64_t mid = (j + b + 1) >> 1;
        if (end_of(in, G, k, mid - 1) <= X) j = mid;
        else b = mid - 1;
    }
    return j;
}

// ---- host: the prelude of an entry point ----------------------------------------------------------------------------------------------
// Per step adv, broken and the prefix G; with `lengths` also the prefix J of broken and per walk the target's length and the bad
// byte (24 B per step and 5 B per walk; without: 16 B per step).
struct TgPieces {
    bool lengths;
    Layout::Piece<uint32_t> adv, brk;
    Layout::Piece<uint64_t> G, J;
    Layout::Piece<uint32_t> len;
    Layout::Piece<uint8_t> bad8;
};
inline TgPieces carve_targets(Layout &L, uint64_t n_steps, uint64_t n_walks, bool lengths) {
    TgPieces p{};
    p.lengths = lengths;
    p.adv = L.take<uint32_t>(n_steps), p.brk = L.take<uint32_t>(n_steps);
    p.G = L.take<uint64_t>(n_steps + 1);
    if (lengths) {
        p.J = L.take<uint64_t>(n_steps + 1);
        p.len = L.take<uint32_t>(n_walks);
        p.bad8 = L.take<uint8_t>(n_walks);
    }
    return p;
}
inline void launch_tg_check(Call &c, const TgIn &in, uint32_t *bad) {
    c.launch(tg_check_kernel, grid_for(std::max<uint64_t>(std::max(in.n_all_steps, in.n_walks), std::max<uint64_t>(in.n_unitigs, 1))), UT, in, bad);
}
// the steps and their scans: G, and J when the lengths follow
inline void launch_tg_steps(Call &c, const TgIn &in, const TgPieces &p, char *w, uint64_t *tmp) {
    if (!in.n_all_steps) return;
    c.launch(tg_steps_kernel, (unsigned)((in.n_all_steps + TG_T - 1) / TG_T), TG_T, in, p.adv(w), p.brk(w));
    c.scan(p.adv(w), in.n_all_steps, p.G(w), tmp);
    if (p.lengths) c.scan(p.brk(w), in.n_all_steps, p.J(w), tmp);
}
// every walk's length and bad byte (n_walks > 0); 2 in *bad: a target of 2^32 bytes or more
inline void launch_tg_lens(Call &c, const TgIn &in, const TgPieces &p, char *w, uint32_t *bad) {
    c.launch(tg_len_kernel, (unsigned)((in.n_walks + TG_T - 1) / TG_T), TG_T, in, p.G(w), p.J(w), p.len(w), p.bad8(w), bad);
}

} // namespace
} // namespace s2k

// s2k_span_dev.h -- which edge of the CSR over the oriented unitigs every step of a read path follows (include/s2k.h, "Step s follows
// edge e"): what the spans (s2k_span.hip) and the walks (s2k_walk.hip, §3.16) share.  One tile of TB_TILE steps per
// workgroup, lane tid holds steps r * TB_THREADS + tid.
#pragma once
#include <algorithm>

#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

constexpr uint32_t SP_NONE = 0xFFFFFFFFu; // no edge (n_edges < 2^32: an index stays below it)

struct Csr {
    const uint64_t *row_off;
    const uint32_t *dst;
};

// the index of B in the row of A (strictly ascending), SP_NONE if it is not there
__device__ __forceinline__ uint32_t find_edge(const Csr &g, uint32_t A, uint32_t B) {
    uint64_t lo = g.row_off[A], hi = g.row_off[A + 1];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint32_t v = g.dst[mid];
        if (v < B) lo = mid + 1;
        else if (v > B) hi = mid;
        else return (uint32_t)mid;
    }
    return SP_NONE;
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

struct Paths {
    const uint64_t *path_off;
    const uint32_t *unitig, *pos, *count, *flags;
    uint64_t n_reads, n_steps;
};

constexpr uint8_t SF_ATEND = 1, SF_SELF = 2; // the step ends at its unitig's last member; it is linked and begins at position 0

// a tile's steps in LDS; index x + 1 <-> step t0 + x: index 0 is the step before the tile, index TB_TILE + 1 the one after it
struct FollowLds {
    uint32_t U[TB_TILE + 2], E[TB_TILE + 2]; // the oriented unitig (SP_NONE: no such step); the edge the step follows (SP_NONE: none)
    uint8_t f[TB_TILE + 2], start[TB_TILE + 2]; // SF_*; the step starts a read
    uint64_t reads[2];
};

// What the lane's TB_Q steps are (U, ps, cnt, fl; len = the members of their unitigs) and the edge each follows (e), and all of the
// tile with its two halo steps in LDS.  The read starts in [t0, t0 + TB_TILE] are marked from the reads a binary search of path_off
// finds there; the row bounds of all TB_Q steps are loaded before the first probe and the TB_Q searches run side by side.  Ends with
// a barrier: s.E is whole.
__device__ __forceinline__ void follow_tile(const Paths &p, const Csr &g, const uint64_t *__restrict__ uni_off, uint64_t t0, FollowLds &s,
                                            uint32_t (&U)[TB_Q], uint32_t (&ps)[TB_Q], uint32_t (&cnt)[TB_Q], uint32_t (&fl)[TB_Q], uint64_t (&len)[TB_Q],
                                            uint32_t (&e)[TB_Q]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, p.n_steps - 1);
        U[r] = p.unitig[j], ps[r] = p.pos[j], cnt[r] = p.count[j], fl[r] = p.flags[j];
    }
    if (tid < 2) s.reads[tid] = tid ? reads_upto(p.path_off, p.n_reads, t0 + TB_TILE) : t0 ? reads_upto(p.path_off, p.n_reads, t0 - 1) : 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) len[r] = uni_off[(U[r] >> 1) + 1] - uni_off[U[r] >> 1];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int x = r * TB_THREADS + tid;
        const bool valid = t0 + x < p.n_steps;
        s.U[x + 1] = valid ? U[r] : SP_NONE;
        s.f[x + 1] = valid ? (uint8_t)(((uint64_t)ps[r] + cnt[r] == len[r] ? SF_ATEND : 0) | ((fl[r] & S2K_STEP_LINKED) && ps[r] == 0 ? SF_SELF : 0)) : 0;
        s.start[x + 1] = 0;
    }
    if (tid == 0 || tid == 64) { // the two halo steps, one lane of two different waves
        const uint64_t j = tid == 0 ? t0 + TB_TILE : t0 - 1; // t0 - 1 wraps to 2^64 - 1 for the first tile: no such step
        uint32_t hU = SP_NONE;
        uint8_t hf = 0;
        if (j < p.n_steps) {
            hU = p.unitig[j];
            const uint64_t hl = uni_off[(hU >> 1) + 1] - uni_off[hU >> 1];
            const uint32_t hp = p.pos[j];
            hf = (uint8_t)(((uint64_t)hp + p.count[j] == hl ? SF_ATEND : 0) | ((p.flags[j] & S2K_STEP_LINKED) && hp == 0 ? SF_SELF : 0));
        }
        const int i = tid == 0 ? TB_TILE + 1 : 0;
        s.U[i] = hU;
        s.f[i] = hf;
        s.start[i] = 0;
        s.E[i] = SP_NONE;
    }
    __syncthreads();
    for (uint64_t r = s.reads[0] + tid; r < s.reads[1]; r += TB_THREADS) {
        const uint64_t x = p.path_off[r] - t0; // in [0, TB_TILE] for a non-decreasing path_off
        if (x <= TB_TILE) s.start[x + 1] = 1;
    }
    __syncthreads();
    // index i may follow an edge out of index i - 1 (i >= 1): everything but the search
    auto may_follow = [&](int i) { return (s.f[i] & SF_SELF) && !s.start[i] && s.U[i - 1] != SP_NONE && (s.f[i - 1] & SF_ATEND); };
    uint64_t lo[TB_Q], hi[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) { // every row bound in flight before the first probe
        const int i = r * TB_THREADS + tid + 1;
        const bool m = t0 + (i - 1) < p.n_steps && may_follow(i);
        const uint32_t A = m ? s.U[i - 1] : 0u;
        lo[r] = g.row_off[A];
        hi[r] = m ? g.row_off[A + 1] : lo[r];
        e[r] = SP_NONE;
    }
    for (;;) { // TB_Q searches side by side
        bool more = false;
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            if (lo[r] < hi[r]) {
                const uint64_t mid = (lo[r] + hi[r]) >> 1;
                const uint32_t v = g.dst[mid], B = U[r];
                if (v < B) lo[r] = mid + 1;
                else if (v > B) hi[r] = mid;
                else {
                    e[r] = (uint32_t)mid;
                    lo[r] = hi[r];
                }
                more |= lo[r] < hi[r];
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (int r = 0; r < TB_Q; r++) s.E[r * TB_THREADS + tid + 1] = e[r];
    if (tid == 0 && may_follow(TB_TILE + 1)) s.E[TB_TILE + 1] = find_edge(g, s.U[TB_TILE], s.U[TB_TILE + 1]); // the step after the tile
    __syncthreads();
}

} // namespace
} // namespace s2k

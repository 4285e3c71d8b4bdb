// s2k_span_dev.h -- which edge of the CSR over the oriented unitigs every step of a read path follows (include/s2k.h, "Step s follows
// edge e"): what the spans (s2k_span.hip), the walks (s2k_walk.hip, §3.16) and the lift (s2k_lift.hip, §3.18) share, and the rules that the
// check kernels of every read-path call have in common.  One tile of TB_TILE steps per
// workgroup, lane tid holds steps r * TB_THREADS + tid.
#pragma once
#include <algorithm>

#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

constexpr uint32_t SP_NONE = NONE; // no edge (n_edges < 2^32: an index stays below it)

struct Paths {
    const uint64_t *path_off;
    const uint32_t *unitig, *pos, *count, *flags;
    uint64_t n_reads, n_steps;
};

// host: a read-path input is all there: path_off, and the step arrays every call reads (item: also item) when there are steps
inline bool paths_given(const s2k_thread_out *paths, uint64_t n_steps, bool item) {
    if (!paths || !paths->path_off) return false;
    return !n_steps || (paths->unitig && paths->pos && paths->count && paths->flags && (!item || paths->item));
}
inline Paths paths_of(const s2k_thread_out *paths, uint64_t n_reads, uint64_t n_steps) {
    return Paths{paths->path_off, paths->unitig, paths->pos, paths->count, paths->flags, n_reads, n_steps};
}

// ---- what the check kernels of the read-path calls share: every read is clamped to the arrays whatever they hold -------------------
// path_off runs from 0 to n_steps without decreasing (the reads i0, i0 + stride, ..)
__device__ __forceinline__ bool path_off_ok(const uint64_t *__restrict__ path_off, uint64_t n_reads, uint64_t n_steps, uint64_t i0, uint64_t stride) {
    bool ok = true;
    for (uint64_t r = i0; r <= n_reads; r += stride) {
        const uint64_t a = path_off[r];
        if (r == 0 && a != 0) ok = false;
        if (r == n_reads ? a != n_steps : a > path_off[r + 1]) ok = false;
    }
    return ok;
}

// every step (i0, i0 + stride, ..) lies on a unitig below n_ids, has items and lies inside its unitig (it may run round a circular one)
__device__ __forceinline__ bool steps_ok(const uint32_t *__restrict__ unitig, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ count,
                                         uint64_t n_steps, const uint64_t *__restrict__ uni_off, const uint8_t *__restrict__ circular, uint64_t n_ids,
                                         uint64_t i0, uint64_t stride) {
    bool ok = true;
    for (uint64_t s = i0; s < n_steps; s += stride) {
        const uint64_t U = unitig[s];
        if (U >= n_ids) {
            ok = false;
            continue;
        }
        const uint64_t a = uni_off[U >> 1], b = uni_off[(U >> 1) + 1], c = count[s], q = pos[s];
        if (a >= b || c == 0 || q >= b - a || (!circular[U >> 1] && q + c > b - a)) ok = false;
    }
    return ok;
}

// row u is a CSR row with ids below n_ids; for an even u, uni_off ascends at its unitig, which has fewer than 2^32 members
__device__ __forceinline__ bool unitig_row_ok(const Csr &g, const uint64_t *__restrict__ uni_off, uint64_t u, uint64_t n_ids, uint64_t n_edges) {
    bool ok = csr_ids_ok(g.row_off, g.dst, u, n_ids, n_edges);
    if (!(u & 1)) {
        const uint64_t a = uni_off[u >> 1], b = uni_off[(u >> 1) + 1];
        if (a >= b || b - a >= (1ull << 32)) ok = false;
    }
    return ok;
}

// ---- the edge a step follows ----------------------------------------------------------------------------------------------------------
// TB_Q binary searches side by side: B[r] in dst[lo[r] .. hi[r]) (strictly ascending; an empty range: no search); found(r, index)
template <typename F>
__device__ __forceinline__ void search_rows(const Csr &g, uint64_t (&lo)[TB_Q], uint64_t (&hi)[TB_Q], const uint32_t (&B)[TB_Q], F found) {
    for (;;) {
        bool more = false;
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            if (lo[r] < hi[r]) {
                const uint64_t mid = (lo[r] + hi[r]) >> 1;
                const uint32_t v = g.dst[mid];
                if (v < B[r]) lo[r] = mid + 1;
                else if (v > B[r]) hi[r] = mid;
                else {
                    found(r, mid);
                    lo[r] = hi[r];
                }
                more |= lo[r] < hi[r];
            }
        }
        if (!more) break;
    }
}

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
    search_rows(g, lo, hi, U, [&](int r, uint64_t mid) { e[r] = (uint32_t)mid; });
#pragma unroll
    for (int r = 0; r < TB_Q; r++) s.E[r * TB_THREADS + tid + 1] = e[r];
    if (tid == 0 && may_follow(TB_TILE + 1)) s.E[TB_TILE + 1] = find_edge(g, s.U[TB_TILE], s.U[TB_TILE + 1]); // the step after the tile
    __syncthreads();
}

} // namespace
} // namespace s2k

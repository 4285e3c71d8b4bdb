// s2k_coords_dev.h -- where a position of an oriented unitig lies in base space: what the walks (s2k_walk.hip) and the
// anchors of the segmented alignment (s2k_segment.hip, §3.22) share: the decomposition with its member offsets, the rules their check
// kernels have in common, and the base interval of a position (include/s2k.h, "Base interval of a position").
#pragma once
#include <algorithm>

#include "s2k_dev.h"

namespace s2k {
namespace {

// the decomposition and where its members lie in base space
struct Lift {
    const uint64_t *uni_off, *member_off, *out_off;
    const uint32_t *members, *seq_len, *overlap;
    const uint8_t *circular;
    uint64_t n_unitigs, n_nodes;
};

// the last t in [0, n_unitigs - 1] with uni_off[t] <= x: every index stays inside uni_off whatever it holds
__device__ inline uint64_t unitig_of(const uint64_t *__restrict__ uni_off, uint64_t n_unitigs, uint64_t x) {
    uint64_t lo = 0, hi = n_unitigs - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (uni_off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// unitig t: uni_off ascends strictly from 0 to n_nodes; out_off does not decrease and the unitig has fewer than 2^32 bases
__device__ __forceinline__ bool lift_unitig_ok(const Lift &v, uint64_t t) {
    const uint64_t a = v.uni_off[t], b = v.uni_off[t + 1], oa = v.out_off[t], ob = v.out_off[t + 1];
    bool ok = !(a >= b || b > v.n_nodes || (t == 0 && a != 0) || (t == v.n_unitigs - 1 && b != v.n_nodes)); // n_nodes < 2^31
    if (oa > ob || ob - oa >= (1ull << 32)) ok = false;
    return ok;
}

// member slot x: an oriented node below 2 n_nodes whose offset lies inside its unitig's bases (the unitig by a search of uni_off)
__device__ __forceinline__ bool lift_member_ok(const Lift &v, uint64_t x) {
    bool ok = v.members[x] < 2 * v.n_nodes;
    const uint64_t t = unitig_of(v.uni_off, v.n_unitigs, x), o = v.member_off[x];
    if (o < v.out_off[t] || o > v.out_off[t + 1]) ok = false;
    return ok;
}

// The base interval [*lo, *hi) of position q of the oriented unitig U on its own strand (include/s2k.h, "Base interval of a
// position"), *L = the unitig's bases.  A linear unitig clamps hi to L.  A circular one does not; on its twin strand the interval is
// shifted by *w, the multiple of L that brings lo into [0, L) (0 elsewhere).
__device__ __forceinline__ void interval(const Lift &v, uint32_t U, uint64_t q, uint64_t *lo, uint64_t *hi, uint64_t *L, uint64_t *w) {
    const uint64_t t = U >> 1, a = v.uni_off[t], len = v.uni_off[t + 1] - a, o0 = v.out_off[t];
    const uint64_t x = a + ((U & 1u) ? len - 1 - q : q);
    const uint64_t o = v.member_off[x] - o0;
    uint64_t e = o + v.seq_len[v.members[x] >> 1];
    *L = v.out_off[t + 1] - o0;
    *w = 0;
    if (!v.circular[t]) e = std::min(e, *L);
    if (!(U & 1u)) {
        *lo = o, *hi = e;
        return;
    }
    if (e > *L) *w = *L ? ((e - 1) / *L) * *L : e;
    *lo = *w + *L - e;
    *hi = *w + *L - o;
}

} // namespace
} // namespace s2k

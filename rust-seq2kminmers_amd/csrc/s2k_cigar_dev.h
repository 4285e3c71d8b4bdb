// s2k_cigar_dev.h -- the CIGAR run word and the run slots of a batch of alignments (include/s2k.h, s2k_align_out): what the trace
// (s2k_align.hip), the pile-up (s2k_pileup.hip, §3.21) and the join (s2k_segment.hip, §3.22) share.  A run is one
// 32-bit word len << 4 | op; record i owns the slots ops_off[i] .. ops_off[i + 1) of which its n_ops[i] first hold runs.
#pragma once
#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"

namespace s2k {
namespace {

__device__ __forceinline__ uint32_t run_op(uint32_t v) { return v & 15u; }
__device__ __forceinline__ uint32_t run_len(uint32_t v) { return v >> 4; }
__device__ __forceinline__ uint32_t run_pack(uint32_t op, uint32_t len) { return len << 4 | op; }
// a run an alignment may hold: not of length 0, and with a known code
__device__ __forceinline__ bool run_legal(uint32_t v) {
    const uint32_t op = run_op(v);
    return run_len(v) != 0 && (op == S2K_CIGAR_I || op == S2K_CIGAR_D || op == S2K_CIGAR_EQ || op == S2K_CIGAR_X);
}
// the bytes of target and of query that a run consumes
__device__ __forceinline__ uint32_t run_target(uint32_t v) { return run_op(v) != S2K_CIGAR_I ? run_len(v) : 0; }
__device__ __forceinline__ uint32_t run_query(uint32_t v) { return run_op(v) != S2K_CIGAR_D ? run_len(v) : 0; }

// ops_off does not decrease and ends inside the n_ops_total runs, n_ops[i] fits record i's slots (the records i0, i0 + stride, ..)
__device__ __forceinline__ bool ops_off_ok(const uint64_t *__restrict__ ops_off, const uint32_t *__restrict__ n_ops, uint64_t n, uint64_t n_ops_total, uint64_t i0,
                                           uint64_t stride) {
    bool ok = true;
    for (uint64_t i = i0; i < n; i += stride) {
        const uint64_t a = ops_off[i], b = ops_off[i + 1];
        if (a > b || b > n_ops_total || n_ops[i] > b - a) ok = false;
    }
    return ok;
}

// host: ops_off[0] and ops_off[n] (no wait: the caller's check pass has one)
inline void fetch_ops_ends(Call &c, const uint64_t *ops_off, uint64_t n, uint64_t *r0, uint64_t *r1) {
    c.fetch(r0, ops_off, 8);
    c.fetch(r1, ops_off + n, 8);
}

} // namespace
} // namespace s2k

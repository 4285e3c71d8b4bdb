// s2k_stitch_dev.h -- where every member's piece lies in the stitched unitigs: the piece-length, last-member and
// offset passes that the stitch (s2k_seq.hip: s2k_unitig_sequences) and the member offsets (s2k_walk.hip: s2k_unitig_member_offsets,
// §3.16) share, and the host sequence that runs them.
#pragma once
#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"

namespace s2k {
namespace {

constexpr int SQ_T = 256;

struct NodeView {
    const uint64_t *seq_off;
    const uint32_t *seq_len, *shift_fwd, *shift_rev;
    const uint8_t *rev, *pool;
    uint64_t pool_capacity, n_nodes;
};

__global__ __launch_bounds__(SQ_T) void piece_len_kernel(const uint32_t *__restrict__ members, uint64_t n_members, NodeView nv, uint32_t *__restrict__ len,
                                                         uint32_t *__restrict__ bad) {
    const uint64_t p = (uint64_t)blockIdx.x * SQ_T + threadIdx.x;
    if (p >= n_members) return;
    const uint32_t u = members[p], i = u >> 1;
    uint32_t l = 0;
    bool ok = i < nv.n_nodes;
    if (ok) {
        const uint32_t sl = nv.seq_len[i], rv = nv.rev[i];
        l = (u & 1u) == rv ? nv.shift_fwd[i] : nv.shift_rev[i];
        const uint64_t so = nv.seq_off[i];
        ok = rv <= 1 && nv.shift_fwd[i] <= sl && nv.shift_rev[i] <= sl && (sl == 0 || (so <= nv.pool_capacity && sl <= nv.pool_capacity - so));
    }
    if (!ok) {
        atomicOr(bad, 1u);
        l = 0;
    }
    len[p] = l;
}

__global__ __launch_bounds__(SQ_T) void unitig_last_kernel(const uint64_t *__restrict__ uni_off, const uint32_t *__restrict__ members,
                                                           const uint8_t *__restrict__ circular, uint64_t n_unitigs, uint64_t n_members, NodeView nv,
                                                           uint32_t *__restrict__ len, uint32_t *__restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * SQ_T + threadIdx.x;
    if (t >= n_unitigs) return;
    const uint64_t a = uni_off[t], b = uni_off[t + 1];
    if ((t == 0 && a != 0) || a >= b || b > n_members || (t == n_unitigs - 1 && b != n_members)) { // every unitig holds a member
        atomicOr(bad, 2u);
        return;
    }
    if (circular[t]) return;
    const uint32_t i = members[b - 1] >> 1;
    if (i < nv.n_nodes) len[b - 1] = nv.seq_len[i]; // (else piece_len_kernel has set the flag)
}

__global__ __launch_bounds__(SQ_T) void unitig_off_kernel(const uint64_t *__restrict__ uni_off, const uint32_t *__restrict__ members, uint64_t n_unitigs,
                                                          NodeView nv, const uint64_t *__restrict__ piece_off, uint64_t *__restrict__ out_off,
                                                          uint32_t *__restrict__ overlap) {
    const uint64_t t = (uint64_t)blockIdx.x * SQ_T + threadIdx.x;
    if (t > n_unitigs) return;
    const uint64_t a = uni_off[t];
    if (out_off) out_off[t] = piece_off[a];
    if (!overlap || t == n_unitigs) return;
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) { // the last member of the oriented unitig 2 t + s
        const uint32_t u = s ? members[a] ^ 1u : members[uni_off[t + 1] - 1], i = u >> 1;
        overlap[2 * t + s] = nv.seq_len[i] - ((u & 1u) == nv.rev[i] ? nv.shift_fwd[i] : nv.shift_rev[i]);
    }
}

// The passes up to the scan on c's stream: bad (16 zeroed bytes), len (n_members) and piece_off (n_members + 1) are workspace, tmp the
// scan's.  -> the flag word (0: the inputs keep the rules); *total = the bases of all unitigs.  The caller asks c.ok().
inline uint32_t stitch_offsets(Call &c, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs,
                               uint64_t n_members, const NodeView &nv, uint32_t *bad, uint32_t *len, uint64_t *piece_off, uint64_t *tmp,
                               uint64_t *total) {
    const unsigned gm = (unsigned)((n_members + SQ_T - 1) / SQ_T), gu = (unsigned)((n_unitigs + 1 + SQ_T - 1) / SQ_T);
    return c.check(bad, 16, bad, [&] {
        hipLaunchKernelGGL(piece_len_kernel, dim3(gm), dim3(SQ_T), 0, c.st, d_members, n_members, nv, len, bad);
        hipLaunchKernelGGL(unitig_last_kernel, dim3(gu), dim3(SQ_T), 0, c.st, d_uni_off, d_members, d_circular, n_unitigs, n_members, nv, len, bad);
        c.launched();
        c.scan(len, n_members, piece_off, tmp);
        c.fetch(total, piece_off + n_members, 8);
    });
}

} // namespace
} // namespace s2k

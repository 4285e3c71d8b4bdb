// s2k_walk.hip -- read walks on the unitig graph with base coordinates: where every member's piece lies in the stitched unitigs, and
// each read's steps joined into walks along the graph's edges, lifted to bases (include/s2k.h: s2k_unitig_member_offsets,
// s2k_paths_walks).
//
// s2k_unitig_member_offsets: the stitch's piece-length, last-member, scan and offset passes (s2k_stitch_dev.h) without the copy
// kernel; the scan's first n_nodes entries are the member offsets.
//
// s2k_paths_walks, runs of steps (s2k_runs_dev.h), tiles of TB_TILE steps (lane tid holds steps r * 256 + tid):
//  1. walks_check_kernel: the shared rules of s2k_span_dev.h (path_off_ok, steps_ok, unitig_row_ok) and of s2k_coords_dev.h
//     (lift_unitig_ok, lift_member_ok): uni_off runs from 0 to n_nodes; out_off does not decrease and no unitig has 2^32 bases or
//     more; every member < 2 n_nodes, its offset inside its unitig's bases (the unitig by a search of uni_off).  One flag word, read
//     by the host before anything is written; every read is clamped to the arrays whatever they hold.
//  2. walks_count_kernel: follow_tile (s2k_span_dev.h) gives the edge every step follows, to workspace and LDS.  Heads: the step
//     follows no edge; tails: the step after it follows none.  Per step adv(U) to workspace.
//  3. launch_scan_u32 over adv and over count: a walk's path_len, path_end and items are differences of two prefix entries.
//  4. run_offsets_kernel: walk_off[r] = heads before path_off[r].
//  5. walks_write_kernel: walk s is the s-th head and the s-th tail.  The tail's lane gathers the head's step, the two prefixes and
//     the two base intervals.
//
// Workspace (the context's grow-only count workspace): member offsets 12 B per member; walks 24 B per step (edge 4, adv 4, two
// prefixes 8 + 8), and per mask 8 B + 4 B per 64 steps and 4 B + 8 B per tile.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_coords_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_runs_dev.h"
#include "s2k_span_dev.h"
#include "s2k_stitch_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

struct WalkWs {
    uint32_t *edge, *adv; // per step: the edge it follows (SP_NONE: none); adv(unitig)
    uint64_t *A, *C;      // n_steps + 1: the exclusive prefixes of adv and of count
    RunWs run;            // open: the tile's first step follows an edge
};

__global__ __launch_bounds__(UT) void walks_check_kernel(Paths p, Csr g, Lift v, uint64_t n_edges, uint32_t *__restrict__ bad) {
    const uint64_t n_ids = 2 * v.n_unitigs;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(p.path_off, p.n_reads, p.n_steps, i0, stride);
    if (!steps_ok(p.unitig, p.pos, p.count, p.n_steps, v.uni_off, v.circular, n_ids, i0, stride)) ok = false;
    for (uint64_t u = i0; u < n_ids; u += stride) {
        if (!unitig_row_ok(g, v.uni_off, u, n_ids, n_edges)) ok = false;
        if (!(u & 1) && !lift_unitig_ok(v, u >> 1)) ok = false;
    }
    for (uint64_t x = i0; x < v.n_nodes; x += stride)
        if (!lift_member_ok(v, x)) ok = false;
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(TB_THREADS) void walks_count_kernel(Paths p, Csr g, Lift v, WalkWs ws,
                                                                 unsigned long long *__restrict__ totals /* followed, off-graph */) {
    __shared__ FollowLds s;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint32_t U[TB_Q], ps[TB_Q], cnt[TB_Q], fl[TB_Q], e[TB_Q];
    uint64_t len[TB_Q];
    follow_tile(p, g, v.uni_off, t0, s, U, ps, cnt, fl, len, e);
    uint64_t oa[TB_Q], ob[TB_Q];
    uint32_t ov[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) oa[r] = v.out_off[U[r] >> 1], ob[r] = v.out_off[(U[r] >> 1) + 1], ov[r] = v.overlap[U[r]];
    uint32_t n[2] = {0, 0}; // followed, off-graph
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        if (j < p.n_steps) {
            const uint32_t L = (uint32_t)(ob[r] - oa[r]); // the check pass: below 2^32
            ws.edge[j] = e[r];
            ws.adv[j] = L - std::min(ov[r], L);
            n[0] += e[r] != SP_NONE;
            n[1] += (fl[r] & S2K_STEP_LINKED) && e[r] == SP_NONE;
        }
    }
    auto valid = [&](int i) { return t0 + (i - 1) < p.n_steps; };
    run_count_end(
        ws.run, t0, p.n_steps, [&](int, int i) { return valid(i) && s.E[i] == SP_NONE; }, [&](int, int i) { return valid(i) && s.E[i + 1] == SP_NONE; },
        [&] { return s.E[1] != SP_NONE; });
    block_add(n, totals);
}

struct WalkIo {
    const uint32_t *start, *end;
    uint64_t *first_step, *items, *path_len, *path_start, *path_end;
    uint32_t *n_steps, *qstart, *qend, *flags;
};

__global__ __launch_bounds__(TB_THREADS) void walks_write_kernel(Paths p, Lift v, WalkIo io, WalkWs ws) {
    __shared__ uint4 stage4[(TB_TILE + STAGE_PAD) / 2]; // TB_TILE 64-bit elements, and a run's shift
    const int tid = threadIdx.x;
    RunTile rt;
    if (!run_tile(ws.run, p.n_steps, rt)) return;
    const uint64_t t0 = rt.t0;
    uint64_t hd[TB_Q], pstart[TB_Q], pend[TB_Q], plen[TB_Q];
    uint32_t circ = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hd[r] = pstart[r] = pend[r] = plen[r] = 0;
        if ((rt.tkeep >> r) & 1u) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t h = rt.head_of(r);
            const uint32_t Uh = p.unitig[h], Uj = p.unitig[j];
            const uint64_t last = (uint64_t)p.pos[j] + p.count[j] - 1, lenj = v.uni_off[(Uj >> 1) + 1] - v.uni_off[Uj >> 1];
            const uint64_t dA = ws.A[j] - ws.A[h];
            uint64_t lo, hi, L, w, lo2, w2;
            interval(v, Uh, p.pos[h], &lo, &hi, &L, &w);
            uint64_t turns = 0, ql = last;
            if (last >= lenj) turns = last / lenj, ql = last - turns * lenj; // only round a circular unitig
            interval(v, Uj, ql, &lo2, &hi, &L, &w2);
            hd[r] = h;
            pstart[r] = lo;
            pend[r] = dA + (hi - w2) + w + turns * L; // on a circular unitig h == j: the head's shift, and whole turns
            plen[r] = dA + L;
            circ |= (v.circular[Uj >> 1] ? 1u : 0u) << r;
        }
    }
    rt.leave_tails(io.first_step, stage4, [&](int r, uint64_t) { return hd[r]; });
    rt.leave_tails(io.items, stage4, [&](int r, uint64_t j) { return ws.C[j + 1] - ws.C[hd[r]]; });
    rt.leave_tails(io.path_len, stage4, [&](int r, uint64_t) { return plen[r]; });
    rt.leave_tails(io.path_start, stage4, [&](int r, uint64_t) { return pstart[r]; });
    rt.leave_tails(io.path_end, stage4, [&](int r, uint64_t) { return pend[r]; });
    rt.leave_tails(io.n_steps, stage4, [&](int r, uint64_t j) { return j - hd[r] + 1; });
    rt.leave_tails(io.qstart, stage4, [&](int r, uint64_t) { return io.start[hd[r]]; });
    rt.leave_tails(io.qend, stage4, [&](int, uint64_t j) { return io.end[j] + 1u; });
    rt.leave_tails(io.flags, stage4, [&](int r, uint64_t) { return (circ >> r) & 1u; });
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_unitig_member_offsets(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs,
                                     uint64_t n_nodes, const s2k_node_seqs *nodes, uint64_t *d_member_off, uint64_t *d_out_off, uint32_t *d_overlap,
                                     uint64_t *n_bases) {
    if (n_bases) *n_bases = 0;
    if (!ctx || !n_bases || !d_uni_off || !nodes) return S2K_ERR_INVALID_ARG;
    if (n_unitigs && (!d_members || !d_circular || !nodes->seq_off || !nodes->seq_len || !nodes->shift_fwd || !nodes->shift_rev || !nodes->rev))
        return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_unitig_member_offsets");
    if (n_nodes >= (1ull << 31) || n_unitigs > n_nodes) return c.invalid("2^31 nodes or more, or more unitigs than nodes");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_unitigs == 0) { // no unitigs: no nodes
        uint64_t first = 1;
        c.fetch(&first, d_uni_off, 8);
        if (!c.sync()) return c.device_error();
        if (first != 0 || n_nodes != 0) return c.invalid("uni_off must start at 0 and end at n_nodes");
        if (d_out_off) {
            c.zero(d_out_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    const uint64_t n_members = n_nodes;
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const auto len_p = L.take<uint32_t>(n_members);
    const auto off_p = L.take<uint64_t>(n_members + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_members));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint64_t *piece_off = off_p(w);
    const NodeView nv{nodes->seq_off, nodes->seq_len, nodes->shift_fwd, nodes->shift_rev, nodes->rev, nodes->pool, nodes->pool_capacity, n_nodes};
    uint64_t total = 0;
    const uint32_t hbad = stitch_offsets(c, d_uni_off, d_members, d_circular, n_unitigs, n_members, nv, flag(w), len_p(w), piece_off, tmp_p(w), &total);
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("uni_off is not the offsets of n_unitigs non-empty unitigs over n_nodes members, a member names a node >= n_nodes, or a "
                         "node record is inconsistent (rev > 1, a shift above seq_len, bytes outside the pool)");
    *n_bases = total;
    if (d_member_off) c.copy(d_member_off, piece_off, n_members * 8, hipMemcpyDeviceToDevice);
    if (d_out_off || d_overlap) {
        hipLaunchKernelGGL(unitig_off_kernel, dim3((unsigned)((n_unitigs + 1 + SQ_T - 1) / SQ_T)), dim3(SQ_T), 0, c.st, d_uni_off, d_members, n_unitigs, nv,
                           piece_off, d_out_off, d_overlap);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_paths_walks(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off,
                           const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular, uint64_t n_unitigs,
                           const uint64_t *d_member_off, const uint64_t *d_out_off, const uint32_t *d_overlap, const uint32_t *d_seq_len,
                           const uint32_t *d_members, uint64_t n_nodes, const s2k_walk_out *out, uint64_t *n_walks, uint64_t *n_followed,
                           uint64_t *n_off_graph) {
    if (n_walks) *n_walks = 0;
    if (n_followed) *n_followed = 0;
    if (n_off_graph) *n_off_graph = 0;
    if (!ctx || !n_walks || !n_followed || !n_off_graph || !paths_given(paths, n_steps, false)) return S2K_ERR_INVALID_ARG;
    if (out && n_steps && ((out->qstart && !paths->start) || (out->qend && !paths->end))) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_paths_walks");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^32 edges or more (an edge index is 32-bit)");
    if (n_nodes >= (1ull << 31) || n_unitigs > n_nodes || (n_unitigs == 0 && (n_edges || n_nodes)))
        return c.invalid("2^31 nodes or more, more unitigs than nodes, or edges or nodes without unitigs");
    if (n_unitigs && (!d_row_off || !d_uni_off || !d_circular || !d_member_off || !d_out_off || !d_overlap || !d_seq_len || !d_members || (n_edges && !d_dst)))
        return S2K_ERR_INVALID_ARG;
    const uint64_t nt = (n_steps + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many steps for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto words = L.bytes<unsigned long long>(64); // followed, off-graph; then the check's flag
    const auto edge = L.take<uint32_t>(n_steps), adv = L.take<uint32_t>(n_steps);
    const auto A = L.take<uint64_t>(n_steps + 1), C = L.take<uint64_t>(n_steps + 1);
    const auto stmp = L.bytes<uint64_t>(scan_tmp_bytes(n_steps));
    const auto runs = carve_runs(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 2);
    const WalkWs ws{edge(w), adv(w), A(w), C(w), runs(w)};
    const Paths p = paths_of(paths, n_reads, n_steps);
    const Csr g{d_row_off, d_dst};
    const Lift v{d_uni_off, d_member_off, d_out_off, d_members, d_seq_len, d_overlap, d_circular, n_unitigs, n_nodes};
    const uint32_t hbad = c.check(totals, 32, bad, [&] {
        hipLaunchKernelGGL(walks_check_kernel, dim3(grid_for(std::max(std::max(n_reads + 1, n_steps), std::max(2 * n_unitigs, n_nodes)))), dim3(UT), 0, c.st,
                           p, g, v, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("path_off that does not run from 0 to n_steps without decreasing, a step on a unitig >= n_unitigs, without items or outside "
                         "its unitig, not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, uni_off that does not ascend "
                         "strictly from 0 to n_nodes, out_off that decreases or a unitig of 2^32 bases or more, a member >= 2 * n_nodes, or a member "
                         "offset outside its unitig's bases");
    const bool records = out && (out->first_step || out->n_steps || out->items || out->qstart || out->qend || out->path_len || out->path_start ||
                                 out->path_end || out->flags);
    if (n_steps == 0) { // no steps: no walks
        if (out && out->walk_off) {
            c.zero(out->walk_off, (n_reads + 1) * 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    uint64_t total = 0;
    unsigned long long h[2] = {0, 0};
    if (!count_runs(c, ws.run, nt, runs.h.scan_tmp(w), [&] { hipLaunchKernelGGL(walks_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, v, ws, totals); },
                    &total, totals, h, 2))
        return c.device_error();
    *n_walks = total;
    *n_followed = h[0];
    *n_off_graph = h[1];
    if (!out) return S2K_OK;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (out->edge) c.copy(out->edge, ws.edge, n_steps * 4, hipMemcpyDeviceToDevice);
    if (out->walk_off) launch_run_offsets(c, paths->path_off, n_reads, n_steps, nt, ws.run, out->walk_off);
    if (records) {
        c.scan(ws.adv, n_steps, ws.A, stmp(w));
        c.scan(paths->count, n_steps, ws.C, stmp(w));
        const WalkIo io{paths->start, paths->end, out->first_step, out->items, out->path_len, out->path_start, out->path_end,
                        out->n_steps, out->qstart, out->qend, out->flags};
        if (c.ok()) {
            hipLaunchKernelGGL(walks_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, v, io, ws);
            c.launched();
        }
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

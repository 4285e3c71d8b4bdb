// s2k_bridge.hip -- error gaps in read paths bridged: consecutive steps of a read that lie a few items apart on one unitig are merged,
// and two that lie a few items apart across one edge are extended to the edge, so that the spans, walks and GAF lines downstream see
// the crossing (include/s2k.h: s2k_paths_bridge).
//
// Runs of steps (s2k_runs_dev.h), tiles of TB_TILE steps (lane tid holds steps r * 256 + tid):
//  1. bridge_check_kernel: the shared rules of s2k_span_dev.h (path_off_ok, steps_ok, unitig_row_ok).  One flag word, read by the
//     host before anything is written; every read is clamped to the arrays.
//  2. bridge_count_kernel: per step its unitig, where it ends (pos + count), the members left behind it (len - pos - count; BR_NONE
//     on a circular unitig) and the item it ends at go to LDS with the step before the tile; the read starts in [t0, t0 + TB_TILE] are
//     marked from the reads a binary search of path_off finds there.  One lane per step decides join from its neighbour in LDS; the
//     row search of kind 2 (search_rows) runs only where the limits already stand.  join goes to workspace and to LDS; one lane
//     decides the step after the tile.  Heads: join != 1; tails: the step after it is not joined by 1.  Merged and bridged joins: a
//     block sum.  An item order that would wrap gi sets the flag word, which the host reads again with the totals, before anything
//     is written.
//  3. launch_scan_u32 over count: matched is a difference of two prefix entries.
//  4. run_offsets_kernel: out path_off[r] = heads before path_off[r].
//  5. bridge_write_kernel: output step s is the s-th head and the s-th tail.  The tail's lane gathers the head's fields and the join
//     of the step after it.  There is no atomic on an output.
//
// Workspace (the context's grow-only count workspace): 9 B per step (join 1, the prefix of count 8), and per mask 8 B + 4 B per 64
// steps and 4 B + 8 B per tile.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_runs_dev.h"
#include "s2k_span_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

constexpr uint32_t BR_NONE = 0xFFFFFFFFu; // no step there (U); a circular unitig (rem)

struct BridgeIn {
    const uint64_t *path_off;
    const uint32_t *unitig, *pos, *count, *item, *flags, *start, *end;
    const uint64_t *uni_off;
    const uint8_t *circular;
    uint64_t n_reads, n_steps, n_unitigs;
    uint32_t max_gap, max_slip;
};

struct BridgeWs {
    uint8_t *join; // per step
    uint64_t *C;   // n_steps + 1: the exclusive prefix of count
    RunWs run;     // open: the tile's first step is joined to the step before it on the same unitig
};

__global__ __launch_bounds__(UT) void bridge_check_kernel(BridgeIn p, Csr g, uint64_t n_edges, uint32_t *__restrict__ bad) {
    const uint64_t n_ids = 2 * p.n_unitigs;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(p.path_off, p.n_reads, p.n_steps, i0, stride);
    if (!steps_ok(p.unitig, p.pos, p.count, p.n_steps, p.uni_off, p.circular, n_ids, i0, stride)) ok = false;
    for (uint64_t u = i0; u < n_ids; u += stride)
        if (!unitig_row_ok(g, p.uni_off, u, n_ids, n_edges)) ok = false;
    if (!ok) atomicOr(bad, 1u);
}

// a tile's steps in LDS; index x + 1 <-> step t0 + x: index 0 is the step before the tile, index TB_TILE + 1 the one after it
struct BridgeLds {
    uint32_t U[TB_TILE + 1], endp[TB_TILE + 1], rem[TB_TILE + 1], iend[TB_TILE + 1]; // of the step: unitig (BR_NONE: no such step), pos + count,
                                                                                     // len - (pos + count) (BR_NONE: circular), item + count
    uint8_t join[TB_TILE + 2], start[TB_TILE + 2], wrap[TB_TILE + 1]; // wrap: item + count does not fit 32 bits
    uint64_t reads[2];
};

// What joins a step (U, ps, it; circ: on a circular unitig; first: its read's first step) to the step before it (pU .. pWrap of
// BridgeLds) but for the row search: 0 none, 1 the same unitig, 2 across the edge pU -> U if it exists.  *slack = gi + gp; *bad is set
// when the step's items begin before those of the step before it end.
__device__ __forceinline__ uint32_t join_before_search(const BridgeIn &p, uint32_t pU, uint32_t pEndp, uint32_t pRem, uint32_t pIend, bool pWrap, uint32_t U,
                                                       uint32_t ps, uint32_t it, bool circ, bool first, uint64_t *slack, bool *bad) {
    *slack = 0;
    if (first || pU == BR_NONE) return 0;
    if (pWrap || it < pIend) {
        *bad = true;
        return 0;
    }
    if (circ || pRem == BR_NONE) return 0;
    const uint64_t gi = it - pIend;
    const bool same = pU == U && ps >= pEndp;
    const uint64_t gp = same ? (uint64_t)(ps - pEndp) : (uint64_t)pRem + ps;
    if (gi > p.max_gap || gp > p.max_gap || (gi > gp ? gi - gp : gp - gi) > p.max_slip) return 0;
    *slack = gi + gp;
    return same ? 1u : 2u;
}

__global__ __launch_bounds__(TB_THREADS) void bridge_count_kernel(BridgeIn p, Csr g, BridgeWs ws, unsigned long long *__restrict__ totals /* merged, bridged */,
                                                                  uint32_t *__restrict__ bad) {
    __shared__ BridgeLds s;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint32_t U[TB_Q], ps[TB_Q], it[TB_Q];
    bool circ[TB_Q], wrong = false;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int x = r * TB_THREADS + tid;
        const bool valid = t0 + x < p.n_steps;
        const uint64_t j = std::min<uint64_t>(t0 + x, p.n_steps - 1);
        U[r] = p.unitig[j], ps[r] = p.pos[j], it[r] = p.item[j];
        const uint32_t cnt = p.count[j];
        const uint64_t len = p.uni_off[(U[r] >> 1) + 1] - p.uni_off[U[r] >> 1], e = (uint64_t)ps[r] + cnt;
        circ[r] = p.circular[U[r] >> 1] != 0;
        s.U[x + 1] = valid ? U[r] : BR_NONE;
        s.endp[x + 1] = (uint32_t)e;
        s.rem[x + 1] = circ[r] ? BR_NONE : (uint32_t)(len - e); // the check pass: e <= len < 2^32 where the unitig is not circular
        s.iend[x + 1] = it[r] + cnt;
        s.wrap[x + 1] = (uint64_t)it[r] + cnt > 0xFFFFFFFFull;
        s.start[x + 1] = 0;
        s.join[x + 1] = 0;
    }
    if (tid < 2) s.reads[tid] = tid ? reads_upto(p.path_off, p.n_reads, t0 + TB_TILE) : t0 ? reads_upto(p.path_off, p.n_reads, t0 - 1) : 0;
    if (tid == 64) { // the step before the tile; t0 - 1 wraps to 2^64 - 1 for the first tile: no such step
        const uint64_t j = t0 - 1;
        uint32_t hU = BR_NONE, he = 0, hr = BR_NONE, hi = 0;
        bool hw = false;
        if (j < p.n_steps) {
            hU = p.unitig[j];
            const uint32_t cnt = p.count[j], hit = p.item[j];
            const uint64_t len = p.uni_off[(hU >> 1) + 1] - p.uni_off[hU >> 1], e = (uint64_t)p.pos[j] + cnt;
            he = (uint32_t)e;
            hr = p.circular[hU >> 1] ? BR_NONE : (uint32_t)(len - e);
            hi = hit + cnt;
            hw = (uint64_t)hit + cnt > 0xFFFFFFFFull;
        }
        s.U[0] = hU, s.endp[0] = he, s.rem[0] = hr, s.iend[0] = hi;
        s.wrap[0] = hw;
        s.start[0] = 0;
        s.join[0] = 0;
    }
    if (tid == 0) s.start[TB_TILE + 1] = 0, s.join[TB_TILE + 1] = 0;
    __syncthreads();
    for (uint64_t r = s.reads[0] + tid; r < s.reads[1]; r += TB_THREADS) {
        const uint64_t x = p.path_off[r] - t0; // in [0, TB_TILE] for a non-decreasing path_off
        if (x <= TB_TILE) s.start[x + 1] = 1;
    }
    __syncthreads();
    uint32_t kind[TB_Q];
    uint64_t slack[TB_Q], lo[TB_Q], hi[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) { // every row bound in flight before the first probe
        const int i = r * TB_THREADS + tid + 1;
        const bool valid = t0 + (i - 1) < p.n_steps;
        kind[r] = valid ? join_before_search(p, s.U[i - 1], s.endp[i - 1], s.rem[i - 1], s.iend[i - 1], s.wrap[i - 1] != 0, U[r], ps[r], it[r], circ[r],
                                             s.start[i] != 0, &slack[r], &wrong)
                        : 0u;
        const uint32_t A = kind[r] == 2 ? s.U[i - 1] : 0u;
        lo[r] = g.row_off[A];
        hi[r] = kind[r] == 2 ? g.row_off[A + 1] : lo[r];
        if (kind[r] == 2) kind[r] = 0; // until the edge is found
    }
    search_rows(g, lo, hi, U, [&](int r, uint64_t) { kind[r] = 2; });
    uint32_t n[2] = {0, 0}; // merged, bridged
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int x = r * TB_THREADS + tid;
        if (t0 + x < p.n_steps) {
            s.join[x + 1] = (uint8_t)kind[r];
            ws.join[t0 + x] = (uint8_t)kind[r];
            n[0] += kind[r] == 1;
            n[1] += kind[r] == 2 && slack[r] > 0;
        }
    }
    if (tid == 0 && t0 + TB_TILE < p.n_steps) { // the step after the tile: only whether it is joined by 1, which needs no search
        const uint64_t j = t0 + TB_TILE;
        const uint32_t hU = p.unitig[j];
        uint64_t sl;
        bool w = false; // its own tile reports it
        const uint32_t k = join_before_search(p, s.U[TB_TILE], s.endp[TB_TILE], s.rem[TB_TILE], s.iend[TB_TILE], s.wrap[TB_TILE] != 0, hU, p.pos[j], p.item[j],
                                              p.circular[hU >> 1] != 0, s.start[TB_TILE + 1] != 0, &sl, &w);
        s.join[TB_TILE + 1] = (uint8_t)(k == 1);
    }
    __syncthreads();
    auto valid = [&](int i) { return t0 + (i - 1) < p.n_steps; };
    run_count_end(
        ws.run, t0, p.n_steps, [&](int, int i) { return valid(i) && s.join[i] != 1; }, [&](int, int i) { return valid(i) && s.join[i + 1] != 1; },
        [&] { return s.join[1] == 1; });
    block_add(n, totals);
    if (wrong) atomicOr(bad, 1u);
}

struct BridgeOut {
    uint32_t *unitig, *pos, *count, *item, *flags, *start, *end, *matched;
};

__global__ __launch_bounds__(TB_THREADS) void bridge_write_kernel(BridgeIn p, BridgeOut io, BridgeWs ws) {
    __shared__ uint4 stage4[(TB_TILE + 2 * STAGE_PAD) / 4]; // TB_TILE 32-bit elements, and a run's shift
    const int tid = threadIdx.x;
    RunTile rt;
    if (!run_tile(ws.run, p.n_steps, rt)) return;
    const uint64_t t0 = rt.t0;
    uint64_t hd[TB_Q];
    uint32_t opos[TB_Q], ocnt[TB_Q], edge = 0; // edge: the run's head was entered across an edge
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hd[r] = 0, opos[r] = ocnt[r] = 0;
        if ((rt.tkeep >> r) & 1u) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t h = rt.head_of(r);
            const bool in2 = ws.join[h] == 2, out2 = j + 1 < p.n_steps && ws.join[j + 1] == 2; // a read's first step has join 0
            const uint32_t Uj = p.unitig[j];
            const uint32_t endpos = out2 ? (uint32_t)(p.uni_off[(Uj >> 1) + 1] - p.uni_off[Uj >> 1]) : p.pos[j] + p.count[j];
            hd[r] = h;
            opos[r] = in2 ? 0u : p.pos[h];
            ocnt[r] = endpos - opos[r];
            edge |= (in2 ? 1u : 0u) << r;
        }
    }
    rt.leave_tails(io.unitig, stage4, [&](int r, uint64_t) { return p.unitig[hd[r]]; });
    rt.leave_tails(io.pos, stage4, [&](int r, uint64_t) { return opos[r]; });
    rt.leave_tails(io.count, stage4, [&](int r, uint64_t) { return ocnt[r]; });
    rt.leave_tails(io.item, stage4, [&](int r, uint64_t) { return p.item[hd[r]]; });
    rt.leave_tails(io.flags, stage4, [&](int r, uint64_t) { return p.flags[hd[r]] | (((edge >> r) & 1u) ? S2K_STEP_LINKED : 0u); });
    rt.leave_tails(io.start, stage4, [&](int r, uint64_t) { return p.start[hd[r]]; });
    rt.leave_tails(io.end, stage4, [&](int, uint64_t j) { return p.end[j]; });
    rt.leave_tails(io.matched, stage4, [&](int r, uint64_t j) { return ws.C[j + 1] - ws.C[hd[r]]; });
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_paths_bridge(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off, const uint32_t *d_dst,
                            uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular, uint64_t n_unitigs, uint32_t max_gap, uint32_t max_slip,
                            const s2k_thread_out *out, uint32_t *d_matched, uint8_t *d_join, uint64_t *n_out_steps, uint64_t *n_merged, uint64_t *n_bridged) {
    if (n_out_steps) *n_out_steps = 0;
    if (n_merged) *n_merged = 0;
    if (n_bridged) *n_bridged = 0;
    if (!ctx || !out || !n_out_steps || !n_merged || !n_bridged || !paths_given(paths, n_steps, true) || !out->path_off) return S2K_ERR_INVALID_ARG;
    if (n_steps && ((out->start && !paths->start) || (out->end && !paths->end))) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_paths_bridge");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^32 edges or more (an edge index is 32-bit)");
    if (n_unitigs == 0 && n_edges) return c.invalid("edges without unitigs");
    if (n_unitigs && (!d_row_off || !d_uni_off || !d_circular || (n_edges && !d_dst))) return S2K_ERR_INVALID_ARG;
    const uint64_t nt = (n_steps + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many steps for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto words = L.bytes<unsigned long long>(64); // merged, bridged; then the flag
    const auto join = L.take<uint8_t>(n_steps);
    const auto C = L.take<uint64_t>(n_steps + 1);
    const auto stmp = L.bytes<uint64_t>(scan_tmp_bytes(n_steps));
    const auto runs = carve_runs(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 2);
    const BridgeWs ws{join(w), C(w), runs(w)};
    const BridgeIn p{paths->path_off, paths->unitig, paths->pos, paths->count, paths->item, paths->flags, paths->start, paths->end,
                     d_uni_off,       d_circular,    n_reads,    n_steps,      n_unitigs,   max_gap,      max_slip};
    const Csr g{d_row_off, d_dst};
    uint32_t hbad = c.check(totals, 32, bad, [&] {
        hipLaunchKernelGGL(bridge_check_kernel, dim3(grid_for(std::max(std::max(n_reads + 1, n_steps), 2 * n_unitigs))), dim3(UT), 0, c.st, p, g, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    const char *refusal = "path_off that does not run from 0 to n_steps without decreasing, a step on a unitig >= n_unitigs, without items or outside its "
                          "unitig, items of a read that overlap or go backwards, not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * "
                          "n_unitigs, uni_off that does not ascend strictly, or a unitig of 2^32 members or more";
    if (hbad) return c.invalid(refusal);
    if (n_steps == 0) { // no steps: none come out
        c.zero(out->path_off, (n_reads + 1) * 8);
        if (!c.sync()) return c.device_error();
        return S2K_OK;
    }
    uint64_t total = 0;
    unsigned long long h[2] = {0, 0};
    if (!count_runs(c, ws.run, nt, runs.h.scan_tmp(w), [&] { hipLaunchKernelGGL(bridge_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, ws, totals, bad); },
                    &total, totals, h, 2, bad, &hbad))
        return c.device_error();
    if (hbad) return c.invalid(refusal);
    *n_out_steps = total;
    *n_merged = h[0];
    *n_bridged = h[1];
    const bool records = out->unitig || out->pos || out->count || out->item || out->flags || out->start || out->end || d_matched;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (d_join) c.copy(d_join, ws.join, n_steps, hipMemcpyDeviceToDevice);
    launch_run_offsets(c, paths->path_off, n_reads, n_steps, nt, ws.run, out->path_off);
    if (records) {
        if (d_matched) c.scan(paths->count, n_steps, ws.C, stmp(w));
        const BridgeOut io{out->unitig, out->pos, out->count, out->item, out->flags, out->start, out->end, d_matched};
        if (c.ok()) {
            hipLaunchKernelGGL(bridge_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, io, ws);
            c.launched();
        }
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

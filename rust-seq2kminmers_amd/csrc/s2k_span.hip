// s2k_span.hip -- what the read paths say about the junctions of the unitig graph: the reads that traverse a unitig from an in-edge to
// an out-edge (spans), and the repeat unitigs those pairings resolve (include/s2k.h: s2k_paths_spans, s2k_graph_resolve_mask;
// DESIGN.md §3.14).
//
// s2k_paths_spans, the stable stream compaction of s2k_compact_dev.h over the steps, tiles of TB_TILE steps (lane tid holds steps
// r * 256 + tid):
//  1. spans_check_kernel: path_off_ok (s2k_span_dev.h); every step's unitig < 2 T; the CSR rules of simplify_check_kernel; uni_off
//     strictly ascending.  One flag word, read by the host before anything is written; every read is
//     clamped to the arrays whatever they hold.
//  2. spans_count_kernel (follow_tile of s2k_span_dev.h, shared with the walks of s2k_walk.hip): per step its unitig, "ends at its unitig's last member" and "starts a read" to LDS, with one halo step on
//     either side; the read starts in [t0, t0 + TB_TILE] are marked from the reads a binary search of path_off finds there.  The edge a
//     step follows: a binary search of the row of the step before it, the row bounds of all TB_Q steps loaded before the first probe,
//     the TB_Q searches side by side; the index (SP_NONE: none) goes to workspace and to LDS.  Step s spans iff it and step s + 1
//     follow an edge and it covers its whole unitig: one ballot per 64 steps, per word the spans before it inside the tile, per tile
//     the total.  Followed and off-graph steps: a block sum, one integer atomic per block and total.
//  3. launch_scan_u32 over the spans per tile; keys = 2 * spans.
//  4. spans_support_kernel (d_edge_support given; after the capacity decision, so that a refused call adds nothing): one lane per step,
//     one 64-bit integer atomic for the followed edge and one for its twin, found by a search of one row.
//  5. spans_write_kernel: a = the edge of step s, b = that of s + 1, both from workspace; tw(a) and tw(b) by two row searches; the
//     two keys staged in LDS at twice the span's slot, the run leaves with leave_run.
//
// s2k_graph_resolve_mask, one lane per oriented unitig V:
//  1. resolve_check_kernel: the CSR rules; span keys strictly ascending, both halves < n_edges, the out half in the row of the unitig
//     the in half enters.
//  2. resolve_mask_kernel: the in-edges of V are the twins of the row of V ^ 1 (one row search each); the spans of an in-edge are one
//     range of the span keys (one binary search); the lane counts the supported ones and compares the matched out-edges of every two
//     in-edges (quadratic in a hub's degree: slow, never wrong).  Lanes 2 j and 2 j + 1 hold V and V ^ 1: the unitig's verdict is one
//     lane exchange.  d_partner is filled with 0xFF bytes first; a resolved lane writes the entries of its in-edges.
//
// Workspace (the context's grow-only count workspace): spans 4 B per step, 8 B + 4 B per 64 steps, 4 B + 8 B per tile, 64 B; the
// resolution 32 B.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_span_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

// ---- spans -----------------------------------------------------------------------------------------------------------------------
struct SpanWs {
    uint32_t *edge; // per step: the index of the edge it follows, SP_NONE when none
    CompactWs c;    // the span mask
};

__global__ __launch_bounds__(UT) void spans_check_kernel(Paths p, Csr g, const uint64_t *__restrict__ uni_off, uint64_t n_ids, uint64_t n_edges,
                                                         uint32_t *__restrict__ bad) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(p.path_off, p.n_reads, p.n_steps, i0, stride);
    for (uint64_t s = i0; s < p.n_steps; s += stride) // of a step only its unitig: less than steps_ok asks
        if (p.unitig[s] >= n_ids) ok = false;
    for (uint64_t u = i0; u < n_ids; u += stride) {
        if (!(u & 1) && uni_off[u >> 1] >= uni_off[(u >> 1) + 1]) ok = false;
        if (!csr_ids_ok(g.row_off, g.dst, u, n_ids, n_edges)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(TB_THREADS) void spans_count_kernel(Paths p, Csr g, const uint64_t *__restrict__ uni_off, SpanWs ws,
                                                                 unsigned long long *__restrict__ totals /* followed, off-graph */) {
    __shared__ FollowLds s;
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint32_t U[TB_Q], ps[TB_Q], cnt[TB_Q], fl[TB_Q], e[TB_Q];
    uint64_t len[TB_Q];
    follow_tile(p, g, uni_off, t0, s, U, ps, cnt, fl, len, e);
    uint32_t n[2] = {0, 0}; // followed, off-graph
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        if (j < p.n_steps) {
            ws.edge[j] = e[r];
            n[0] += e[r] != SP_NONE;
            n[1] += (fl[r] & S2K_STEP_LINKED) && e[r] == SP_NONE;
        }
    }
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        const bool whole = t0 + (i - 1) < p.n_steps && cnt[r] == len[r];
        tile_ballot(wc, r, t0, p.n_steps, ws.c, whole && s.E[i] != SP_NONE && s.E[i + 1] != SP_NONE);
    }
    __syncthreads();
    tile_prefixes(wc, t0, p.n_steps, ws.c);
    block_add(n, totals);
}

__global__ __launch_bounds__(UT) void spans_support_kernel(Paths p, Csr g, const uint32_t *__restrict__ edge, unsigned long long *__restrict__ support) {
    for (uint64_t s = (uint64_t)blockIdx.x * UT + threadIdx.x; s < p.n_steps; s += (uint64_t)gridDim.x * UT) {
        const uint32_t e = edge[s];
        if (e == SP_NONE) continue; // a step that follows an edge has a step before it
        atomicAdd(support + e, 1ull);
        const uint32_t tw = find_edge(g, p.unitig[s] ^ 1u, p.unitig[s - 1] ^ 1u);
        if (tw != e && tw != SP_NONE) atomicAdd(support + tw, 1ull); // a hairpin is its own twin: counted once
    }
}

__global__ __launch_bounds__(TB_THREADS) void spans_write_kernel(Paths p, Csr g, SpanWs ws, uint64_t *__restrict__ keys) {
    __shared__ uint4 stage[(2 * TB_TILE + STAGE_PAD) / 2];
    uint64_t *s64 = (uint64_t *)stage;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t base = 2 * ws.c.tile_off[blockIdx.x];
    const uint32_t tot = 2 * (uint32_t)(ws.c.tile_off[blockIdx.x + 1] - ws.c.tile_off[blockIdx.x]);
    if (tot == 0) return;
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ws.c, t0, p.n_steps, slot);
    const uint32_t sh = shift_of(keys + base);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if ((keep >> r) & 1u) { // a span: steps j - 1, j and j + 1 exist and lie in one read
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t a = ws.edge[j], b = ws.edge[j + 1];
            const uint32_t A = p.unitig[j - 1], V = p.unitig[j], C = p.unitig[j + 1];
            const uint64_t ta = find_edge(g, V ^ 1u, A ^ 1u), tb = find_edge(g, C ^ 1u, V ^ 1u);
            s64[sh + 2 * slot[r]] = a << 32 | b;
            s64[sh + 2 * slot[r] + 1] = tb << 32 | ta;
        }
    __syncthreads();
    leave_run(keys + base, s64, sh, tot);
}

// ---- resolution ------------------------------------------------------------------------------------------------------------------
struct Spans {
    const uint64_t *keys;
    const uint32_t *counts;
    uint64_t n;
    uint32_t min_support;
};

__global__ __launch_bounds__(UT) void resolve_check_kernel(Csr g, uint64_t n_ids, uint64_t n_edges, Spans sp, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t u = i0; u < n_ids; u += stride)
        if (!csr_ids_ok(g.row_off, g.dst, u, n_ids, n_edges)) ok = false;
    for (uint64_t i = i0; i < sp.n; i += stride) {
        const uint64_t k = sp.keys[i], a = k >> 32, b = k & 0xFFFFFFFFull;
        if (i && sp.keys[i - 1] >= k) ok = false;
        if (a >= n_edges || b >= n_edges) {
            ok = false;
            continue;
        }
        const uint64_t V = g.dst[a];
        if (V >= n_ids || b < g.row_off[V] || b >= g.row_off[V + 1]) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

// the one out-edge that in-edge a is paired with by a supported span, SP_NONE when there is none or more than one
__device__ __forceinline__ uint32_t matched_out(const Spans &sp, uint32_t a) {
    const uint64_t first = (uint64_t)a << 32;
    uint64_t lo = 0, hi = sp.n; // the first key >= a << 32
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sp.keys[mid] < first) lo = mid + 1;
        else hi = mid;
    }
    uint32_t b = SP_NONE, n = 0;
    for (uint64_t i = lo; i < sp.n && (sp.keys[i] >> 32) == a; i++)
        if (sp.counts[i] >= sp.min_support) {
            b = (uint32_t)sp.keys[i];
            n++;
        }
    return n == 1 ? b : SP_NONE;
}

// in-edge number f - row_off[V ^ 1] of V: the twin of edge f of the row of V ^ 1
__device__ __forceinline__ uint32_t in_edge(const Csr &g, uint32_t V, uint64_t f) { return find_edge(g, g.dst[f] ^ 1u, V); }

__device__ __forceinline__ bool resolved_strand(const Csr &g, const Spans &sp, uint32_t V, bool *candidate) {
    const uint64_t ia = g.row_off[V ^ 1u], ib = g.row_off[(V ^ 1u) + 1], oa = g.row_off[V], ob = g.row_off[V + 1];
    *candidate = ib - ia >= 2 && ob - oa >= 2;
    if (!*candidate || ib - ia != ob - oa) return false;
    for (uint64_t f = ia; f < ib; f++)
        if ((g.dst[f] >> 1) == (V >> 1)) return false; // a predecessor of V's own unitig
    for (uint64_t f = oa; f < ob; f++)
        if ((g.dst[f] >> 1) == (V >> 1)) return false;
    for (uint64_t f = ia; f < ib; f++) { // every in-edge has one supported out-edge, and no two in-edges the same one: with in == out
        const uint32_t a = in_edge(g, V, f); // a perfect matching
        if (a == SP_NONE) return false;
        const uint32_t b = matched_out(sp, a);
        if (b == SP_NONE) return false;
        for (uint64_t h = ia; h < f; h++)
            if (matched_out(sp, in_edge(g, V, h)) == b) return false;
    }
    return true;
}

__global__ __launch_bounds__(UT) void resolve_mask_kernel(Csr g, uint64_t n_ids, Spans sp, uint8_t *__restrict__ resolved, uint32_t *__restrict__ partner,
                                                          unsigned long long *__restrict__ totals /* candidates, resolved */) {
    uint32_t n[2] = {0, 0};
    // n_ids is even and the stride a multiple of 64: lanes 2 j and 2 j + 1 of a wave hold V and V ^ 1, both in range or neither
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        const uint32_t V = (uint32_t)u;
        bool cand;
        uint32_t ok = resolved_strand(g, sp, V, &cand) ? 1u : 0u;
        ok &= __shfl_xor(ok, 1, 64); // the verdict on the unitig: both strands
        if (!(V & 1u)) {
            n[0] += cand;
            n[1] += ok;
            if (resolved) resolved[V >> 1] = (uint8_t)ok;
        }
        if (ok && partner) // every edge enters one oriented unitig: one writer per entry
            for (uint64_t f = g.row_off[V ^ 1u]; f < g.row_off[(V ^ 1u) + 1]; f++) {
                const uint32_t a = in_edge(g, V, f);
                partner[a] = matched_out(sp, a);
            }
    }
    block_add(n, totals);
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_paths_spans(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off,
                           const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, uint64_t n_unitigs, uint64_t *d_span_keys,
                           uint64_t capacity, uint64_t *d_edge_support, uint64_t *n_keys, uint64_t *n_followed, uint64_t *n_off_graph) {
    if (n_keys) *n_keys = 0;
    if (n_followed) *n_followed = 0;
    if (n_off_graph) *n_off_graph = 0;
    if (!ctx || !n_keys || !n_followed || !n_off_graph || !paths_given(paths, n_steps, false)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_paths_spans");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^32 edges or more (a span key holds two edge indices)");
    if (n_unitigs == 0 && n_edges) return c.invalid("edges without unitigs");
    if (n_unitigs && (!d_row_off || !d_uni_off || (n_edges && !d_dst))) return S2K_ERR_INVALID_ARG;
    const uint64_t nt = (n_steps + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many steps for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto words = L.bytes<unsigned long long>(64); // followed, off-graph; then the check's flag
    const auto edge = L.take<uint32_t>(n_steps);
    const auto cw = carve(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 2);
    const SpanWs ws{edge(w), cw(w)};
    const Paths p = paths_of(paths, n_reads, n_steps);
    const Csr g{d_row_off, d_dst};
    const uint64_t n_ids = 2 * n_unitigs;
    const uint32_t hbad = c.check(totals, 32, bad, [&] {
        hipLaunchKernelGGL(spans_check_kernel, dim3(grid_for(std::max(std::max(n_reads + 1, n_steps), n_ids))), dim3(UT), 0, c.st, p, g, d_uni_off,
                           n_ids, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("path_off that does not run from 0 to n_steps without decreasing, a step on a unitig >= n_unitigs, not a CSR of "
                         "2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, or a unitig without a member");
    if (n_steps == 0) return S2K_OK;
    uint64_t spans = 0;
    unsigned long long h[2] = {0, 0};
    hipLaunchKernelGGL(spans_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, d_uni_off, ws, totals);
    c.launched();
    c.scan(ws.c.tile_kept, nt, ws.c.tile_off, cw.scan_tmp(w));
    c.fetch(&spans, ws.c.tile_off + nt, 8);
    c.fetch(h, totals, sizeof(h));
    if (!c.sync()) return c.device_error();
    *n_keys = 2 * spans;
    *n_followed = h[0];
    *n_off_graph = h[1];
    if (d_span_keys && *n_keys > capacity) return S2K_ERR_CAPACITY;
    if (d_edge_support && h[0]) {
        hipLaunchKernelGGL(spans_support_kernel, dim3(grid_for(n_steps)), dim3(UT), 0, c.st, p, g, ws.edge, (unsigned long long *)d_edge_support);
        c.launched();
    }
    if (d_span_keys && spans) {
        hipLaunchKernelGGL(spans_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, ws, d_span_keys);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_graph_resolve_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                  const uint64_t *d_span_keys, const uint32_t *d_span_counts, uint64_t n_spans, uint32_t min_support,
                                  uint8_t *d_resolved, uint32_t *d_partner, uint64_t *n_candidates, uint64_t *n_resolved) {
    if (n_candidates) *n_candidates = 0;
    if (n_resolved) *n_resolved = 0;
    if (!ctx || !n_candidates || !n_resolved) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_resolve_mask");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^32 edges or more (a span key holds two edge indices)");
    if (n_unitigs == 0) return n_edges == 0 && n_spans == 0 ? S2K_OK : c.invalid("edges or spans without unitigs");
    if (!d_row_off || (n_edges && !d_dst) || (n_spans && (!d_span_keys || !d_span_counts))) return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    unsigned long long *w = (unsigned long long *)ctx_count_table(ctx, 256);
    if (!w) return c.nomem();
    unsigned long long *totals = w; // candidates, resolved; then the check's flag
    uint32_t *bad = (uint32_t *)(w + 2);
    const uint64_t n_ids = 2 * n_unitigs;
    const Csr g{d_row_off, d_dst};
    const Spans sp{d_span_keys, d_span_counts, n_spans, min_support ? min_support : 1u};
    const uint32_t hbad = c.check(w, 32, bad, [&] {
        hipLaunchKernelGGL(resolve_check_kernel, dim3(grid_for(std::max(n_ids, n_spans))), dim3(UT), 0, c.st, g, n_ids, n_edges, sp, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, span keys that do not ascend strictly, "
                         "an edge index >= n_edges, or an out-edge that does not leave the unitig its in-edge enters");
    if (d_partner && n_edges) c.fill(d_partner, 0xFF, n_edges * 4);
    unsigned long long h[2] = {0, 0};
    hipLaunchKernelGGL(resolve_mask_kernel, dim3(grid_for(n_ids)), dim3(UT), 0, c.st, g, n_ids, sp, d_resolved, d_partner, totals);
    c.launched();
    c.fetch(h, totals, sizeof(h));
    if (!c.sync()) return c.device_error();
    *n_candidates = h[0];
    *n_resolved = h[1];
    return S2K_OK;
}

} // extern "C"

// s2k_bubble.hip -- one round of bounded superbubble popping on the unitig graph (include/s2k.h: s2k_graph_bubble_mask;
// DESIGN.md §3.24).
//
//  1. bubble_check_kernel, tiles of TB_TILE oriented unitigs: the check of s2k_graph_simplify_mask (csr_ids_ok, uni_off strictly
//     ascending; one flag word, read by the host before anything is written) and, in the same pass, the ballot "out(U) >= 2" of the
//     stable compaction of s2k_compact_dev.h.  launch_scan_u32 over the tile totals; the host reads the flag and the number of sources.
//  2. bubble_sources_kernel: the sources, ascending, from tile_slots.
//  3. bubble_kernel<false>, one wave per source in a bounded grid (at most S2K_BUBBLE_WAVES waves, a wave takes sources w, w + waves,
//     ...): the traversal of the header with lane i holding slot i of the list -- id, r, best, bp in registers -- so "is W in the list"
//     and "is W ^ 1 in the list" are one ballot each, the ready set is a ballot and its lowest bit the entry to expand.  A row is
//     loaded 64 entries at a time, one per lane, and walked entry by entry in row order (a row adds at most max_nodes + 2 entries to
//     the list before the traversal fails: a hub is slow, never wrong).  found[i] = the source has a bubble with something to
//     remove; its interior lanes claim owner[id >> 1] with one atomicMin each.
//  4. bubble_kernel<true>: the sources with found[i] run the same traversal again (it is a function of the input: the same list in
//     the same slots) and apply the bubble when every interior lane reads its own source from owner; the removable lanes set
//     remove[id >> 1].  Nothing of a source's list is kept between the two passes: a list is 64 slots of 4 B, and the second
//     traversal reads what the first left in L2.
// The totals are integer sums: per wave in lane 0, one block_add per block.
//
// Workspace (the context's grow-only count workspace): 64 B of totals and flag, the compaction's 0.2 B per oriented unitig, 4 B per
// oriented unitig for the sources, 1 B per oriented unitig for found, 4 B per unitig for owner: 14.4 B per unitig.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

static_assert(S2K_BUBBLE_MAX_NODES + 2 == 64, "one lane per list slot: S, T and the interior");
static_assert(S2K_BUBBLE_WAVES % (UT / 64) == 0, "whole blocks");

struct BGraph {
    const uint64_t *row_off;
    const uint32_t *dst;
    const uint64_t *uni_off, *cnt;
    uint32_t cap; // max_nodes + 2 list entries
    uint64_t max_bubble;
};

__global__ __launch_bounds__(TB_THREADS) void bubble_check_kernel(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst,
                                                                  const uint64_t *__restrict__ uni_off, uint64_t n_ids, uint64_t n_edges,
                                                                  CompactWs ws, uint32_t *__restrict__ bad) {
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    bool ok = true;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t u = t0 + (uint64_t)r * TB_THREADS + tid;
        bool src = false;
        if (u < n_ids) {
            if (!(u & 1) && uni_off[u >> 1] >= uni_off[(u >> 1) + 1]) ok = false;
            if (!csr_ids_ok(row_off, dst, u, n_ids, n_edges)) ok = false;
            src = row_off[u + 1] - row_off[u] >= 2; // (of a refused input: never used)
        }
        tile_ballot(wc, r, t0, n_ids, ws, src);
    }
    if (!ok) atomicOr(bad, 1u);
    __syncthreads();
    tile_prefixes(wc, t0, n_ids, ws);
}

__global__ __launch_bounds__(TB_THREADS) void bubble_sources_kernel(uint64_t n_ids, CompactWs ws, uint32_t *__restrict__ sources) {
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t base = ws.tile_off[blockIdx.x];
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ws, t0, n_ids, slot);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if ((keep >> r) & 1u) sources[base + slot[r]] = (uint32_t)(t0 + (uint64_t)r * TB_THREADS + threadIdx.x);
}

__device__ __forceinline__ int low_bit(uint64_t m) { return __ffsll((unsigned long long)m) - 1; }

// The traversal from S by the whole wave, lane i = slot i of the list.  true: S has a bubble with a non-empty removable set; then
// *id = this lane's entry and the two masks tell the slots of the interior and of the removable set.  Every branch is wave-uniform.
__device__ __forceinline__ bool traverse(const BGraph &g, uint32_t S, uint32_t *id_out, uint64_t *interior_out, uint64_t *removable_out) {
    const int lane = threadIdx.x & 63;
    uint32_t id = lane == 0 ? S : NONE, r = 0, bp = NONE; // of slot `lane`, once lane < n
    uint64_t best = 0;
    uint32_t n = 1;        // entries in the list
    uint64_t expanded = 0; // their slots
    int tslot;
    for (;;) {
        const uint64_t live = n == 64 ? ~0ull : (1ull << n) - 1ull;
        const uint64_t ready = __ballot(r == 0) & live & ~expanded;
        if (expanded && __popcll(ready) == 1 && (live & ~expanded) == ready) { // one entry ready, every other one expanded
            tslot = low_bit(ready);
            break;
        }
        if (!ready) return false; // an entry waits for an in-edge from outside
        const int e = low_bit(ready);
        expanded |= 1ull << e;
        const uint32_t V = __shfl(id, e, 64);
        const uint64_t a = g.row_off[V], b = g.row_off[(uint64_t)V + 1];
        if (a == b) return false; // a dead end inside
        const uint64_t vb = __shfl(best, e, 64) + (e ? g.cnt[V >> 1] : 0ull);
        for (uint64_t c0 = a; c0 < b; c0 += 64) {
            const uint32_t mine = c0 + lane < b ? g.dst[c0 + lane] : 0u;
            const int m = (int)std::min<uint64_t>(64, b - c0);
            for (int j = 0; j < m; j++) {
                const uint32_t W = __shfl(mine, j, 64);
                if ((W >> 1) == (S >> 1)) return false; // a cycle or a hairpin back
                const uint64_t lv = n == 64 ? ~0ull : (1ull << n) - 1ull;
                if (__ballot(id == (W ^ 1u)) & lv) return false; // an inversion
                const uint64_t at = __ballot(id == W) & lv;
                if (!at) {
                    if (n == g.cap) return false; // the list would exceed max_nodes + 2 entries
                    const uint64_t in = g.row_off[(uint64_t)(W ^ 1u) + 1] - g.row_off[W ^ 1u];
                    if (in == 0) return false; // an edge into an entry without in-edges: not twin-symmetric
                    if (lane == (int)n) {
                        id = W;
                        r = (uint32_t)std::min<uint64_t>(in, 0xFFFFFFFFull) - 1u;
                        best = vb;
                        bp = V;
                    }
                    n++;
                } else {
                    const int s = low_bit(at);
                    if (__shfl(r, s, 64) == 0) return false; // more edges into it than in(W): not twin-symmetric
                    if (lane == s) {
                        r--;
                        if (vb > best || (vb == best && V < bp)) best = vb, bp = V;
                    }
                }
            }
        }
    }
    const uint64_t live = n == 64 ? ~0ull : (1ull << n) - 1ull;
    const uint64_t interior = live & ~1ull & ~(1ull << tslot);
    if (!interior) return false;
    const bool inside = (interior >> lane) & 1ull;
    uint64_t len = inside ? g.uni_off[(id >> 1) + 1] - g.uni_off[id >> 1] : 0ull;
    for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o, 64);
    if (len > g.max_bubble) return false;
    uint64_t kept = 0; // the slots of the kept path: bp from T back to S (an entry's bp was expanded before it)
    int cur = tslot;
    for (uint32_t k = 0; k < n && cur != 0; k++) {
        const uint32_t p = __shfl(bp, cur, 64);
        cur = low_bit(__ballot(id == p) & live);
        kept |= 1ull << cur;
    }
    *id_out = id;
    *interior_out = interior;
    *removable_out = interior & ~kept;
    return (interior & ~kept) != 0;
}

// APPLY false: found[i] and the claims; totals[0] += bubbles found.  APPLY true: the bubbles that own their interior set remove[];
// totals[1] += bubbles applied, totals[2] += unitigs removed.
template <bool APPLY>
__global__ __launch_bounds__(UT) void bubble_kernel(BGraph g, const uint32_t *__restrict__ sources, uint64_t n_sources, uint8_t *__restrict__ found,
                                                    uint32_t *__restrict__ owner, uint8_t *__restrict__ remove,
                                                    unsigned long long *__restrict__ totals /* found, applied, removed */) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (UT / 64) + (threadIdx.x >> 6)), stride = gridDim.x * (UT / 64);
    unsigned long long n[3] = {0, 0, 0};
    for (uint64_t i = wave; i < n_sources; i += stride) {
        if (APPLY && !found[i]) continue;
        const uint32_t S = sources[i];
        uint32_t id = NONE;
        uint64_t interior = 0, removable = 0;
        const bool ok = traverse(g, S, &id, &interior, &removable);
        const bool inside = ok && ((interior >> lane) & 1ull);
        if (!APPLY) {
            if (lane == 0) found[i] = ok, n[0] += ok;
            if (inside) atomicMin(owner + (id >> 1), S);
        } else {
            const bool other = inside && owner[id >> 1] != S;
            if (ok && !__any(other)) {
                if (remove && ((removable >> lane) & 1ull)) remove[id >> 1] = 1;
                if (lane == 0) n[1]++, n[2] += __popcll(removable);
            }
        }
    }
    block_add(n, totals);
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_graph_bubble_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                 const uint64_t *d_uni_off, const uint64_t *d_uni_count, uint32_t max_nodes, uint32_t max_bubble,
                                 uint8_t *d_remove, uint64_t *n_sources, uint64_t *n_found, uint64_t *n_applied, uint64_t *n_removed) {
    if (n_sources) *n_sources = 0;
    if (n_found) *n_found = 0;
    if (n_applied) *n_applied = 0;
    if (n_removed) *n_removed = 0;
    if (!ctx || !n_sources || !n_found || !n_applied || !n_removed) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_bubble_mask");
    if (max_nodes == 0 || max_nodes > S2K_BUBBLE_MAX_NODES) return c.invalid("max_nodes is 0 or above S2K_BUBBLE_MAX_NODES");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 40))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^40 edges or more");
    if (n_unitigs == 0) return n_edges == 0 ? S2K_OK : c.invalid("edges without unitigs");
    if (!d_row_off || !d_uni_off || !d_uni_count || (n_edges && !d_dst)) return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const uint64_t n_ids = 2 * n_unitigs, n_tiles = (n_ids + TB_TILE - 1) / TB_TILE;
    Layout L;
    const auto words = L.bytes<unsigned long long>(64); // found, applied, removed; then the check's flag
    const auto src_ws = carve(L, n_ids, n_tiles);
    const auto sources_p = L.take<uint32_t>(n_ids);
    const auto found_p = L.take<uint8_t>(n_ids);
    const auto owner_p = L.take<uint32_t>(n_unitigs);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 3);
    const CompactWs sw = src_ws(w);
    uint64_t ns = 0;
    const uint32_t hbad = c.check(totals, 64, bad, [&] {
        hipLaunchKernelGGL(bubble_check_kernel, dim3((unsigned)n_tiles), dim3(TB_THREADS), 0, c.st, d_row_off, d_dst, d_uni_off, n_ids, n_edges, sw, bad);
        c.launched();
        c.scan(sw.tile_kept, n_tiles, sw.tile_off, src_ws.scan_tmp(w));
        c.fetch(&ns, sw.tile_off + n_tiles, 8);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, or a unitig without a member");
    unsigned long long h[3] = {0, 0, 0};
    if (d_remove) c.zero(d_remove, n_unitigs);
    if (ns) {
        const BGraph g{d_row_off, d_dst, d_uni_off, d_uni_count, max_nodes + 2, max_bubble};
        const unsigned blocks = (unsigned)((std::min<uint64_t>(ns, S2K_BUBBLE_WAVES) + UT / 64 - 1) / (UT / 64));
        c.fill(owner_p(w), 0xFF, n_unitigs * 4); // no source: every id is below it
        c.launch(bubble_sources_kernel, (unsigned)n_tiles, TB_THREADS, n_ids, sw, sources_p(w));
        c.launch(bubble_kernel<false>, blocks, UT, g, (const uint32_t *)sources_p(w), ns, found_p(w), owner_p(w), d_remove, totals);
        c.launch(bubble_kernel<true>, blocks, UT, g, (const uint32_t *)sources_p(w), ns, found_p(w), owner_p(w), d_remove, totals);
        c.fetch(h, totals, sizeof(h));
    }
    if (!c.sync()) return c.device_error();
    *n_sources = ns;
    *n_found = h[0];
    *n_applied = h[1];
    *n_removed = h[2];
    return S2K_OK;
}

} // extern "C"

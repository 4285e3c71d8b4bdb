// s2k_simplify.hip -- one round of graph simplification on the unitig graph, and the subgraph the kept nodes induce
// (include/s2k.h: s2k_graph_simplify_mask, s2k_graph_induced).
//
// s2k_graph_simplify_mask, one lane per oriented unitig U = 2 t + s:
//  1. simplify_check_kernel: row_off[0] == 0, non-decreasing, row_off[2 T] == n_edges, every id < 2 T; the even lane also checks
//     uni_off[t] < uni_off[t + 1].  One flag word, read by the host before anything is written.  Every read is clamped to the arrays
//     whatever they hold.
//  2. simplify_mask_kernel: the tip rule and the bubble rule of the header for U, each a walk over the rows at U's junctions (short:
//     a hub is slow, never wrong).  Lanes 2 j and 2 j + 1 of a wave hold U and U ^ 1, so the unitig's verdict is one lane exchange;
//     the even lane writes remove[t].  The three totals: a block sum, then one integer atomic per block on a workspace word.
//     "W beats U" compares cnt[W] * len[U] with cnt[U] * len[W] as 128-bit products (__umul64hi and the low product).
//
// s2k_graph_induced, the stable stream compaction of s2k_compact_dev.h applied to two streams, tiles of TB_TILE items (lane tid
// holds items r * 256 + tid):
//  1. node_count_kernel: keep[i] from d_node_keep, or gathered as !remove[node_unitig[i]]; per 64 nodes the kept mask (one wave's
//     ballot) and the kept nodes before that word inside its tile; per tile the kept total.
//  2. edge_count_kernel: an edge is kept iff the kept bits of both its nodes are set (two gathers from the node masks, 1 bit per
//     node); the same three outputs per word / tile.  A node id >= n_nodes sets the flag word.
//  3. launch_scan_u32 over the tile totals of either stream; the host reads both totals and the flag.
//  4. node_write_kernel: new_id for every node of the tile, coalesced; kept keys, then kept counts, staged in LDS at their
//     tile-relative slots and written as one contiguous run.  edge_write_kernel: the same for the edges, the new key from two gathers
//     of new_id -- the only dependent loads.
// A run leaves LDS in 16-byte pieces: the tile is staged `shift` elements in, shift = the elements between the run's first output
// address and the 16-byte boundary below it, so that LDS and global addresses are aligned alike; the at most two partial pieces at
// the ends go element by element.
//
// Workspace (the context's grow-only count workspace): the mask call 32 B; the induced call per stream 8 B + 4 B per 64 items and
// 4 B + 8 B per tile (0.2 B per item), and 4 B per node for new_id when the caller does not take it.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

// ---- the mask ---------------------------------------------------------------------------------------------------------------------
struct UGraph {
    const uint64_t *row_off;
    const uint32_t *dst;
    const uint64_t *uni_off, *cnt;
    uint64_t max_tip, max_bubble;
};

__device__ __forceinline__ uint64_t out_deg(const UGraph &g, uint32_t U) { return g.row_off[U + 1] - g.row_off[U]; }
__device__ __forceinline__ uint64_t len_of(const UGraph &g, uint32_t U) { return g.uni_off[(U >> 1) + 1] - g.uni_off[U >> 1]; }
__device__ __forceinline__ bool tip_candidate(const UGraph &g, uint32_t U) {
    return out_deg(g, U) == 0 && out_deg(g, U ^ 1u) >= 1 && len_of(g, U) <= g.max_tip;
}
// W beats U (different unitigs): the higher mean count, then more members, then the smaller index
__device__ __forceinline__ bool beats(const UGraph &g, uint32_t W, uint32_t U) {
    const uint64_t cw = g.cnt[W >> 1], cu = g.cnt[U >> 1], lw = len_of(g, W), lu = len_of(g, U);
    const uint64_t ah = __umul64hi(cw, lu), al_ = cw * lu, bh = __umul64hi(cu, lw), bl = cu * lw;
    if (ah != bh) return ah > bh;
    if (al_ != bl) return al_ > bl;
    if (lw != lu) return lw > lu;
    return (W >> 1) < (U >> 1);
}

__device__ __forceinline__ bool removable_tip(const UGraph &g, uint32_t U) {
    if (!tip_candidate(g, U)) return false;
    const uint64_t a = g.row_off[U ^ 1u], b = g.row_off[(U ^ 1u) + 1];
    for (uint64_t e = a; e < b; e++) { // every predecessor P = X ^ 1, X in succ(U ^ 1)
        const uint32_t P = g.dst[e] ^ 1u;
        if ((P >> 1) == (U >> 1)) return false;
        bool alt = false;
        const uint64_t pa = g.row_off[P], pb = g.row_off[P + 1];
        for (uint64_t f = pa; f < pb && !alt; f++) {
            const uint32_t W = g.dst[f];
            if ((W >> 1) == (U >> 1)) continue;
            alt = !tip_candidate(g, W) || beats(g, W, U);
        }
        if (!alt) return false;
    }
    return true;
}

__device__ __forceinline__ bool removable_bubble(const UGraph &g, uint32_t U) {
    if (out_deg(g, U) != 1 || out_deg(g, U ^ 1u) != 1 || len_of(g, U) > g.max_bubble) return false;
    const uint32_t P = g.dst[g.row_off[U ^ 1u]] ^ 1u, S = g.dst[g.row_off[U]];
    if ((P >> 1) == (U >> 1) || (S >> 1) == (U >> 1)) return false;
    const uint64_t pa = g.row_off[P], pb = g.row_off[P + 1];
    for (uint64_t f = pa; f < pb; f++) {
        const uint32_t W = g.dst[f];
        if ((W >> 1) == (U >> 1)) continue;
        if (out_deg(g, W) == 1 && out_deg(g, W ^ 1u) == 1 && g.dst[g.row_off[W]] == S && beats(g, W, U)) return true;
    }
    return false;
}

__global__ __launch_bounds__(UT) void simplify_check_kernel(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst,
                                                            const uint64_t *__restrict__ uni_off, uint64_t n_ids, uint64_t n_edges,
                                                            uint32_t *__restrict__ bad) {
    bool ok = true;
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        if (!(u & 1) && uni_off[u >> 1] >= uni_off[(u >> 1) + 1]) ok = false;
        uint64_t a, b;
        if (!csr_row_ok(row_off, u, n_ids, n_edges, &a, &b)) {
            ok = false;
            continue;
        }
        for (uint64_t e = a; e < b; e++)
            if (dst[e] >= n_ids) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void simplify_mask_kernel(UGraph g, uint64_t n_ids, uint8_t *__restrict__ remove,
                                                           unsigned long long *__restrict__ totals /* tips, bubbles, removed */) {
    uint32_t n[3] = {0, 0, 0}; // tips, bubbles, removed
    // n_ids is even and the stride a multiple of 64: lanes 2 j and 2 j + 1 of a wave hold U and U ^ 1, both in range or neither
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        const uint32_t U = (uint32_t)u;
        uint32_t f = (removable_tip(g, U) ? 1u : 0u) | (removable_bubble(g, U) ? 2u : 0u);
        f |= __shfl_xor(f, 1, 64); // the verdict on the unitig: either strand
        if (!(U & 1u)) {
            n[0] += f & 1u;
            n[1] += (f >> 1) & 1u;
            n[2] += f != 0;
            if (remove) remove[U >> 1] = f != 0;
        }
    }
    block_add(n, totals);
}

// ---- the induced subgraph: two stable stream compactions ---------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void node_count_kernel(const uint8_t *__restrict__ keep, const uint32_t *__restrict__ node_unitig,
                                                                const uint8_t *__restrict__ remove, uint64_t n_unitigs, uint64_t n_nodes,
                                                                CompactWs ws, uint32_t *__restrict__ bad) {
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    bool ok = true;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        bool k = false;
        if (j < n_nodes) {
            if (keep) {
                k = keep[j] != 0;
            } else {
                const uint32_t t = node_unitig[j];
                if (t < n_unitigs) k = remove[t] == 0;
                else ok = false;
            }
        }
        tile_ballot(wc, r, t0, n_nodes, ws, k);
    }
    if (!ok) atomicOr(bad, 1u);
    __syncthreads();
    tile_prefixes(wc, t0, n_nodes, ws);
}

__global__ __launch_bounds__(TB_THREADS) void edge_count_kernel(const uint64_t *__restrict__ edge_keys, uint64_t n_edges, uint64_t n_nodes,
                                                                const uint64_t *__restrict__ node_mask, CompactWs ws, uint32_t *__restrict__ bad) {
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint64_t key[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) key[r] = edge_keys[std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, n_edges - 1)];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        const uint64_t a = key[r] >> 33, b = (key[r] & 0xFFFFFFFFull) >> 1; // the two node indices
        bool k = false;
        if (j < n_edges) {
            if (a < n_nodes && b < n_nodes) k = ((node_mask[a >> 6] >> (a & 63)) & (node_mask[b >> 6] >> (b & 63)) & 1ull) != 0;
            else ok = false;
        }
        tile_ballot(wc, r, t0, n_edges, ws, k);
    }
    if (!ok) atomicOr(bad, 1u);
    __syncthreads();
    tile_prefixes(wc, t0, n_edges, ws);
}

__global__ __launch_bounds__(TB_THREADS) void node_write_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts, uint64_t n_nodes,
                                                                CompactWs ws, uint32_t *__restrict__ new_id, uint64_t *__restrict__ o_keys,
                                                                uint32_t *__restrict__ o_counts) {
    __shared__ uint4 stage[(TB_TILE + STAGE_PAD) / 2];
    uint64_t *s64 = (uint64_t *)stage;
    uint32_t *s32 = (uint32_t *)stage;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t base = ws.tile_off[blockIdx.x];
    const uint32_t tot = (uint32_t)(ws.tile_off[blockIdx.x + 1] - base);
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ws, t0, n_nodes, slot);
    if (new_id) {
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            if (j < n_nodes) new_id[j] = (keep >> r) & 1u ? (uint32_t)(base + slot[r]) : NONE;
        }
    }
    if (tot == 0) return;
    if (o_keys) {
        const uint32_t sh = shift_of(o_keys + base);
#pragma unroll
        for (int r = 0; r < TB_Q; r++)
            if ((keep >> r) & 1u) s64[sh + slot[r]] = keys[t0 + (uint64_t)r * TB_THREADS + tid];
        __syncthreads();
        leave_run(o_keys + base, s64, sh, tot);
    }
    if (o_counts) {
        const uint32_t sh = shift_of(o_counts + base);
#pragma unroll
        for (int r = 0; r < TB_Q; r++)
            if ((keep >> r) & 1u) s32[sh + slot[r]] = counts[t0 + (uint64_t)r * TB_THREADS + tid];
        __syncthreads();
        leave_run(o_counts + base, s32, sh, tot);
    }
}

__global__ __launch_bounds__(TB_THREADS) void edge_write_kernel(const uint64_t *__restrict__ edge_keys, const uint32_t *__restrict__ edge_counts,
                                                                uint64_t n_edges, CompactWs ws, const uint32_t *__restrict__ new_id,
                                                                uint64_t *__restrict__ o_keys, uint32_t *__restrict__ o_counts) {
    __shared__ uint4 stage[(TB_TILE + STAGE_PAD) / 2];
    uint64_t *s64 = (uint64_t *)stage;
    uint32_t *s32 = (uint32_t *)stage;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t base = ws.tile_off[blockIdx.x];
    const uint32_t tot = (uint32_t)(ws.tile_off[blockIdx.x + 1] - base);
    if (tot == 0) return;
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ws, t0, n_edges, slot);
    if (o_keys) {
        const uint32_t sh = shift_of(o_keys + base);
        uint64_t key[TB_Q];
#pragma unroll
        for (int r = 0; r < TB_Q; r++) key[r] = (keep >> r) & 1u ? edge_keys[t0 + (uint64_t)r * TB_THREADS + tid] : 0ull;
#pragma unroll
        for (int r = 0; r < TB_Q; r++)
            if ((keep >> r) & 1u) { // both ends are kept: the count pass saw their bits
                const uint32_t u = (uint32_t)(key[r] >> 32), v = (uint32_t)key[r];
                const uint64_t nu = 2ull * new_id[u >> 1] + (u & 1u), nv = 2ull * new_id[v >> 1] + (v & 1u);
                s64[sh + slot[r]] = nu << 32 | nv;
            }
        __syncthreads();
        leave_run(o_keys + base, s64, sh, tot);
    }
    if (o_counts) {
        const uint32_t sh = shift_of(o_counts + base);
#pragma unroll
        for (int r = 0; r < TB_Q; r++)
            if ((keep >> r) & 1u) s32[sh + slot[r]] = edge_counts[t0 + (uint64_t)r * TB_THREADS + tid];
        __syncthreads();
        leave_run(o_counts + base, s32, sh, tot);
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_graph_simplify_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                   const uint64_t *d_uni_off, const uint64_t *d_uni_count, uint32_t max_tip, uint32_t max_bubble,
                                   uint8_t *d_remove, uint64_t *n_tips, uint64_t *n_bubbles, uint64_t *n_removed) {
    if (n_tips) *n_tips = 0;
    if (n_bubbles) *n_bubbles = 0;
    if (n_removed) *n_removed = 0;
    if (!ctx || !n_tips || !n_bubbles || !n_removed) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_simplify_mask");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 40))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^40 edges or more");
    if (n_unitigs == 0) return n_edges == 0 ? S2K_OK : c.invalid("edges without unitigs");
    if (!d_row_off || !d_uni_off || !d_uni_count || (n_edges && !d_dst)) return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    unsigned long long *w = (unsigned long long *)ctx_count_table(ctx, 256);
    if (!w) return c.nomem();
    unsigned long long *totals = w; // tips, bubbles, removed; then the check's flag
    uint32_t *bad = (uint32_t *)(w + 3);
    const uint64_t n_ids = 2 * n_unitigs;
    const unsigned grid = grid_for(n_ids);
    const uint32_t hbad = c.check(w, 32, bad, [&] {
        hipLaunchKernelGGL(simplify_check_kernel, dim3(grid), dim3(UT), 0, c.st, d_row_off, d_dst, d_uni_off, n_ids, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, or a unitig without a member");
    const UGraph g{d_row_off, d_dst, d_uni_off, d_uni_count, max_tip, max_bubble};
    unsigned long long h[3] = {0, 0, 0};
    hipLaunchKernelGGL(simplify_mask_kernel, dim3(grid), dim3(UT), 0, c.st, g, n_ids, d_remove, totals);
    c.launched();
    c.fetch(h, totals, sizeof(h));
    if (!c.sync()) return c.device_error();
    *n_tips = h[0];
    *n_bubbles = h[1];
    *n_removed = h[2];
    return S2K_OK;
}

s2k_status s2k_graph_induced(s2k_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n_nodes, const uint64_t *d_edge_keys,
                             const uint32_t *d_edge_counts, uint64_t n_edges, const uint8_t *d_node_keep, const uint32_t *d_node_unitig,
                             const uint8_t *d_remove, uint64_t n_unitigs, uint32_t *d_new_id, uint64_t *d_keys_out, uint32_t *d_counts_out,
                             uint64_t node_capacity, uint64_t *d_edge_keys_out, uint32_t *d_edge_counts_out, uint64_t edge_capacity,
                             uint64_t *n_nodes_out, uint64_t *n_edges_out) {
    if (n_nodes_out) *n_nodes_out = 0;
    if (n_edges_out) *n_edges_out = 0;
    if (!ctx || !n_nodes_out || !n_edges_out) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_induced");
    if (n_nodes >= (1ull << 31) || n_edges >= (1ull << 40))
        return c.invalid("2^31 nodes or more (oriented node ids are 32-bit), or 2^40 edges or more");
    if (n_nodes == 0) return n_edges == 0 ? S2K_OK : c.invalid("edges without nodes");
    if (!d_node_keep && (!d_node_unitig || !d_remove)) return S2K_ERR_INVALID_ARG;
    if ((d_keys_out && !d_keys) || (d_counts_out && !d_counts) || (d_edge_counts_out && !d_edge_counts) || (n_edges && !d_edge_keys))
        return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const bool want_nodes = d_keys_out || d_counts_out, want_edges = n_edges && (d_edge_keys_out || d_edge_counts_out);
    const uint64_t node_tiles = (n_nodes + TB_TILE - 1) / TB_TILE, edge_tiles = (n_edges + TB_TILE - 1) / TB_TILE;
    Layout L; // the flag word, the two streams, new_id when the caller does not take it
    const auto flag = L.bytes<uint32_t>(64);
    const auto nodes_ws = carve(L, n_nodes, node_tiles), edges_ws = carve(L, n_edges, edge_tiles);
    const auto ids = L.take<uint32_t>(!d_new_id && want_edges ? n_nodes : 0);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    const CompactWs nw = nodes_ws(w), ew = edges_ws(w);
    uint32_t *bad = flag(w);
    uint32_t *new_id = d_new_id ? d_new_id : want_edges ? ids(w) : nullptr;
    uint64_t nodes = 0, edges = 0;
    const uint32_t hbad = c.check(bad, 4, bad, [&] {
        hipLaunchKernelGGL(node_count_kernel, dim3((unsigned)node_tiles), dim3(TB_THREADS), 0, c.st, d_node_keep, d_node_unitig, d_remove,
                           n_unitigs, n_nodes, nw, bad);
        c.launched();
        c.scan(nw.tile_kept, node_tiles, nw.tile_off, nodes_ws.scan_tmp(w));
        if (c.ok() && n_edges) {
            hipLaunchKernelGGL(edge_count_kernel, dim3((unsigned)edge_tiles), dim3(TB_THREADS), 0, c.st, d_edge_keys, n_edges, n_nodes, nw.wmask,
                               ew, bad);
            c.launched();
            c.scan(ew.tile_kept, edge_tiles, ew.tile_off, edges_ws.scan_tmp(w));
            c.fetch(&edges, ew.tile_off + edge_tiles, 8);
        }
        c.fetch(&nodes, nw.tile_off + node_tiles, 8);
    });
    if (!c.ok()) return c.device_error();
    if (hbad) return c.invalid("a node_unitig entry >= n_unitigs, or an edge that names a node >= n_nodes");
    *n_nodes_out = nodes;
    *n_edges_out = edges;
    if (!d_new_id && !want_nodes && !want_edges) return S2K_OK;
    if ((want_nodes && nodes > node_capacity) || (want_edges && edges > edge_capacity)) return S2K_ERR_CAPACITY;
    hipLaunchKernelGGL(node_write_kernel, dim3((unsigned)node_tiles), dim3(TB_THREADS), 0, c.st, d_keys, d_counts, n_nodes, nw, new_id, d_keys_out,
                       d_counts_out);
    c.launched();
    if (c.ok() && want_edges) {
        hipLaunchKernelGGL(edge_write_kernel, dim3((unsigned)edge_tiles), dim3(TB_THREADS), 0, c.st, d_edge_keys, d_edge_counts, n_edges, ew, new_id,
                           d_edge_keys_out, d_edge_counts_out);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

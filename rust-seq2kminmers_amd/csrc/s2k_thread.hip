// s2k_thread.hip -- reads threaded through the unitig graph: where every node lies on the oriented unitigs, and each read's items
// compressed into the steps of its path (include/s2k.h: s2k_unitig_node_places, s2k_table_thread).
//
// s2k_unitig_node_places, one lane per node: places_check_kernel (unitig < n_unitigs, its members inside [0, n_nodes], pos < len,
// members[uni_off[t] + pos] >> 1 == i; one flag word, read by the host before anything is written, every read clamped to the arrays
// whatever they hold), then places_write_kernel (one 16-byte store per node).
//
// s2k_table_thread, runs of items (s2k_runs_dev.h: the two masks, the scan, the offsets, the pairing of tails with heads and the
// staged writes are there), tiles of TB_TILE items (lane tid holds items r * 256 + tid):
//  1. thread_count_kernel: the look-up with ranks fused in, one 16-byte gather of the place record per item, (U, q) per item to
//     workspace (8 B).  The tile's items and one halo item on either side (the item before the tile by lane 64, the one after it by
//     lane 0, looked up once more) go to LDS; the read starts in [t0, t0 + TB_TILE] are marked from the reads a binary search of
//     km_off finds there.  Heads: solid, does not continue its predecessor; tails: solid, its successor does not continue it.  A
//     record that names a unitig >= n_unitigs or a position outside it sets the flag word.
//  2. run_offsets_kernel: path_off[r] = heads before km_off[r].
//  3. thread_write_kernel (when step arrays are wanted and fit, or d_uni_items is given): step s is the s-th head and the s-th tail.
//     unitig, pos, item, flags and start come from the head, count and end from the tail.  One integer atomic per step adds count
//     to d_uni_items.
//
// Workspace (the context's grow-only count workspace): 8 B per item, and per mask 8 B + 4 B per 64 items and 4 B + 8 B per tile.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_runs_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

static_assert(sizeof(s2k_node_place) == 16, "the place record is one 16-byte load");

// ---- places ----------------------------------------------------------------------------------------------------------------------
struct Unitigs {
    const uint64_t *uni_off;
    const uint32_t *members, *node_unitig, *node_pos;
    const uint8_t *circular;
    uint64_t n_nodes, n_unitigs;
};

__global__ __launch_bounds__(256) void places_check_kernel(Unitigs g, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n_nodes) return;
    const uint64_t t = g.node_unitig[i], p = g.node_pos[i];
    bool ok = t < g.n_unitigs;
    if (ok) {
        const uint64_t a = g.uni_off[t], b = g.uni_off[t + 1];
        ok = a < b && b <= g.n_nodes && p < b - a;
        if (ok) ok = (g.members[a + p] >> 1) == i;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void places_write_kernel(Unitigs g, s2k_node_place *__restrict__ place) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n_nodes) return;
    const uint32_t t = g.node_unitig[i], p = g.node_pos[i];
    const uint64_t a = g.uni_off[t];
    const uint32_t len = (uint32_t)(g.uni_off[t + 1] - a), o = g.members[a + p] & 1u;
    const uint4 rec = make_uint4(2u * t + o, o ? len - 1u - p : p, len, g.circular[t] ? 1u : 0u);
    ((uint4 *)place)[i] = rec;
}

// ---- threading -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t TH_NONE = 0xFFFFFFFFu; // U of an item that is not solid (an oriented unitig stays below 2^32 - 2: < 2^31 nodes)

struct ThreadWs {
    uint2 *uq; // per item: (U, q), U == TH_NONE when it is not solid
    RunWs run;
};

struct Item { // what the step rule reads of one item
    uint32_t U, q;
    bool wrap; // the last position of a circular unitig: position 0 continues it
};

__device__ __forceinline__ Item item_of(uint4 rec, uint32_t rev, bool solid) {
    Item it{TH_NONE, 0u, false};
    if (solid) {
        it.U = rec.x ^ rev;
        it.q = rev ? rec.z - 1u - rec.y : rec.y;
        it.wrap = rec.w != 0 && it.q == rec.z - 1u;
    }
    return it;
}
__device__ __forceinline__ bool place_ok(uint4 rec, uint64_t n_unitigs) { return (rec.x >> 1) < n_unitigs && rec.y < rec.z; }

__global__ __launch_bounds__(TB_THREADS) void thread_count_kernel(TableView tv, const uint64_t *__restrict__ km_off, uint64_t n_reads,
                                                                  const uint64_t *__restrict__ hash, const uint8_t *__restrict__ rev,
                                                                  uint64_t n_items, uint32_t minc, const uint4 *__restrict__ place,
                                                                  uint64_t n_unitigs, ThreadWs ws, uint32_t *__restrict__ bad) {
    // index x + 1 <-> item t0 + x: index 0 is the item before the tile, index TB_TILE + 1 the one after it
    __shared__ uint32_t sU[TB_TILE + 2], sq[TB_TILE + 2];
    __shared__ uint8_t swrap[TB_TILE + 2], sstart[TB_TILE + 2]; // sstart: the item starts a read
    __shared__ uint64_t sreads[2];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint64_t q[TB_Q];
    uint32_t c[TB_Q], pos[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = hash[std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, n_items - 1)];
    if (tid < 2) sreads[tid] = tid ? reads_upto(km_off, n_reads, t0 + TB_TILE) : t0 ? reads_upto(km_off, n_reads, t0 - 1) : 0;
    lookup_many<true>(tv, q, c, pos);
    uint4 rec[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) rec[r] = tv.n ? place[pos[r]] : make_uint4(0, 0, 0, 0); // a miss has rank 0: every gather is in flight at once
    bool ok = true;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int x = r * TB_THREADS + tid;
        const uint64_t j = t0 + x;
        Item it{TH_NONE, 0u, false};
        if (j < n_items) {
            const bool solid = c[r] >= minc;
            if (solid) ok &= place_ok(rec[r], n_unitigs);
            it = item_of(rec[r], rev[j], solid);
            ws.uq[j] = make_uint2(it.U, it.q);
        }
        sU[x + 1] = it.U;
        sq[x + 1] = it.q;
        swrap[x + 1] = it.wrap;
        sstart[x + 1] = 0;
    }
    if (tid == 0 || tid == 64) { // the two halo items, one lane of two different waves
        const bool after = tid == 0;
        const uint64_t j = after ? t0 + TB_TILE : t0 - 1; // t0 - 1 wraps to 2^64 - 1 for the first tile: no such item
        Item it{TH_NONE, 0u, false};
        if (j < n_items) {
            uint32_t hc, hp;
            lookup_one(tv, hash[j], &hc, &hp);
            if (hc >= minc) {
                const uint4 hrec = place[hp];
                ok &= place_ok(hrec, n_unitigs);
                it = item_of(hrec, rev[j], true);
            }
        }
        const int i = after ? TB_TILE + 1 : 0;
        sU[i] = it.U;
        sq[i] = it.q;
        swrap[i] = it.wrap;
        sstart[i] = 0;
    }
    if (!ok) atomicOr(bad, 1u);
    __syncthreads();
    for (uint64_t r = sreads[0] + tid; r < sreads[1]; r += TB_THREADS) {
        const uint64_t x = km_off[r] - t0; // in [0, TB_TILE] for a non-decreasing km_off; a table that is not one writes no LDS outside
        if (x <= TB_TILE) sstart[x + 1] = 1;
    }
    __syncthreads();
    // index i continues index i - 1 (i >= 1); a first tile's index 0 and everything from item n_items on hold TH_NONE
    auto continues = [&](int i) {
        const uint32_t a = sU[i - 1], b = sU[i];
        return a != TH_NONE && b == a && !sstart[i] && (sq[i] == sq[i - 1] + 1u || (swrap[i - 1] && sq[i] == 0u));
    };
    auto solid = [&](int i) { return sU[i] != TH_NONE; };
    run_count_end(
        ws.run, t0, n_items, [&](int, int i) { return solid(i) && !continues(i); }, [&](int, int i) { return solid(i) && !continues(i + 1); },
        [&] { return continues(1); });
}

struct ThreadIo {
    const uint64_t *km_off;
    uint64_t n_reads;
    const uint32_t *start, *end;
    uint32_t *o_unitig, *o_pos, *o_count, *o_item, *o_flags, *o_start, *o_end;
    unsigned long long *uni_items;
};

__global__ __launch_bounds__(TB_THREADS) void thread_write_kernel(ThreadIo io, uint64_t n_items, ThreadWs ws) {
    __shared__ uint4 stage4[TB_TILE / 4 + 1]; // a run of 32-bit elements starts at most 3 elements into its first 16-byte piece
    __shared__ uint64_t sread[2];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, t1 = std::min<uint64_t>(t0 + TB_TILE, n_items);
    RunTile rt;
    if (!run_tile(ws.run, n_items, true, rt, [&] {
            if (tid < 2 && (io.o_item || io.o_flags)) // the reads that hold the tile's first and last item
                sread[tid] = read_of(io.km_off, 0, io.n_reads - 1, tid == 0 ? t0 : t1 - 1);
        }))
        return;
    if (rt.htot) {
        rt.leave_heads(io.o_unitig, stage4, [&](int, uint64_t j) { return ws.uq[j].x; });
        rt.leave_heads(io.o_pos, stage4, [&](int, uint64_t j) { return ws.uq[j].y; });
        rt.leave_heads(io.o_start, stage4, [&](int, uint64_t j) { return io.start[j]; });
        if (io.o_item || io.o_flags) {
            const uint64_t rlo = sread[0], rhi = sread[1];
            uint32_t item[TB_Q];
#pragma unroll
            for (int r = 0; r < TB_Q; r++) {
                const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
                item[r] = (rt.hkeep >> r) & 1u ? (uint32_t)(j - io.km_off[read_of(io.km_off, rlo, rhi, j)]) : 0u;
            }
            rt.leave_heads(io.o_item, stage4, [&](int r, uint64_t) { return item[r]; });
            // linked: not its read's first item, and the item before it is solid
            rt.leave_heads(io.o_flags, stage4, [&](int r, uint64_t j) { return item[r] && ws.uq[j - 1].x != TH_NONE ? S2K_STEP_LINKED : 0u; });
        }
    }
    if (rt.ttot) {
        rt.leave_tails(io.o_end, stage4, [&](int, uint64_t j) { return io.end[j]; });
        if (io.o_count || io.uni_items) {
            uint32_t count[TB_Q];
#pragma unroll
            for (int r = 0; r < TB_Q; r++) {
                count[r] = 0;
                if ((rt.tkeep >> r) & 1u) {
                    const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
                    count[r] = (uint32_t)(j - rt.head_of(r) + 1);
                    if (io.uni_items) atomicAdd(io.uni_items + (ws.uq[j].x >> 1), (unsigned long long)count[r]);
                }
            }
            rt.leave_tails(io.o_count, stage4, [&](int r, uint64_t) { return count[r]; });
        }
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_unitig_node_places(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint32_t *d_node_unitig,
                                  const uint32_t *d_node_pos, const uint8_t *d_circular, uint64_t n_nodes, uint64_t n_unitigs,
                                  s2k_node_place *d_place) {
    if (!ctx) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_unitig_node_places");
    if (n_nodes >= (1ull << 31)) return c.invalid("2^31 nodes or more (oriented ids are 32-bit)");
    if (n_nodes == 0) return S2K_OK;
    if (!d_uni_off || !d_members || !d_node_unitig || !d_node_pos || !d_circular || !d_place) return S2K_ERR_INVALID_ARG;
    if (((uintptr_t)d_place & 15u) != 0) return c.invalid("d_place must be 16-byte aligned");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    uint32_t *bad = (uint32_t *)ctx_count_table(ctx, 4);
    if (!bad) return c.nomem();
    const Unitigs g{d_uni_off, d_members, d_node_unitig, d_node_pos, d_circular, n_nodes, n_unitigs};
    const unsigned grid = (unsigned)((n_nodes + 255) / 256);
    const uint32_t hbad = c.check(bad, 4, bad, [&] { hipLaunchKernelGGL(places_check_kernel, dim3(grid), dim3(256), 0, c.st, g, bad); });
    if (!c.ok()) return c.device_error();
    if (hbad) return c.invalid("a node whose unitig is >= n_unitigs, whose position lies outside it, or that is not the member there");
    hipLaunchKernelGGL(places_write_kernel, dim3(grid), dim3(256), 0, c.st, g, d_place);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_table_thread(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, const s2k_node_place *d_place,
                            uint64_t n_nodes, const s2k_thread_out *out, uint64_t *d_uni_items, uint64_t n_unitigs, uint64_t *n_steps) {
    if (n_steps) *n_steps = 0;
    if (!t || !in || !out || !n_steps || !in->km_off || !in->hash || !in->rev || !out->path_off || (out->start && !in->start) ||
        (out->end && !in->end) || (n_nodes && !d_place))
        return S2K_ERR_INVALID_ARG;
    Call c(t->ctx, "s2k_table_thread");
    if (t->n >= (1ull << 31)) return c.invalid("2^31 keys or more (oriented ids are 32-bit)");
    if (n_nodes != t->n) return c.invalid("n_nodes is not the table's number of keys");
    if (((uintptr_t)d_place & 15u) != 0) return c.invalid("d_place must be 16-byte aligned");
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const Ends ends = read_ends(c, in->km_off, nullptr, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ends.n_items < ends.km0) return c.invalid("in->km_off must start at 0 and end at or after its start");
    const uint64_t n_items = ends.n_items;
    if (n_items == 0) { // no items: every path is empty
        c.zero(out->path_off, (n_reads + 1) * 8);
        if (!c.sync()) return c.device_error();
        return S2K_OK;
    }
    const uint64_t nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many items for one call");
    Layout L;
    const auto flag = L.bytes<uint32_t>(64);
    const auto uq = L.take<uint2>(n_items);
    const auto runs = carve_runs(L, n_items, nt);
    char *w = L.alloc(t->ctx);
    if (!w) return c.nomem();
    const ThreadWs ws{uq(w), runs(w)};
    uint32_t *bad = flag(w);
    const uint32_t minc = min_count ? min_count : 1u;
    uint64_t total = 0;
    const uint32_t hbad = c.check(bad, 4, bad, [&] {
        hipLaunchKernelGGL(thread_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), in->km_off, n_reads, in->hash, in->rev,
                           n_items, minc, (const uint4 *)d_place, n_unitigs, ws, bad);
        c.launched();
        c.scan(ws.run.h.tile_kept, nt, ws.run.h.tile_off, runs.h.scan_tmp(w));
        c.fetch(&total, ws.run.h.tile_off + nt, 8);
    });
    if (!c.ok()) return c.device_error();
    if (hbad) return c.invalid("a place record that names a unitig >= n_unitigs or a position outside its unitig");
    *n_steps = total;
    launch_run_offsets(c, in->km_off, n_reads, n_items, nt, ws.run, out->path_off);
    const bool want = out->unitig || out->pos || out->count || out->item || out->flags || out->start || out->end;
    const bool fits = total <= out->capacity;
    if (c.ok() && total && ((want && fits) || (d_uni_items && !want))) {
        ThreadIo io{in->km_off, n_reads, in->start, in->end, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                    (unsigned long long *)d_uni_items};
        if (want) {
            io.o_unitig = out->unitig, io.o_pos = out->pos, io.o_count = out->count, io.o_item = out->item, io.o_flags = out->flags;
            io.o_start = out->start, io.o_end = out->end;
        }
        hipLaunchKernelGGL(thread_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, io, n_items, ws);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return want && !fits ? S2K_ERR_CAPACITY : S2K_OK;
}

} // extern "C"

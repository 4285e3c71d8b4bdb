// s2k_bridge.hip -- error gaps in read paths bridged: consecutive steps of a read that lie a few items apart on one unitig are merged,
// and two that lie a few items apart across one edge are extended to the edge, so that the spans, walks and GAF lines downstream see
// the crossing (include/s2k.h: s2k_paths_bridge).
//
// The stable stream compaction of s2k_compact_dev.h with two masks, as s2k_table_thread and s2k_paths_walks, over tiles of TB_TILE
// steps (lane tid holds steps r * 256 + tid):
//  1. bridge_check_kernel: the path and CSR rules of walks_check_kernel (s2k_walk.hip) without the base-space arrays, and no unitig
//     of 2^32 members or more.  One flag word, read by the host before anything is written; every read is clamped to the arrays.
//  2. bridge_count_kernel: per step its unitig, where it ends (pos + count), the members left behind it (len - pos - count; BR_NONE
//     on a circular unitig) and the item it ends at go to LDS with the step before the tile; the read starts in [t0, t0 + TB_TILE] are
//     marked from the reads a binary search of path_off finds there.  One lane per step decides join from its neighbour in LDS; the
//     row search of kind 2 runs only where the limits already stand, the row bounds of all TB_Q steps loaded before the first probe,
//     the TB_Q searches side by side.  join goes to workspace and to LDS; one lane decides the step after the tile.  Heads (join !=
//     1) and tails (the step after it is not joined by 1): two ballots per 64 steps, tile_prefixes twice, and whether a run is open at
//     the tile's first step.  Merged and bridged joins: a block sum.  An item order that would wrap gi sets the flag word, which the
//     host reads again with the totals, before anything is written.
//  3. launch_scan_u32 over the heads per tile (tails before a tile = heads before it - open) and over count: matched is a difference
//     of two prefix entries.
//  4. bridge_offsets_kernel: out path_off[r] = heads before path_off[r].
//  5. bridge_write_kernel: output step s is the s-th head and the s-th tail, paired as in thread_write_kernel and walks_write_kernel
//     (heads' indices in LDS by slot; the one tail per tile whose head lies in an earlier tile finds it by head_item).  The tail's
//     lane gathers the head's fields and the join of the step after it; each array is staged in LDS and leaves with leave_run.  No
//     lane walks a run, and there is no atomic on an output.
//
// Workspace (the context's grow-only count workspace): 9 B per step (join 1, the prefix of count 8), and per mask 8 B + 4 B per 64
// steps and 4 B + 8 B per tile.
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
    uint8_t *join;       // per step
    uint64_t *C;         // n_steps + 1: the exclusive prefix of count
    uint32_t *tile_open; // per tile: 1 when its first step is joined to the step before it on the same unitig
    CompactWs h, t;      // heads; tails (of the tails only wmask, wpre and tile_kept are used)
};

__global__ __launch_bounds__(UT) void bridge_check_kernel(BridgeIn p, Csr g, uint64_t n_edges, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t n_ids = 2 * p.n_unitigs;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t r = i0; r <= p.n_reads; r += stride) {
        const uint64_t a = p.path_off[r];
        if (r == 0 && a != 0) ok = false;
        if (r == p.n_reads ? a != p.n_steps : a > p.path_off[r + 1]) ok = false;
    }
    for (uint64_t s = i0; s < p.n_steps; s += stride) {
        const uint64_t U = p.unitig[s];
        if (U >= n_ids) {
            ok = false;
            continue;
        }
        const uint64_t a = p.uni_off[U >> 1], b = p.uni_off[(U >> 1) + 1], c = p.count[s], q = p.pos[s];
        if (a >= b || c == 0 || q >= b - a || (!p.circular[U >> 1] && q + c > b - a)) ok = false;
    }
    for (uint64_t u = i0; u < n_ids; u += stride) {
        if (!csr_ids_ok(g.row_off, g.dst, u, n_ids, n_edges)) ok = false;
        if (u & 1) continue;
        const uint64_t a = p.uni_off[u >> 1], b = p.uni_off[(u >> 1) + 1];
        if (a >= b || b - a >= (1ull << 32)) ok = false;
    }
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
    __shared__ uint32_t wch[TB_WORDS], wct[TB_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
    for (;;) { // TB_Q searches side by side
        bool more = false;
#pragma unroll
        for (int r = 0; r < TB_Q; r++) {
            if (lo[r] < hi[r]) {
                const uint64_t mid = (lo[r] + hi[r]) >> 1;
                const uint32_t v = g.dst[mid], B = U[r];
                if (v < B) lo[r] = mid + 1;
                else if (v > B) hi[r] = mid;
                else {
                    kind[r] = 2;
                    lo[r] = hi[r];
                }
                more |= lo[r] < hi[r];
            }
        }
        if (!more) break;
    }
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
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        const bool valid = t0 + (i - 1) < p.n_steps;
        const uint64_t mh = __ballot(valid && s.join[i] != 1), mt = __ballot(valid && s.join[i + 1] != 1);
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64;
        if (lane == 0) {
            wch[r * 4 + wv] = (uint32_t)__popcll(mh);
            wct[r * 4 + wv] = (uint32_t)__popcll(mt);
            if (w0 < p.n_steps) {
                ws.h.wmask[w0 >> 6] = mh;
                ws.t.wmask[w0 >> 6] = mt;
            }
        }
    }
    if (tid == 0) ws.tile_open[blockIdx.x] = s.join[1] == 1;
    __syncthreads();
    tile_prefixes(wch, t0, p.n_steps, ws.h);
    tile_prefixes(wct, t0, p.n_steps, ws.t);
    block_add(n, totals);
    if (wrong) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void bridge_offsets_kernel(const uint64_t *__restrict__ path_off, uint64_t n_reads, uint64_t n_steps, uint64_t n_tiles,
                                                             CompactWs heads, uint64_t *__restrict__ out_off) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    out_off[r] = kept_before(heads, n_steps, n_tiles, path_off[r]);
}

struct BridgeOut {
    uint32_t *unitig, *pos, *count, *item, *flags, *start, *end, *matched;
};

__global__ __launch_bounds__(TB_THREADS) void bridge_write_kernel(BridgeIn p, BridgeOut io, BridgeWs ws) {
    __shared__ uint4 stage4[(TB_TILE + 2 * STAGE_PAD) / 4]; // TB_TILE 32-bit elements, and a run's shift
    __shared__ uint32_t shead[TB_TILE];                     // by head slot: the head's step, relative to the tile
    __shared__ uint64_t sopen;
    uint32_t *stage = (uint32_t *)stage4;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t hbase = ws.h.tile_off[blockIdx.x];
    const uint32_t ttot = ws.t.tile_kept[blockIdx.x];
    if (ttot == 0) return;
    const uint32_t open = ws.tile_open[blockIdx.x];
    const uint64_t tbase = hbase - open; // tails before the tile: every head before it has its tail but the open one
    uint32_t hslot[TB_Q], tslot[TB_Q];
    const uint32_t hkeep = tile_slots(ws.h, t0, p.n_steps, hslot), tkeep = tile_slots(ws.t, t0, p.n_steps, tslot);
    if (tid == 64 && open) sopen = head_item(ws.h, blockIdx.x, tbase);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if ((hkeep >> r) & 1u) shead[hslot[r]] = (uint32_t)(r * TB_THREADS + tid);
    __syncthreads();
    uint64_t hd[TB_Q];
    uint32_t opos[TB_Q], ocnt[TB_Q], edge = 0; // edge: the run's head was entered across an edge
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hd[r] = 0, opos[r] = ocnt[r] = 0;
        if ((tkeep >> r) & 1u) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t h = tslot[r] >= open ? t0 + shead[tslot[r] - open] : sopen;
            const bool in2 = ws.join[h] == 2, out2 = j + 1 < p.n_steps && ws.join[j + 1] == 2; // a read's first step has join 0
            const uint32_t Uj = p.unitig[j];
            const uint32_t endpos = out2 ? (uint32_t)(p.uni_off[(Uj >> 1) + 1] - p.uni_off[Uj >> 1]) : p.pos[j] + p.count[j];
            hd[r] = h;
            opos[r] = in2 ? 0u : p.pos[h];
            ocnt[r] = endpos - opos[r];
            edge |= (in2 ? 1u : 0u) << r;
        }
    }
#define BR_LEAVE(OUT, VAL)                                                                  \
    do {                                                                                    \
        if (OUT) {                                                                          \
            const uint32_t sh = shift_of(OUT + tbase);                                      \
            _Pragma("unroll") for (int r = 0; r < TB_Q; r++) if ((tkeep >> r) & 1u) {       \
                const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;                     \
                (void)j;                                                                    \
                stage[sh + tslot[r]] = (VAL);                                               \
            }                                                                               \
            __syncthreads();                                                                \
            leave_run(OUT + tbase, stage, sh, ttot);                                        \
        }                                                                                   \
    } while (0)
    BR_LEAVE(io.unitig, p.unitig[hd[r]]);
    BR_LEAVE(io.pos, opos[r]);
    BR_LEAVE(io.count, ocnt[r]);
    BR_LEAVE(io.item, p.item[hd[r]]);
    BR_LEAVE(io.flags, p.flags[hd[r]] | (((edge >> r) & 1u) ? S2K_STEP_LINKED : 0u));
    BR_LEAVE(io.start, p.start[hd[r]]);
    BR_LEAVE(io.end, p.end[j]);
    BR_LEAVE(io.matched, (uint32_t)(ws.C[j + 1] - ws.C[hd[r]]));
#undef BR_LEAVE
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
    if (!ctx || !paths || !out || !n_out_steps || !n_merged || !n_bridged || !paths->path_off || !out->path_off) return S2K_ERR_INVALID_ARG;
    if (n_steps && (!paths->unitig || !paths->pos || !paths->count || !paths->item || !paths->flags)) return S2K_ERR_INVALID_ARG;
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
    const auto topen = L.take<uint32_t>(nt);
    const auto hw = carve(L, n_steps, nt), tw = carve(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 2);
    const BridgeWs ws{join(w), C(w), topen(w), hw(w), tw(w)};
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
    hipLaunchKernelGGL(bridge_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, ws, totals, bad);
    c.launched();
    c.scan(ws.h.tile_kept, nt, ws.h.tile_off, hw.scan_tmp(w));
    c.fetch(&total, ws.h.tile_off + nt, 8);
    c.fetch(h, totals, sizeof(h));
    c.fetch(&hbad, bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad) return c.invalid(refusal);
    *n_out_steps = total;
    *n_merged = h[0];
    *n_bridged = h[1];
    const bool records = out->unitig || out->pos || out->count || out->item || out->flags || out->start || out->end || d_matched;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (d_join) c.copy(d_join, ws.join, n_steps, hipMemcpyDeviceToDevice);
    hipLaunchKernelGGL(bridge_offsets_kernel, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, c.st, paths->path_off, n_reads, n_steps, nt, ws.h,
                       out->path_off);
    c.launched();
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

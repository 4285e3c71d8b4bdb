// s2k_walk.hip -- read walks on the unitig graph with base coordinates: where every member's piece lies in the stitched unitigs, and
// each read's steps joined into walks along the graph's edges, lifted to bases (include/s2k.h: s2k_unitig_member_offsets,
// s2k_paths_walks).
//
// s2k_unitig_member_offsets: the stitch's piece-length, last-member, scan and offset passes (s2k_stitch_dev.h) without the copy
// kernel; the scan's first n_nodes entries are the member offsets.
//
// s2k_paths_walks, the stable stream compaction of s2k_compact_dev.h with two masks, as s2k_table_thread, over tiles of TB_TILE steps
// (lane tid holds steps r * 256 + tid):
//  1. walks_check_kernel: the rules of spans_check_kernel; every step has count >= 1, pos < len, and pos + count <= len unless its
//     unitig is circular; uni_off runs from 0 to n_nodes; out_off does not decrease and no unitig has 2^32 bases or more; every
//     member < 2 n_nodes, its offset inside its unitig's bases (the unitig by a search of uni_off).  One flag word, read by the host
//     before anything is written; every read is clamped to the arrays whatever they hold.
//  2. walks_count_kernel: follow_tile (s2k_span_dev.h: the row searches of spans_count_kernel, side by side) gives the edge every
//     step follows, to workspace and LDS.  Heads (the step follows no edge) and tails (the step after it follows none): two ballots
//     per 64 steps, tile_prefixes twice, and whether a walk is open at the tile's first step.  Per step adv(U) to workspace.
//  3. launch_scan_u32 over the heads per tile (tails before a tile = heads before it - open), over adv and over count: a walk's
//     path_len, path_end and items are differences of two prefix entries.
//  4. walks_offsets_kernel: walk_off[r] = heads before path_off[r].
//  5. walks_write_kernel: walk s is the s-th head and the s-th tail, paired as in thread_write_kernel (heads' indices in LDS by slot;
//     the one tail per tile whose head lies in an earlier tile finds it by head_item).  The tail's lane gathers the head's step, the
//     two prefixes and the two base intervals; each array is staged in LDS and leaves with leave_run.  No lane walks a walk.
//
// Workspace (the context's grow-only count workspace): member offsets 12 B per member; walks 24 B per step (edge 4, adv 4, two
// prefixes 8 + 8), and per mask 8 B + 4 B per 64 steps and 4 B + 8 B per tile.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_span_dev.h"
#include "s2k_stitch_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

// the decomposition and where its members lie in base space
struct Lift {
    const uint64_t *uni_off, *member_off, *out_off;
    const uint32_t *members, *seq_len, *overlap;
    const uint8_t *circular;
    uint64_t n_unitigs, n_nodes;
};

struct WalkWs {
    uint32_t *edge, *adv; // per step: the edge it follows (SP_NONE: none); adv(unitig)
    uint64_t *A, *C;      // n_steps + 1: the exclusive prefixes of adv and of count
    uint32_t *tile_open;  // per tile: 1 when its first step follows an edge
    CompactWs h, t;       // heads; tails (of the tails only wmask, wpre and tile_kept are used)
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

__global__ __launch_bounds__(UT) void walks_check_kernel(Paths p, Csr g, Lift v, uint64_t n_edges, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t n_ids = 2 * v.n_unitigs;
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
        const uint64_t a = v.uni_off[U >> 1], b = v.uni_off[(U >> 1) + 1], c = p.count[s], q = p.pos[s];
        if (a >= b || c == 0 || q >= b - a || (!v.circular[U >> 1] && q + c > b - a)) ok = false;
    }
    for (uint64_t u = i0; u < n_ids; u += stride) {
        if (!csr_ids_ok(g.row_off, g.dst, u, n_ids, n_edges)) ok = false;
        if (u & 1) continue;
        const uint64_t t = u >> 1, a = v.uni_off[t], b = v.uni_off[t + 1], oa = v.out_off[t], ob = v.out_off[t + 1];
        if (a >= b || b > v.n_nodes || (t == 0 && a != 0) || (t == v.n_unitigs - 1 && b != v.n_nodes)) ok = false;
        if (oa > ob || ob - oa >= (1ull << 32)) ok = false;
    }
    for (uint64_t x = i0; x < v.n_nodes; x += stride) {
        if (v.members[x] >= 2 * v.n_nodes) ok = false;
        const uint64_t t = unitig_of(v.uni_off, v.n_unitigs, x), o = v.member_off[x];
        if (o < v.out_off[t] || o > v.out_off[t + 1]) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(TB_THREADS) void walks_count_kernel(Paths p, Csr g, Lift v, WalkWs ws,
                                                                 unsigned long long *__restrict__ totals /* followed, off-graph */) {
    __shared__ FollowLds s;
    __shared__ uint32_t wch[TB_WORDS], wct[TB_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        const bool valid = t0 + (i - 1) < p.n_steps;
        const uint64_t mh = __ballot(valid && s.E[i] == SP_NONE), mt = __ballot(valid && s.E[i + 1] == SP_NONE);
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
    if (tid == 0) ws.tile_open[blockIdx.x] = s.E[1] != SP_NONE;
    __syncthreads();
    tile_prefixes(wch, t0, p.n_steps, ws.h);
    tile_prefixes(wct, t0, p.n_steps, ws.t);
    block_add(n, totals);
}

__global__ __launch_bounds__(256) void walks_offsets_kernel(const uint64_t *__restrict__ path_off, uint64_t n_reads, uint64_t n_steps, uint64_t n_tiles,
                                                            CompactWs heads, uint64_t *__restrict__ walk_off) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    walk_off[r] = kept_before(heads, n_steps, n_tiles, path_off[r]);
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

struct WalkIo {
    const uint32_t *start, *end;
    uint64_t *first_step, *items, *path_len, *path_start, *path_end;
    uint32_t *n_steps, *qstart, *qend, *flags;
};

__global__ __launch_bounds__(TB_THREADS) void walks_write_kernel(Paths p, Lift v, WalkIo io, WalkWs ws) {
    __shared__ uint4 stage4[(TB_TILE + STAGE_PAD) / 2]; // TB_TILE 64-bit elements, and a run's shift
    __shared__ uint32_t shead[TB_TILE];                 // by head slot: the head's step, relative to the tile
    __shared__ uint64_t sopen;
    uint64_t *stage8 = (uint64_t *)stage4;
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
    uint64_t hd[TB_Q], pstart[TB_Q], pend[TB_Q], plen[TB_Q];
    uint32_t circ = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hd[r] = pstart[r] = pend[r] = plen[r] = 0;
        if ((tkeep >> r) & 1u) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t h = tslot[r] >= open ? t0 + shead[tslot[r] - open] : sopen;
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
#define WK_LEAVE(OUT, STAGE, VAL)                                                           \
    do {                                                                                    \
        if (OUT) {                                                                          \
            const uint32_t sh = shift_of(OUT + tbase);                                      \
            _Pragma("unroll") for (int r = 0; r < TB_Q; r++) if ((tkeep >> r) & 1u) {       \
                const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;                     \
                (void)j;                                                                    \
                STAGE[sh + tslot[r]] = (VAL);                                               \
            }                                                                               \
            __syncthreads();                                                                \
            leave_run(OUT + tbase, STAGE, sh, ttot);                                        \
        }                                                                                   \
    } while (0)
    WK_LEAVE(io.first_step, stage8, hd[r]);
    WK_LEAVE(io.items, stage8, ws.C[j + 1] - ws.C[hd[r]]);
    WK_LEAVE(io.path_len, stage8, plen[r]);
    WK_LEAVE(io.path_start, stage8, pstart[r]);
    WK_LEAVE(io.path_end, stage8, pend[r]);
    WK_LEAVE(io.n_steps, stage, (uint32_t)(j - hd[r] + 1));
    WK_LEAVE(io.qstart, stage, io.start[hd[r]]);
    WK_LEAVE(io.qend, stage, io.end[j] + 1u);
    WK_LEAVE(io.flags, stage, (circ >> r) & 1u);
#undef WK_LEAVE
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
    if (!ctx || !paths || !n_walks || !n_followed || !n_off_graph || !paths->path_off) return S2K_ERR_INVALID_ARG;
    if (n_steps && (!paths->unitig || !paths->pos || !paths->count || !paths->flags)) return S2K_ERR_INVALID_ARG;
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
    const auto topen = L.take<uint32_t>(nt);
    const auto hw = carve(L, n_steps, nt), tw = carve(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 2);
    const WalkWs ws{edge(w), adv(w), A(w), C(w), topen(w), hw(w), tw(w)};
    const Paths p{paths->path_off, paths->unitig, paths->pos, paths->count, paths->flags, n_reads, n_steps};
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
    hipLaunchKernelGGL(walks_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, p, g, v, ws, totals);
    c.launched();
    c.scan(ws.h.tile_kept, nt, ws.h.tile_off, hw.scan_tmp(w));
    c.fetch(&total, ws.h.tile_off + nt, 8);
    c.fetch(h, totals, sizeof(h));
    if (!c.sync()) return c.device_error();
    *n_walks = total;
    *n_followed = h[0];
    *n_off_graph = h[1];
    if (!out) return S2K_OK;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (out->edge) c.copy(out->edge, ws.edge, n_steps * 4, hipMemcpyDeviceToDevice);
    if (out->walk_off) {
        hipLaunchKernelGGL(walks_offsets_kernel, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, c.st, paths->path_off, n_reads, n_steps, nt, ws.h,
                           out->walk_off);
        c.launched();
    }
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

// s2k_lift.hip -- read paths lifted from the unitigs onto the contigs that the untangling made of them: where every copy of a unitig
// lies on the contigs, and every step of a path mapped to the copy its read used, the steps that the compaction put side by side
// merged into one (include/s2k.h: s2k_unitig_copy_places, s2k_paths_lift).
//
// s2k_unitig_copy_places:
//  1. places_check_kernel: the checks of expand_check_kernel (s2k_untangle.hip) on the same arrays, the piece length of every outer
//     member, and slot_of[copy] = the member slot that names it; places_verify_kernel reads slot_of back: two slots that name one copy
//     cannot both find themselves there, so the members are a permutation of the copies and every record has one writer.
//  2. launch_scan_u32 over the piece lengths; places_contig_kernel, one lane per contig: no contig of 2^32 instances or more.  One
//     flag word for all of it, read by the host before anything is written.
//  3. places_write_kernel, one lane per outer member: its contig by a binary search of the outer uni_off, its record.
//
// s2k_paths_lift, runs of steps (s2k_runs_dev.h), tiles of TB_TILE steps:
//  1. lift_check_kernel: the shared rules of s2k_span_dev.h (path_off_ok, steps_ok, unitig_row_ok), the resolved bytes, copy_off against
//     the rows, every copy record against its unitig.  One flag word, read by the host before anything is written.
//  2. lift_count_kernel: follow_tile (s2k_span_dev.h) gives the edge every step of the tile follows and that of the step behind the
//     tile, which is the leaving edge of the tile's last step.  One lane per step picks the copy (one search of one row for tw(e), only
//     on an even strand of a resolved unitig) and maps the position; V, q' and count go to LDS.  One lane does the same for the step
//     before the tile, whose entering edge takes the one search that follow_tile has not made, and one lane for the step behind it,
//     whose entering edge alone matters.  join from the neighbour in LDS.  Heads: kept, join == 0; tails: kept, the step behind it not
//     joined.  Merged, dropped and conflicts: a block sum.
//  3. launch_scan_u32 over count and over matched_in: a run's sums are differences of two prefix entries.
//  4. run_offsets_kernel: out path_off[r] = heads before path_off[r].
//  5. lift_write_kernel: output step s is the s-th head and the s-th tail.  The tail's lane maps the head again from its copy.
//     lift_items_kernel, one lane per kept input step, adds its count to its contig: the only atomic on an output, an integer sum.
//
// Workspace (the context's grow-only count workspace).  Copy places: 16 B per copy (piece length, piece offset, slot_of).  Lift: 21 B
// per step (join 1, copy 4, the prefixes of count and of matched_in 8 each), and per mask 8 B + 4 B per 64 steps and 4 B + 8 B per tile.
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

// ---- copy places ---------------------------------------------------------------------------------------------------------------------
struct Outer {
    const uint64_t *off;
    const uint32_t *members;
    const uint8_t *circular;
    uint64_t n_contigs, n_copies;
};

struct Inner {
    const uint64_t *uni_off;
    const uint8_t *circular;
    uint64_t n_unitigs;
};

struct PlaceWs {
    uint32_t *len;     // per outer member: the members of its origin
    uint32_t *slot_of; // per copy: the member slot that names it
    uint64_t *off;     // n_copies + 1: the exclusive prefix of len
};

__global__ __launch_bounds__(UT) void places_check_kernel(Outer o, Inner in, const uint32_t *__restrict__ origin, PlaceWs w, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t t = i0; t <= in.n_unitigs; t += stride) {
        const uint64_t a = in.uni_off[t];
        if (t == 0 && a != 0) ok = false;
        if (t < in.n_unitigs && (a >= in.uni_off[t + 1] || in.uni_off[t + 1] - a >= (1ull << 32))) ok = false;
    }
    for (uint64_t t = i0; t <= o.n_contigs; t += stride) {
        const uint64_t a = o.off[t];
        if (t == 0 && a != 0) ok = false;
        if (t == o.n_contigs ? a != o.n_copies : a >= o.off[t + 1]) ok = false;
    }
    for (uint64_t x = i0; x < o.n_copies; x += stride) {
        const uint32_t C = o.members[x];
        uint32_t len = 0;
        if (C >= 2 * o.n_copies) ok = false;
        else {
            w.slot_of[C >> 1] = (uint32_t)x;
            const uint32_t t = origin[C >> 1];
            if (t >= in.n_unitigs) ok = false;
            else len = (uint32_t)(in.uni_off[t + 1] - in.uni_off[t]);
        }
        w.len[x] = len;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void places_verify_kernel(Outer o, PlaceWs w, uint32_t *__restrict__ bad) {
    bool ok = true;
    for (uint64_t x = (uint64_t)blockIdx.x * UT + threadIdx.x; x < o.n_copies; x += (uint64_t)gridDim.x * UT) {
        const uint32_t C = o.members[x];
        if (C < 2 * o.n_copies && w.slot_of[C >> 1] != (uint32_t)x) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

// the instances of contig t, its bounds clamped to the pieces whatever the outer uni_off holds
__global__ __launch_bounds__(UT) void places_contig_kernel(Outer o, PlaceWs w, uint32_t *__restrict__ bad) {
    bool ok = true;
    for (uint64_t t = (uint64_t)blockIdx.x * UT + threadIdx.x; t < o.n_contigs; t += (uint64_t)gridDim.x * UT) {
        const uint64_t a = std::min(o.off[t], o.n_copies), b = std::min(o.off[t + 1], o.n_copies);
        if (a > b || w.off[b] - w.off[a] >= (1ull << 32)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void places_write_kernel(Outer o, Inner in, const uint32_t *__restrict__ origin, PlaceWs w, s2k_node_place *__restrict__ place) {
    for (uint64_t x = (uint64_t)blockIdx.x * UT + threadIdx.x; x < o.n_copies; x += (uint64_t)gridDim.x * UT) {
        uint64_t lo = 0, hi = o.n_contigs - 1; // the largest contig with uni_off <= x
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (o.off[mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        const uint64_t t = lo, a = o.off[t], b = o.off[t + 1];
        const uint32_t C = o.members[x], s = C & 1u, m = w.len[x];
        const uint32_t f = (uint32_t)(w.off[x] - w.off[a]), Lc = (uint32_t)(w.off[b] - w.off[a]);
        const bool alone = b - a == 1; // a single copy: circular when its origin is
        s2k_node_place rec;
        rec.unitig = (uint32_t)(2 * t) | s;
        rec.pos = s ? Lc - f - m : f;
        rec.len = Lc;
        rec.circular = o.circular[t] || (alone && in.circular[origin[o.members[a] >> 1]]);
        place[C >> 1] = rec;
    }
}

// ---- the lift ------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t LIFT_NONE = 0xFFFFFFFFu; // no contig: the step is dropped, or there is no such step (a contig id stays below it)

struct LiftIn {
    Paths p;
    const uint32_t *item, *start, *end, *matched_in;
    const uint64_t *uni_off;
    const uint8_t *circular;
    uint64_t n_unitigs;
    const uint8_t *resolved;
    const uint32_t *partner;
    const uint64_t *copy_off;
    const uint4 *place; // s2k_node_place records: unitig, pos, len, circular
    uint64_t n_copies, n_contigs;
};

struct LiftWs {
    uint8_t *join;   // per step
    uint32_t *copy;  // per step: its copy, S2K_NO_COPY when it is dropped
    uint64_t *C, *M; // n_steps + 1 each: the exclusive prefixes of count and of matched_in
    RunWs run;       // open: the tile's first step is joined to the step before it
};

__global__ __launch_bounds__(UT) void lift_check_kernel(LiftIn k, Csr g, uint64_t n_edges, uint32_t *__restrict__ bad) {
    const Paths &p = k.p;
    const uint64_t n_ids = 2 * k.n_unitigs;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(p.path_off, p.n_reads, p.n_steps, i0, stride);
    if (!steps_ok(p.unitig, p.pos, p.count, p.n_steps, k.uni_off, k.circular, n_ids, i0, stride)) ok = false;
    for (uint64_t u = i0; u < n_ids; u += stride) {
        if (!unitig_row_ok(g, k.uni_off, u, n_ids, n_edges)) ok = false;
        if (u & 1) continue;
        const uint64_t t = u >> 1, a = k.uni_off[t], b = k.uni_off[t + 1];
        const uint8_t r = k.resolved[t];
        if (r > 1) ok = false;
        const uint64_t ca = k.copy_off[t], cb = k.copy_off[t + 1];
        if ((t == 0 && ca != 0) || (t == k.n_unitigs - 1 && cb != k.n_copies) || ca >= cb || cb > k.n_copies) {
            ok = false;
            continue;
        }
        const uint64_t want = r ? g.row_off[u + 1] - g.row_off[u] : 1; // a wrong row bound has been reported above
        if (cb - ca != want) {
            ok = false;
            continue;
        }
        for (uint64_t c = ca; c < cb; c++) {
            const uint4 rec = k.place[c];
            if (rec.x >= 2 * k.n_contigs || (uint64_t)rec.y + (b - a) > rec.z || rec.w > 1) ok = false;
        }
    }
    if (!ok) atomicOr(bad, 1u);
}

// The copy of a step on U that its read enters over edge ein = (A -> U) and leaves over eout = (U -> B), SP_NONE where there is no
// such edge: S2K_NO_COPY when U >> 1 is resolved and there is neither.  *conflict: both exist and pick different copies.  A copy
// index outside its unitig can only come from an input whose twin symmetry or partners, which are trusted, do not hold: it becomes
// copy 0, and every access stays inside the arrays.
__device__ __forceinline__ uint32_t copy_of(const LiftIn &k, const Csr &g, uint32_t U, uint32_t ein, uint32_t A, uint32_t eout, uint32_t B, bool *conflict) {
    const uint64_t t = U >> 1, c0 = k.copy_off[t];
    *conflict = false;
    if (!k.resolved[t]) return (uint32_t)c0;
    if (ein == SP_NONE && eout == SP_NONE) return S2K_NO_COPY;
    const uint64_t base = g.row_off[2 * t + 1], n = k.copy_off[t + 1] - c0;
    uint64_t jin = 0, jout = 0;
    if (ein != SP_NONE) {
        const uint32_t x = (U & 1u) ? k.partner[ein] : find_edge(g, U ^ 1u, A ^ 1u); // odd: the edge that leaves 2 t + 1; even: tw(ein)
        jin = (uint64_t)x - base;
    }
    if (eout != SP_NONE) {
        uint32_t x = eout; // odd: it leaves 2 t + 1
        if (!(U & 1u)) {
            const uint32_t w = find_edge(g, B ^ 1u, U ^ 1u); // tw(eout) enters 2 t + 1
            x = w == SP_NONE ? SP_NONE : k.partner[w];
        }
        jout = (uint64_t)x - base;
    }
    *conflict = ein != SP_NONE && eout != SP_NONE && jin != jout;
    uint64_t j = ein != SP_NONE ? jin : jout;
    if (j >= n) j = 0;
    return (uint32_t)(c0 + j);
}

// where position ps of the oriented unitig U (m members) lies when the forward strand of its copy has the record rec
__device__ __forceinline__ void map_step(const uint4 rec, uint32_t U, uint32_t ps, uint32_t m, uint32_t *V, uint32_t *Q) {
    const uint32_t su = U & 1u;
    *V = rec.x ^ su;
    *Q = su ? rec.z - rec.y - m + ps : rec.y + ps;
}

// a step at (V, Q) on a contig of clen instances goes on where the step (pV, pQ) of pC items ended (both steps are kept)
__device__ __forceinline__ bool goes_on(uint32_t pV, uint32_t pQ, uint32_t pC, uint32_t V, uint32_t Q, uint32_t clen, bool circ) {
    if (pV != V) return false;
    uint64_t x = (uint64_t)pQ + pC;
    if (circ) x %= clen; // clen >= 1: the check pass
    return x == Q;
}

// a tile's lifted steps in LDS, indexed as FollowLds: index 0 is the step before the tile, index TB_TILE + 1 the one behind it
struct LiftLds {
    uint32_t V[TB_TILE + 2], Q[TB_TILE + 2], cnt[TB_TILE + 2]; // V == LIFT_NONE: dropped, or no such step
    uint8_t join[TB_TILE + 2];
};

__global__ __launch_bounds__(TB_THREADS) void lift_count_kernel(LiftIn k, Csr g, LiftWs ws, unsigned long long *__restrict__ totals /* merged, dropped, conflicts */) {
    __shared__ FollowLds s;
    __shared__ LiftLds l;
    const Paths &p = k.p;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint32_t U[TB_Q], ps[TB_Q], cnt[TB_Q], fl[TB_Q], e[TB_Q];
    uint64_t len[TB_Q];
    follow_tile(p, g, k.uni_off, t0, s, U, ps, cnt, fl, len, e);
    uint32_t n[3] = {0, 0, 0}; // merged, dropped, conflicts
    uint32_t V[TB_Q], Q[TB_Q], clen[TB_Q], circ = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        V[r] = LIFT_NONE, Q[r] = 0, clen[r] = 1;
        if (t0 + (i - 1) < p.n_steps) {
            bool cf;
            const uint32_t c = copy_of(k, g, U[r], e[r], s.U[i - 1], s.E[i + 1], s.U[i + 1], &cf);
            ws.copy[t0 + (i - 1)] = c;
            if (c != S2K_NO_COPY) {
                const uint4 rec = k.place[c];
                map_step(rec, U[r], ps[r], (uint32_t)len[r], &V[r], &Q[r]);
                clen[r] = rec.z;
                circ |= (rec.w ? 1u : 0u) << r;
                n[2] += cf;
            } else n[1]++;
        }
        l.V[i] = V[r], l.Q[i] = Q[r], l.cnt[i] = cnt[r];
        l.join[i] = 0;
    }
    if (tid == 0) l.join[0] = l.join[TB_TILE + 1] = 0;
    if (tid == 128) { // the step before the tile: its entering edge is the one search follow_tile has not made
        uint32_t hV = LIFT_NONE, hQ = 0, hC = 0;
        if (t0 > 0) {
            const uint64_t j = t0 - 1; // path_off[reads[0] - 1] <= j < path_off[reads[0]]
            const uint32_t hU = s.U[0], hp = p.pos[j];
            uint32_t ein = SP_NONE, A = 0;
            hC = p.count[j];
            if (j > 0 && p.path_off[s.reads[0] - 1] != j && (p.flags[j] & S2K_STEP_LINKED) && hp == 0) {
                A = p.unitig[j - 1];
                if ((uint64_t)p.pos[j - 1] + p.count[j - 1] == k.uni_off[(A >> 1) + 1] - k.uni_off[A >> 1]) ein = find_edge(g, A, hU);
            }
            bool cf;
            const uint32_t c = copy_of(k, g, hU, ein, A, s.E[1], s.U[1], &cf);
            if (c != S2K_NO_COPY) map_step(k.place[c], hU, hp, (uint32_t)(k.uni_off[(hU >> 1) + 1] - k.uni_off[hU >> 1]), &hV, &hQ);
        }
        l.V[0] = hV, l.Q[0] = hQ, l.cnt[0] = hC;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        if (e[r] != SP_NONE && V[r] != LIFT_NONE && l.V[i - 1] != LIFT_NONE &&
            goes_on(l.V[i - 1], l.Q[i - 1], l.cnt[i - 1], V[r], Q[r], clen[r], (circ >> r) & 1u)) {
            l.join[i] = 1;
            n[0]++;
        }
        if (t0 + (i - 1) < p.n_steps) ws.join[t0 + (i - 1)] = l.join[i];
    }
    if (tid == 0 && s.E[TB_TILE + 1] != SP_NONE && l.V[TB_TILE] != LIFT_NONE) { // the step behind the tile: its entering edge picks its copy
        const uint32_t hU = s.U[TB_TILE + 1];
        bool cf;
        const uint32_t c = copy_of(k, g, hU, s.E[TB_TILE + 1], s.U[TB_TILE], SP_NONE, 0u, &cf);
        const uint4 rec = k.place[c];
        uint32_t hV, hQ;
        map_step(rec, hU, 0u, (uint32_t)(k.uni_off[(hU >> 1) + 1] - k.uni_off[hU >> 1]), &hV, &hQ); // a step that follows an edge begins at 0
        l.join[TB_TILE + 1] = goes_on(l.V[TB_TILE], l.Q[TB_TILE], l.cnt[TB_TILE], hV, hQ, rec.z, rec.w != 0);
    }
    __syncthreads();
    auto kept = [&](int r) { return V[r] != LIFT_NONE; }; // never on a step past n_steps
    run_count_end(
        ws.run, t0, p.n_steps, [&](int r, int i) { return kept(r) && l.join[i] != 1; }, [&](int r, int i) { return kept(r) && l.join[i + 1] != 1; },
        [&] { return l.join[1] == 1; });
    block_add(n, totals);
}

struct LiftOut {
    uint32_t *unitig, *pos, *count, *item, *flags, *start, *end, *matched;
};

__global__ __launch_bounds__(TB_THREADS) void lift_write_kernel(LiftIn k, LiftOut io, LiftWs ws) {
    __shared__ uint4 stage4[(TB_TILE + 2 * STAGE_PAD) / 4]; // TB_TILE 32-bit elements, and a run's shift
    const Paths &p = k.p;
    const int tid = threadIdx.x;
    RunTile rt;
    if (!run_tile(ws.run, p.n_steps, rt)) return;
    const uint64_t t0 = rt.t0;
    uint64_t hd[TB_Q];
    uint32_t oV[TB_Q], opos[TB_Q], ocnt[TB_Q], omat[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        hd[r] = 0, oV[r] = opos[r] = ocnt[r] = omat[r] = 0;
        if ((rt.tkeep >> r) & 1u) {
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
            const uint64_t h = rt.head_of(r);
            const uint32_t Uh = p.unitig[h];
            hd[r] = h;
            map_step(k.place[ws.copy[h]], Uh, p.pos[h], (uint32_t)(k.uni_off[(Uh >> 1) + 1] - k.uni_off[Uh >> 1]), &oV[r], &opos[r]);
            ocnt[r] = (uint32_t)(ws.C[j + 1] - ws.C[h]);
            omat[r] = io.matched && k.matched_in ? (uint32_t)(ws.M[j + 1] - ws.M[h]) : ocnt[r]; // M is scanned only when both are given
        }
    }
    rt.leave_tails(io.unitig, stage4, [&](int r, uint64_t) { return oV[r]; });
    rt.leave_tails(io.pos, stage4, [&](int r, uint64_t) { return opos[r]; });
    rt.leave_tails(io.count, stage4, [&](int r, uint64_t) { return ocnt[r]; });
    rt.leave_tails(io.item, stage4, [&](int r, uint64_t) { return k.item[hd[r]]; });
    rt.leave_tails(io.flags, stage4, [&](int r, uint64_t) { return p.flags[hd[r]]; });
    rt.leave_tails(io.start, stage4, [&](int r, uint64_t) { return k.start[hd[r]]; });
    rt.leave_tails(io.end, stage4, [&](int, uint64_t j) { return k.end[j]; });
    rt.leave_tails(io.matched, stage4, [&](int r, uint64_t) { return omat[r]; });
}

// contig_items[V >> 1] += count of every kept step: the steps of a run lie on one contig, so the sums are those over the output steps
__global__ __launch_bounds__(UT) void lift_items_kernel(LiftIn k, const uint32_t *__restrict__ copy, unsigned long long *__restrict__ items) {
    for (uint64_t s = (uint64_t)blockIdx.x * UT + threadIdx.x; s < k.p.n_steps; s += (uint64_t)gridDim.x * UT) {
        const uint32_t c = copy[s];
        if (c != S2K_NO_COPY) atomicAdd(items + (k.place[c].x >> 1), (unsigned long long)k.p.count[s]);
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_unitig_copy_places(s2k_ctx *ctx, const uint64_t *d_outer_off, const uint32_t *d_outer_members, const uint8_t *d_outer_circular,
                                  uint64_t n_contigs, uint64_t n_copies, const uint32_t *d_origin, const uint64_t *d_uni_off, const uint8_t *d_circular,
                                  uint64_t n_unitigs, s2k_node_place *d_copy_place) {
    if (!ctx) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_unitig_copy_places");
    if (n_copies >= (1ull << 31) || n_contigs > n_copies || n_unitigs >= (1ull << 31))
        return c.invalid("2^31 copies or unitigs or more (oriented ids are 32-bit), or more contigs than copies");
    if (n_copies == 0) return S2K_OK; // no copies: no records
    if (n_contigs == 0 || n_unitigs == 0) return c.invalid("copies without contigs or without unitigs");
    if (!d_outer_off || !d_outer_members || !d_outer_circular || !d_origin || !d_uni_off || !d_circular || !d_copy_place) return S2K_ERR_INVALID_ARG;
    if ((uintptr_t)d_copy_place & 15u) return c.invalid("copy records that are not 16-byte aligned");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const auto len_p = L.take<uint32_t>(n_copies);
    const auto slot_p = L.take<uint32_t>(n_copies);
    const auto off_p = L.take<uint64_t>(n_copies + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_copies));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint32_t *bad = flag(w);
    const PlaceWs p{len_p(w), slot_p(w), off_p(w)};
    const Outer outer{d_outer_off, d_outer_members, d_outer_circular, n_contigs, n_copies};
    const Inner inner{d_uni_off, d_circular, n_unitigs};
    const uint32_t hbad = c.check(bad, 16, bad, [&] {
        hipLaunchKernelGGL(places_check_kernel, dim3(grid_for(std::max(n_copies, n_unitigs) + 1)), dim3(UT), 0, c.st, outer, inner, d_origin, p, bad);
        c.launched();
        if (c.ok()) hipLaunchKernelGGL(places_verify_kernel, dim3(grid_for(n_copies)), dim3(UT), 0, c.st, outer, p, bad);
        c.launched();
        c.scan(p.len, n_copies, p.off, tmp_p(w));
        if (c.ok()) hipLaunchKernelGGL(places_contig_kernel, dim3(grid_for(n_contigs)), dim3(UT), 0, c.st, outer, p, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("uni_off (inner or outer) that does not ascend strictly from 0 (the outer one to n_copies), an outer member >= 2 * n_copies, a "
                         "copy that is not named by exactly one outer member, an origin >= n_unitigs, or a unitig or a contig of 2^32 members or more");
    hipLaunchKernelGGL(places_write_kernel, dim3(grid_for(n_copies)), dim3(UT), 0, c.st, outer, inner, d_origin, p, d_copy_place);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_paths_lift(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint32_t *d_matched_in,
                          const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular,
                          uint64_t n_unitigs, const uint8_t *d_resolved, const uint32_t *d_partner, const uint64_t *d_copy_off,
                          const s2k_node_place *d_copy_place, uint64_t n_copies, uint64_t n_contigs, const s2k_thread_out *out, uint32_t *d_matched,
                          uint32_t *d_step_copy, uint8_t *d_join, uint64_t *d_contig_items, uint64_t *n_out_steps, uint64_t *n_merged,
                          uint64_t *n_dropped, uint64_t *n_conflicts) {
    if (n_out_steps) *n_out_steps = 0;
    if (n_merged) *n_merged = 0;
    if (n_dropped) *n_dropped = 0;
    if (n_conflicts) *n_conflicts = 0;
    if (!ctx || !out || !n_out_steps || !n_merged || !n_dropped || !n_conflicts || !paths_given(paths, n_steps, true) || !out->path_off)
        return S2K_ERR_INVALID_ARG;
    if (n_steps && ((out->start && !paths->start) || (out->end && !paths->end))) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_paths_lift");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32) || n_copies >= (1ull << 31))
        return c.invalid("2^31 unitigs or copies or more (oriented ids are 32-bit), or 2^32 edges or more (an edge index is 32-bit)");
    if (n_unitigs == 0 && (n_edges || n_copies)) return c.invalid("edges or copies without unitigs");
    if (n_copies < n_unitigs || n_contigs > n_copies || (n_copies && !n_contigs)) return c.invalid("fewer copies than unitigs, more contigs than copies, or no contig");
    if (n_unitigs && (!d_row_off || !d_uni_off || !d_circular || !d_resolved || !d_copy_off || !d_copy_place || (n_edges && (!d_dst || !d_partner))))
        return S2K_ERR_INVALID_ARG;
    if ((uintptr_t)d_copy_place & 15u) return c.invalid("copy records that are not 16-byte aligned");
    const uint64_t nt = (n_steps + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many steps for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto words = L.bytes<unsigned long long>(64); // merged, dropped, conflicts; then the flag
    const auto join = L.take<uint8_t>(n_steps);
    const auto copy = L.take<uint32_t>(n_steps);
    const auto C = L.take<uint64_t>(n_steps + 1);
    const auto M = L.take<uint64_t>(n_steps + 1);
    const auto stmp = L.bytes<uint64_t>(scan_tmp_bytes(n_steps));
    const auto runs = carve_runs(L, n_steps, nt);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *totals = words(w);
    uint32_t *bad = (uint32_t *)(totals + 3);
    const LiftWs ws{join(w), copy(w), C(w), M(w), runs(w)};
    const LiftIn k{paths_of(paths, n_reads, n_steps),
                   paths->item,
                   paths->start,
                   paths->end,
                   d_matched_in,
                   d_uni_off,
                   d_circular,
                   n_unitigs,
                   d_resolved,
                   d_partner,
                   d_copy_off,
                   (const uint4 *)d_copy_place,
                   n_copies,
                   n_contigs};
    const Csr g{d_row_off, d_dst};
    const uint32_t hbad = c.check(totals, 32, bad, [&] {
        hipLaunchKernelGGL(lift_check_kernel, dim3(grid_for(std::max(std::max(n_reads + 1, n_steps), 2 * n_unitigs))), dim3(UT), 0, c.st, k, g, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("path_off that does not run from 0 to n_steps without decreasing, a step on a unitig >= n_unitigs, without items or outside its "
                         "unitig, not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, uni_off that does not ascend strictly, a "
                         "unitig of 2^32 members or more, a resolved byte above 1, copy_off that does not run from 0 to n_copies with out(2 t) copies of a "
                         "resolved unitig and one of any other, or a copy record outside the contigs or too short for its unitig");
    if (n_steps == 0) { // no steps: none come out
        c.zero(out->path_off, (n_reads + 1) * 8);
        if (!c.sync()) return c.device_error();
        return S2K_OK;
    }
    uint64_t total = 0;
    unsigned long long h[3] = {0, 0, 0};
    if (!count_runs(c, ws.run, nt, runs.h.scan_tmp(w), [&] { hipLaunchKernelGGL(lift_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, k, g, ws, totals); },
                    &total, totals, h, 3))
        return c.device_error();
    *n_out_steps = total;
    *n_merged = h[0];
    *n_dropped = h[1];
    *n_conflicts = h[2];
    const bool records = out->unitig || out->pos || out->count || out->item || out->flags || out->start || out->end || d_matched;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (d_join) c.copy(d_join, ws.join, n_steps, hipMemcpyDeviceToDevice);
    if (d_step_copy) c.copy(d_step_copy, ws.copy, n_steps * 4, hipMemcpyDeviceToDevice);
    if (c.ok()) launch_run_offsets(c, paths->path_off, n_reads, n_steps, nt, ws.run, out->path_off);
    if (records && total) {
        c.scan(paths->count, n_steps, ws.C, stmp(w));
        if (d_matched && d_matched_in) c.scan(d_matched_in, n_steps, ws.M, stmp(w));
        const LiftOut io{out->unitig, out->pos, out->count, out->item, out->flags, out->start, out->end, d_matched};
        if (c.ok()) {
            hipLaunchKernelGGL(lift_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, k, io, ws);
            c.launched();
        }
    }
    if (d_contig_items && c.ok()) {
        hipLaunchKernelGGL(lift_items_kernel, dim3(grid_for(n_steps)), dim3(UT), 0, c.st, k, ws.copy, (unsigned long long *)d_contig_items);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

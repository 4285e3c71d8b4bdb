// s2k_segment.hip -- long read walks aligned piece by piece: the walks cut into segment pairs at anchor k-min-mers, and the segments'
// CIGARs joined back into one alignment per walk (include/s2k.h: s2k_walks_segments, s2k_align_join).
// s2k_align_pairs (s2k_align.hip) aligns the segments in between and is not touched.
//
// s2k_walks_segments.  Items are the items of the SOURCE steps in order (the exclusive scan C of src->count: item t lies in the
// source step r with C[r] <= t < C[r + 1]), in tiles of TB_TILE (lane tid holds items q * 256 + tid, s2k_compact_dev.h):
//  1. tg_check_kernel (s2k_targets_dev.h) and sg_check_kernel: the shared rules of s2k_span_dev.h (path_off_ok, steps_ok) and
//     s2k_coords_dev.h (lift_unitig_ok, lift_member_ok), and the rules of the walks, the targets and km_off.  One flag word, read by
//     the host with C's total before anything else runs.
//  2. tg_steps_kernel and launch_scan_u32: the per-step prefix G of adv, as the targets have it.
//  3. sg_steps_kernel, one lane per source step: its read (a search of src->path_off), the read's first item of it, the walk that
//     holds its step (a search of first_step; SG_NONE when the whole step is outside); the rules of item and src_step.
//  4. sg_items_kernel, one lane per item: its source step by a search of C inside the tile's range, outside or candidate, (qc, tc),
//     each clamped to 32 bits (a value at or past either end is inadmissible and stops every later one, clamped or not) and stored
//     under the walk: word = (w + 1) << 32 | value, 0 for an item outside.  Walks come in read order, so a plain max-scan over these
//     words IS the segmented one: a maximum from an earlier walk is below every word of this one.  The tile's two maxima.
//  5. sg_tiles_kernel, one workgroup: the exclusive max-scan over the tiles' maxima.
//  6. sg_admit_kernel: the exclusive max-scan inside the tile, seeded with the tile's entry; admissible = inside (0, m) x (0, n) and
//     above both running maxima; a maximum from a LATER walk raises the flag.  Ballots: the admissible mask (tile_prefixes).
//  7. launch_scan_u32 over the tiles; the host reads the flag, the counters and the number of admissible anchors.
//  8. sg_keep_kernel: walk, qc, tc of the admissible anchors, compacted (tile_slots, leave_field).
//  9. sg_heads_kernel over the compacted stream: chosen = bucket >= 1 and another walk or bucket than the anchor before it.  Ballots,
//     launch_scan_u32; the host reads the total and answers the sizes call and the capacity.
// 10. sg_chosen_kernel: the chosen anchors compacted; sg_off_kernel, one lane per walk: seg_off[w] = w + the chosen anchors of walks
//     before w (a search: the chosen are sorted by walk); sg_segments_kernel, one lane per segment, output-ordered.
//
// s2k_align_join.  Slots are the run slots of the segments, ops_off[0] .. ops_off[n_segments), in the same tiles:
//  1. jn_check_kernel: seg_off, ops_off, n_ops (ops_off_ok and the run word: s2k_cigar_dev.h).  The host reads the flag and the two
//     ends of ops_off.
//  2. jn_over_kernel and three launch_scan_u32 over the segments: edits, matches, over.
//  3. jn_slots_kernel, one lane per slot: its segment and walk by searches; a run of a walk that is neither bad nor over is kept, and
//     is a head unless it is the first run of a segment after the walk's first whose op equals the last run's of the segment before.
//     The kept lengths to the workspace, the head mask by ballots.  launch_scan_u32 over the lengths (LP) and over the tiles.
//  4. jn_heads_kernel: per head LP at its slot and its op, compacted; LP's total closes the list.  jn_lens_kernel: a head's length is
//     the difference of two neighbours; 2^28 or more, or a walk whose sums pass 32 bits, raises the flag, which the host reads.
//  5. jn_walks_kernel, one lane per walk (ops_off = the heads before the walk's first slot: kept_before), jn_ops_kernel, one lane per
//     joined run.
//
// Workspace (the context's grow-only count workspace).  Segments: per item 28 B (two scanned words 8 + 8, which the chosen anchors
// reuse, and the compacted walk, qc, tc 4 + 4 + 4), per 64 items twice 8 + 4 B and per tile twice 4 + 8 B for the two masks and 16 B
// for the maxima; per source step 20 B (walk 4, first item 8, C 8); per step of the paths 16 B (adv 4, broken 4, G 8); per walk 8 B
// (seg_off).  Join: per slot 24 B (length 4, LP 8; LP 8 and op 4 of the joined runs, sized by the slots) and the mask's 12 B per 64 slots
// and per tile; per segment 28 B (over 4, three prefixes 8 each).
#include <algorithm>
#include <cstring>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_cigar_dev.h"
#include "s2k_compact_dev.h"
#include "s2k_coords_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_runs_dev.h"
#include "s2k_span_dev.h"
#include "s2k_targets_dev.h"

namespace s2k {
namespace {

constexpr uint32_t SG_NONE = NONE; // a source step none of whose items can be a candidate
constexpr int SG_WORDS = 8;        // the flag word, then the counters of a call
enum { SW_BAD = 0, SW_CAND, SW_OUTSIDE, SW_ADM, SW_CUT };
static_assert(SW_CUT < SG_WORDS && S2K_SEGMENT_STATS <= SG_WORDS, "the counters fit the words");
static_assert(TG_T == TB_THREADS && UT == TB_THREADS, "block_add and the tiles share one block size");

struct SgIn {
    const uint64_t *walk_off, *first_step, *path_start; // the walks
    const uint32_t *n_steps, *qstart, *qend, *wflags;
    uint64_t n_reads, n_walks;
    const uint32_t *unitig, *pos, *count; // the steps of the walks' paths
    uint64_t n_all_steps;
    const uint64_t *q_begin, *tgt_off; // per walk
    const uint8_t *bad;
    const uint64_t *src_off; // the source paths
    const uint32_t *src_pos, *src_count, *src_item;
    const uint64_t *src_step; // nullptr: the identity
    uint64_t n_src;
    const uint64_t *km_off;
    const uint32_t *start;
    uint32_t seg_len;
};

struct SgWs {
    uint32_t *stepw;    // per source step: the walk of its step, SG_NONE when all its items are outside
    uint64_t *stepj;    // per source step: the read's first item of it, absolute in the batch
    uint64_t *C, *G;    // n_src + 1: items before a source step; n_all_steps + 1: adv before a step
    uint64_t *KQ, *KT;  // per item: (w + 1) << 32 | qc, | tc; 0 outside
    uint64_t *TQ, *TT;  // per tile: the maxima, then their exclusive max-scan
    uint32_t *aw, *aq, *at; // the admissible anchors
    uint32_t *cw, *cq, *ct; // the chosen anchors (in the words of KQ and KT)
    uint64_t *seg_off;
};

__device__ __forceinline__ uint64_t step_of(const SgIn &in, uint64_t r) { return in.src_step ? in.src_step[r] : r; }

__global__ __launch_bounds__(UT) void sg_check_kernel(SgIn in, Lift v, uint32_t *__restrict__ bad) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(in.walk_off, in.n_reads, in.n_walks, i0, stride);
    if (!path_off_ok(in.src_off, in.n_reads, in.n_src, i0, stride)) ok = false;
    if (!steps_ok(in.unitig, in.pos, in.count, in.n_all_steps, v.uni_off, v.circular, 2 * v.n_unitigs, i0, stride)) ok = false;
    for (uint64_t t = i0; t < v.n_unitigs; t += stride)
        if (!lift_unitig_ok(v, t)) ok = false;
    for (uint64_t x = i0; x < v.n_nodes; x += stride)
        if (!lift_member_ok(v, x)) ok = false;
    for (uint64_t R = i0; R < in.n_reads; R += stride)
        if (in.km_off[R] > in.km_off[R + 1]) ok = false;
    for (uint64_t w = i0; w < in.n_walks; w += stride) {
        // (tg_check_kernel: first_step + n_steps stays inside the paths, so the sum cannot wrap)
        if (w + 1 < in.n_walks && in.first_step[w] + in.n_steps[w] > in.first_step[w + 1]) ok = false;
        if (in.qstart[w] > in.qend[w]) ok = false;
        const uint64_t a = in.tgt_off[w], b = in.tgt_off[w + 1];
        if (a > b || b - a >= (1ull << 32)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void sg_steps_kernel(SgIn in, SgWs ws, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t r = i0; r < in.n_src; r += stride) {
        const uint64_t R = last_le(in.src_off, 0, in.n_reads, r); // src_off[n_reads] = n_src > r: R < n_reads
        const uint64_t j0 = in.km_off[R] + in.src_item[r];
        if (j0 + in.src_count[r] > in.km_off[R + 1]) ok = false;
        const uint64_t S = step_of(in, r);
        uint32_t w = SG_NONE;
        if (S != S2K_NO_STEP) {
            if (S >= in.n_all_steps) ok = false;
            else if (in.n_walks) {
                const uint64_t x = last_le(in.first_step, 0, in.n_walks - 1, S);
                const uint64_t f = in.first_step[x];
                if (f <= S && S - f < in.n_steps[x]) {
                    if (x < in.walk_off[R] || x >= in.walk_off[R + 1]) ok = false;
                    else if (!(in.wflags[x] & S2K_WALK_CIRCULAR) && !in.bad[x]) w = (uint32_t)x;
                }
            }
            if (r > in.src_off[R]) {
                const uint64_t P = step_of(in, r - 1);
                if (P != S2K_NO_STEP && P > S) ok = false;
            }
        }
        ws.stepw[r] = w;
        ws.stepj[r] = j0;
    }
    if (!ok) atomicOr(bad, 1u);
}

// the maxima of a and b over the workgroup, in every lane; part: 2 * 4 words of LDS
__device__ __forceinline__ void block_max2(uint64_t &a, uint64_t &b, uint64_t (*part)[2]) {
    for (int o = 32; o > 0; o >>= 1) {
        a = std::max<uint64_t>(a, __shfl_xor(a, o, 64));
        b = std::max<uint64_t>(b, __shfl_xor(b, o, 64));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][0] = a, part[threadIdx.x >> 6][1] = b;
    __syncthreads();
    a = b = 0;
    for (int j = 0; j < TB_THREADS / 64; j++) a = std::max(a, part[j][0]), b = std::max(b, part[j][1]);
    __syncthreads();
}

// a, b <- the maxima over the lanes before this one and the carries *ca, *cb; the carries gain the workgroup's maxima.  Two
// barriers; part: 2 * 4 words of LDS
__device__ __forceinline__ void block_excl_max2(uint64_t &a, uint64_t &b, uint64_t &ca, uint64_t &cb, uint64_t (*part)[2]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t ya = __shfl_up(ia, o, 64), yb = __shfl_up(ib, o, 64);
        if (lane >= o) ia = std::max(ia, ya), ib = std::max(ib, yb);
    }
    if (lane == 63) part[wv][0] = ia, part[wv][1] = ib;
    uint64_t ea = __shfl_up(ia, 1, 64), eb = __shfl_up(ib, 1, 64);
    if (lane == 0) ea = eb = 0;
    __syncthreads();
    uint64_t ta = ca, tb = cb;
#pragma unroll
    for (int j = 0; j < TB_THREADS / 64; j++) {
        if (j == wv) ea = std::max(ea, ta), eb = std::max(eb, tb);
        ta = std::max(ta, part[j][0]), tb = std::max(tb, part[j][1]);
    }
    __syncthreads();
    a = ea, b = eb, ca = ta, cb = tb;
}

__global__ __launch_bounds__(TB_THREADS) void sg_items_kernel(SgIn in, Lift v, SgWs ws, uint64_t n_items, unsigned long long *__restrict__ words) {
    __shared__ uint64_t srange[2], part[TB_THREADS / 64][2];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    if (tid < 2) srange[tid] = last_le(ws.C, 0, in.n_src - 1, tid ? std::min<uint64_t>(t0 + TB_TILE, n_items) - 1 : t0);
    __syncthreads();
    unsigned long long n[2] = {0, 0}; // candidates, outside
    uint64_t mq = 0, mt = 0;
    for (int q = 0; q < TB_Q; q++) {
        const uint64_t t = t0 + (uint64_t)q * TB_THREADS + tid;
        if (t >= n_items) break;
        const uint64_t r = last_le(ws.C, srange[0], srange[1], t), i = t - ws.C[r];
        const uint32_t w = ws.stepw[r];
        uint64_t kq = 0, kt = 0;
        if (w != SG_NONE) {
            const uint64_t S = step_of(in, r), x = (uint64_t)in.src_pos[r] + i;
            const uint32_t U = in.unitig[S];
            const uint64_t p0 = in.pos[S], len = v.uni_off[(U >> 1) + 1] - v.uni_off[U >> 1];
            if (x >= p0 && x - p0 < in.count[S] && x < len) {
                uint64_t lo, hi, L, wr;
                interval(v, U, x, &lo, &hi, &L, &wr);
                const uint64_t a = ws.G[S] - ws.G[in.first_step[w]] + lo, ps = in.path_start[w];
                const uint64_t st = in.start[ws.stepj[r] + i], qs = in.qstart[w];
                const uint64_t tc = a <= ps ? 0 : std::min<uint64_t>(a - ps, 0xFFFFFFFFull), qc = st <= qs ? 0 : st - qs;
                kq = ((uint64_t)w + 1) << 32 | qc;
                kt = ((uint64_t)w + 1) << 32 | tc;
            }
        }
        n[kq ? 0 : 1]++;
        ws.KQ[t] = kq;
        ws.KT[t] = kt;
        mq = std::max(mq, kq), mt = std::max(mt, kt);
    }
    block_max2(mq, mt, part);
    if (tid == 0) ws.TQ[blockIdx.x] = mq, ws.TT[blockIdx.x] = mt;
    block_add(n, words + SW_CAND);
}

__global__ __launch_bounds__(TB_THREADS) void sg_tiles_kernel(SgWs ws, uint64_t n_tiles) {
    __shared__ uint64_t part[TB_THREADS / 64][2];
    uint64_t ca = 0, cb = 0;
    for (uint64_t base = 0; base < n_tiles; base += TB_THREADS) {
        const uint64_t i = base + threadIdx.x;
        uint64_t a = i < n_tiles ? ws.TQ[i] : 0, b = i < n_tiles ? ws.TT[i] : 0;
        block_excl_max2(a, b, ca, cb, part);
        if (i < n_tiles) ws.TQ[i] = a, ws.TT[i] = b;
    }
}

__global__ __launch_bounds__(TB_THREADS) void sg_admit_kernel(SgIn in, SgWs ws, uint64_t n_items, CompactWs cw, unsigned long long *__restrict__ words) {
    __shared__ uint64_t part[TB_THREADS / 64][2];
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint64_t ca = ws.TQ[blockIdx.x], cb = ws.TT[blockIdx.x];
    unsigned long long n_adm = 0;
    bool ok = true;
    for (int q = 0; q < TB_Q; q++) { // the rounds in item order: the carries run through them
        const uint64_t t = t0 + (uint64_t)q * TB_THREADS + tid;
        const uint64_t kq = t < n_items ? ws.KQ[t] : 0, kt = t < n_items ? ws.KT[t] : 0;
        uint64_t pq = kq, pt = kt;
        block_excl_max2(pq, pt, ca, cb, part);
        bool adm = false;
        if (kq) {
            if ((pq >> 32) > (kq >> 32)) ok = false; // a candidate of a later walk came first
            const uint64_t w = (kq >> 32) - 1, qc = kq & 0xFFFFFFFFull, tc = kt & 0xFFFFFFFFull;
            const uint64_t m = in.qend[w] - in.qstart[w], nt = in.tgt_off[w + 1] - in.tgt_off[w];
            adm = qc > 0 && qc < m && tc > 0 && tc < nt && pq < kq && pt < kt;
        }
        n_adm += adm;
        tile_ballot(wc, q, t0, n_items, cw, adm);
    }
    if (!ok) atomicOr((uint32_t *)(words + SW_BAD), 2u);
    __syncthreads();
    tile_prefixes(wc, t0, n_items, cw);
    block_add(n_adm, words + SW_ADM);
}

__global__ __launch_bounds__(TB_THREADS) void sg_keep_kernel(SgWs ws, uint64_t n_items, CompactWs cw) {
    __shared__ uint4 stage4[(TB_TILE + STAGE_PAD) / 2];
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, base = cw.tile_off[blockIdx.x];
    const uint32_t tot = (uint32_t)(cw.tile_off[blockIdx.x + 1] - base);
    if (tot == 0) return;
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(cw, t0, n_items, slot);
    leave_field(ws.aw, base, keep, slot, tot, stage4, [&](int, uint64_t t) { return (uint32_t)(ws.KQ[t] >> 32) - 1u; });
    leave_field(ws.aq, base, keep, slot, tot, stage4, [&](int, uint64_t t) { return (uint32_t)ws.KQ[t]; });
    leave_field(ws.at, base, keep, slot, tot, stage4, [&](int, uint64_t t) { return (uint32_t)ws.KT[t]; });
}

__global__ __launch_bounds__(TB_THREADS) void sg_heads_kernel(SgWs ws, uint64_t n_adm, uint32_t seg_len, CompactWs ch) {
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
#pragma unroll
    for (int q = 0; q < TB_Q; q++) {
        const uint64_t i = t0 + (uint64_t)q * TB_THREADS + tid;
        bool head = false;
        if (i < n_adm) {
            const uint32_t b = ws.aq[i] / seg_len;
            head = b >= 1 && (i == 0 || ws.aw[i - 1] != ws.aw[i] || ws.aq[i - 1] / seg_len != b);
        }
        tile_ballot(wc, q, t0, n_adm, ch, head);
    }
    __syncthreads();
    tile_prefixes(wc, t0, n_adm, ch);
}

__global__ __launch_bounds__(TB_THREADS) void sg_chosen_kernel(SgWs ws, uint64_t n_adm, CompactWs ch) {
    __shared__ uint4 stage4[(TB_TILE + STAGE_PAD) / 2];
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, base = ch.tile_off[blockIdx.x];
    const uint32_t tot = (uint32_t)(ch.tile_off[blockIdx.x + 1] - base);
    if (tot == 0) return;
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ch, t0, n_adm, slot);
    leave_field(ws.cw, base, keep, slot, tot, stage4, [&](int, uint64_t i) { return ws.aw[i]; });
    leave_field(ws.cq, base, keep, slot, tot, stage4, [&](int, uint64_t i) { return ws.aq[i]; });
    leave_field(ws.ct, base, keep, slot, tot, stage4, [&](int, uint64_t i) { return ws.at[i]; });
}

// the chosen anchors of walks before w (cw ascends)
__device__ inline uint64_t chosen_before(const uint32_t *__restrict__ cw, uint64_t n_chosen, uint64_t w) {
    uint64_t lo = 0, hi = n_chosen;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (cw[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(UT) void sg_off_kernel(SgWs ws, uint64_t n_walks, uint64_t n_chosen, unsigned long long *__restrict__ words) {
    unsigned long long cut = 0;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t w = i0; w <= n_walks; w += stride) {
        const uint64_t a = chosen_before(ws.cw, n_chosen, w);
        ws.seg_off[w] = w + a;
        cut += w < n_walks && a < n_chosen && ws.cw[a] == w;
    }
    block_add(cut, words + SW_CUT);
}

__global__ __launch_bounds__(UT) void sg_segments_kernel(SgIn in, SgWs ws, uint64_t n_segments, s2k_segment_out out) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t s = i0; s < n_segments; s += stride) {
        const uint64_t w = last_le(ws.seg_off, 0, in.n_walks - 1, s); // seg_off ascends strictly from 0
        const uint64_t k = s - ws.seg_off[w], a = ws.seg_off[w + 1] - ws.seg_off[w] - 1, c0 = ws.seg_off[w] - w;
        const uint64_t qb = in.q_begin[w], tb = in.tgt_off[w];
        const bool bad = in.bad[w] != 0;
        const uint64_t m = bad ? 0 : in.qend[w] - in.qstart[w], n = bad ? 0 : in.tgt_off[w + 1] - tb;
        if (out.q_begin) out.q_begin[s] = qb + (k ? ws.cq[c0 + k - 1] : 0);
        if (out.t_begin) out.t_begin[s] = tb + (k ? ws.ct[c0 + k - 1] : 0);
        if (out.q_end) out.q_end[s] = qb + (k < a ? ws.cq[c0 + k] : m);
        if (out.t_end) out.t_end[s] = tb + (k < a ? ws.ct[c0 + k] : n);
    }
}

// ---- join ----------------------------------------------------------------------------------------------------------------------------
struct JnIn {
    const uint64_t *seg_off;
    const uint8_t *bad;
    uint64_t n_walks, n_segs;
    const uint32_t *edits, *flags, *n_ops, *matches, *ops;
    const uint64_t *ops_off;
    uint64_t n_ops_total;
};

struct JnWs {
    uint32_t *ov;         // per segment: it is over
    uint64_t *E, *M, *OV; // n_segs + 1: the prefixes of edits, matches, over
    uint32_t *len;        // per slot: the length of a kept run, 0 elsewhere
    uint64_t *LP;         // n_slots + 1: its prefix
    uint64_t *HLP;        // per head, and one more: LP at its slot; LP's total
    uint32_t *hop;        // per head: its op
};

__global__ __launch_bounds__(UT) void jn_check_kernel(JnIn in, uint32_t *__restrict__ bad) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    bool ok = path_off_ok(in.seg_off, in.n_walks, in.n_segs, i0, stride);
    if (!ops_off_ok(in.ops_off, in.n_ops, in.n_segs, in.n_ops_total, i0, stride)) ok = false;
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void jn_over_kernel(JnIn in, uint32_t *__restrict__ ov) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t s = i0; s < in.n_segs; s += stride) ov[s] = in.flags[s] & S2K_ALIGN_OVER ? 1u : 0u;
}

// walk w is neither bad nor over: its runs are joined
__device__ __forceinline__ bool joined(const JnIn &in, const JnWs &ws, uint64_t w) {
    return !in.bad[w] && ws.OV[in.seg_off[w + 1]] == ws.OV[in.seg_off[w]];
}

__global__ __launch_bounds__(TB_THREADS) void jn_slots_kernel(JnIn in, JnWs ws, uint64_t r0, uint64_t n_slots, CompactWs ch, uint32_t *__restrict__ bad) {
    __shared__ uint64_t srange[2];
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    if (tid < 2) srange[tid] = last_le(in.ops_off, 0, in.n_segs - 1, r0 + (tid ? std::min<uint64_t>(t0 + TB_TILE, n_slots) - 1 : t0));
    __syncthreads();
    bool ok = true;
    for (int q = 0; q < TB_Q; q++) {
        const uint64_t i = t0 + (uint64_t)q * TB_THREADS + tid;
        bool head = false;
        if (i < n_slots) {
            const uint64_t r = r0 + i, s = last_le(in.ops_off, srange[0], srange[1], r), k = r - in.ops_off[s];
            const uint64_t w = last_le(in.seg_off, 0, in.n_walks - 1, s);
            uint32_t ln = 0;
            if (k < in.n_ops[s] && joined(in, ws, w)) {
                const uint32_t v = in.ops[r];
                ln = run_len(v);
                if (!run_legal(v)) ok = false;
                head = true;
                if (k == 0 && s > in.seg_off[w] && in.n_ops[s - 1]) head = run_op(in.ops[in.ops_off[s - 1] + in.n_ops[s - 1] - 1]) != run_op(v);
            }
            ws.len[i] = ln;
        }
        tile_ballot(wc, q, t0, n_slots, ch, head);
    }
    if (!ok) atomicOr(bad, 1u);
    __syncthreads();
    tile_prefixes(wc, t0, n_slots, ch);
}

__global__ __launch_bounds__(TB_THREADS) void jn_heads_kernel(JnIn in, JnWs ws, uint64_t r0, uint64_t n_slots, CompactWs ch) {
    __shared__ uint4 stage4[(TB_TILE + STAGE_PAD) / 2];
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, base = ch.tile_off[blockIdx.x];
    const uint32_t tot = (uint32_t)(ch.tile_off[blockIdx.x + 1] - base);
    if (tot == 0) return;
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ch, t0, n_slots, slot);
    leave_field(ws.HLP, base, keep, slot, tot, stage4, [&](int, uint64_t i) { return ws.LP[i]; });
    leave_field(ws.hop, base, keep, slot, tot, stage4, [&](int, uint64_t i) { return run_op(in.ops[r0 + i]); });
}

__global__ __launch_bounds__(UT) void jn_lens_kernel(JnIn in, JnWs ws, uint64_t n_heads, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t p = i0; p < n_heads; p += stride)
        if (ws.HLP[p + 1] - ws.HLP[p] >= (1ull << 28)) ok = false;
    for (uint64_t w = i0; w < in.n_walks; w += stride) {
        const uint64_t a = in.seg_off[w], b = in.seg_off[w + 1];
        if (ws.E[b] - ws.E[a] >= (1ull << 32) || ws.M[b] - ws.M[a] >= (1ull << 32)) ok = false;
    }
    if (!ok) atomicOr(bad, 2u);
}

__global__ __launch_bounds__(UT) void jn_walks_kernel(JnIn in, JnWs ws, uint64_t r0, uint64_t n_slots, uint64_t n_tiles, CompactWs ch, s2k_align_out out) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t w = i0; w <= in.n_walks; w += stride) {
        const uint64_t a = in.seg_off[w]; // (seg_off[n_walks] = n_segs: the slots' end)
        const uint64_t oa = kept_before(ch, n_slots, n_tiles, in.ops_off[a] - r0);
        if (out.ops_off) out.ops_off[w] = oa;
        if (w == in.n_walks) continue;
        const uint64_t b = in.seg_off[w + 1];
        const bool isbad = in.bad[w] != 0, live = joined(in, ws, w);
        if (out.flags) out.flags[w] = isbad ? S2K_ALIGN_BAD_PATH : live ? 0u : S2K_ALIGN_OVER;
        if (out.edits) out.edits[w] = isbad ? 0u : (uint32_t)(ws.E[b] - ws.E[a]);
        if (out.matches) out.matches[w] = live ? (uint32_t)(ws.M[b] - ws.M[a]) : 0u;
        if (out.n_ops) out.n_ops[w] = (uint32_t)(kept_before(ch, n_slots, n_tiles, in.ops_off[b] - r0) - oa);
    }
}

__global__ __launch_bounds__(UT) void jn_ops_kernel(JnWs ws, uint64_t n_heads, uint32_t *__restrict__ ops) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t p = i0; p < n_heads; p += stride) ops[p] = run_pack(ws.hop[p], (uint32_t)(ws.HLP[p + 1] - ws.HLP[p]));
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_walks_segments(s2k_ctx *ctx, uint64_t n_reads, const s2k_walk_out *walks, uint64_t n_walks, const s2k_thread_out *paths, uint64_t n_steps,
                              const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs,
                              const uint64_t *d_member_off, const uint64_t *d_out_off, const uint32_t *d_overlap, const uint32_t *d_seq_len, uint64_t n_nodes,
                              const uint64_t *d_q_begin, const uint64_t *d_tgt_off, const uint8_t *d_bad, const s2k_thread_out *src, uint64_t n_src_steps,
                              const uint64_t *d_src_step, const uint32_t *d_src_pos, const s2k_device_out *in, uint32_t seg_len, const s2k_segment_out *out,
                              uint64_t *n_segments, uint64_t *stats) {
    if (n_segments) *n_segments = 0;
    if (stats) memset(stats, 0, S2K_SEGMENT_STATS * sizeof(uint64_t));
    if (!ctx || !n_segments || !stats || !walks || !walks->walk_off || !d_out_off || !d_tgt_off || !src || !src->path_off || !in || !in->km_off)
        return S2K_ERR_INVALID_ARG;
    if (n_walks && (!walks->first_step || !walks->n_steps || !walks->qstart || !walks->qend || !walks->path_start || !walks->path_end || !walks->flags ||
                    !d_q_begin || !d_bad))
        return S2K_ERR_INVALID_ARG;
    if (n_steps && (!paths || !paths->unitig || !paths->pos || !paths->count)) return S2K_ERR_INVALID_ARG;
    if (n_src_steps && (!src->pos || !src->count || !src->item || !in->start)) return S2K_ERR_INVALID_ARG;
    if (n_unitigs && (!d_uni_off || !d_members || !d_circular || !d_member_off || !d_overlap || !d_seq_len)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_walks_segments");
    if (seg_len == 0) seg_len = S2K_SEGMENT_LEN;
    if (seg_len < S2K_SEGMENT_MIN_LEN) return c.invalid("seg_len below S2K_SEGMENT_MIN_LEN");
    if (n_unitigs >= (1ull << 31) || n_nodes >= (1ull << 31) || n_unitigs > n_nodes || n_walks >= (1ull << 31))
        return c.invalid("2^31 unitigs, nodes or walks or more (oriented ids and the scanned words are 32-bit), or more unitigs than nodes");
    if (n_unitigs == 0 && (n_steps || n_nodes)) return c.invalid("steps or nodes without unitigs");
    if (n_steps >= (1ull << 40) || n_src_steps >= (1ull << 40) || n_reads >= (1ull << 40)) return c.invalid("too many steps or reads for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const bool records = out && (out->q_begin || out->q_end || out->t_begin || out->t_end);
    SgIn sg{walks->walk_off, walks->first_step, walks->path_start, walks->n_steps, walks->qstart, walks->qend, walks->flags, n_reads, n_walks,
            paths ? paths->unitig : nullptr, paths ? paths->pos : nullptr, paths ? paths->count : nullptr, n_steps, d_q_begin, d_tgt_off, d_bad,
            src->path_off, d_src_pos ? d_src_pos : src->pos, src->count, src->item, d_src_step, n_src_steps, in->km_off, in->start, seg_len};
    const Lift v{d_uni_off, d_member_off, d_out_off, d_members, d_seq_len, d_overlap, d_circular, n_unitigs, n_nodes};
    // (n_bases is not an argument here: out_off is held to the rules that need no end)
    const TgIn tg{walks->first_step, walks->path_start, walks->path_end, walks->n_steps, walks->flags, sg.unitig, d_out_off, nullptr,
                  d_overlap, n_walks, n_steps, n_unitigs, ~0ull};
    // the part of the workspace whose size the arguments give: the checks, and the number of items
    Layout L;
    const auto words_p = L.bytes<unsigned long long>(SG_WORDS * 8);
    const TgPieces tp = carve_targets(L, n_steps, n_walks, false);
    const auto stepw_p = L.take<uint32_t>(n_src_steps);
    const auto stepj_p = L.take<uint64_t>(n_src_steps), C_p = L.take<uint64_t>(n_src_steps + 1);
    const auto soff_p = L.take<uint64_t>(n_walks + 1);
    uint64_t n_items = 0;
    {
        Layout L0 = L;
        const auto tmp_p = L0.bytes<uint64_t>(scan_tmp_bytes(n_src_steps));
        char *w = L0.alloc(ctx);
        if (!w) return c.nomem();
        uint32_t *bad = (uint32_t *)words_p(w);
        const uint32_t hbad = c.check(
            bad, SG_WORDS * 8, bad,
            [&] {
                launch_tg_check(c, tg, bad);
                c.launch(sg_check_kernel, grid_for(std::max(std::max(n_reads + 1, n_steps), std::max(std::max(n_walks, n_src_steps), n_nodes))), UT, sg, v, bad);
                c.scan(src->count, n_src_steps, C_p(w), tmp_p(w));
            },
            [&] { c.fetch(&n_items, C_p(w) + n_src_steps, 8); });
        if (!c.ok()) return c.device_error();
        if (hbad)
            return c.invalid("a check of s2k_walks_targets or s2k_paths_walks on the walks, the steps or the decomposition; walk_off or src->path_off that does "
                             "not run from 0 to its total without decreasing; walks whose step ranges overlap or descend; qstart above qend; tgt_off that "
                             "decreases or a target of 2^32 bytes or more; or km_off that decreases");
    }
    const uint64_t nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 31)) return c.invalid("too many items for one call");
    const auto KQ_p = L.take<uint64_t>(n_items), KT_p = L.take<uint64_t>(n_items);
    const auto TQ_p = L.take<uint64_t>(nt), TT_p = L.take<uint64_t>(nt);
    const auto aw_p = L.take<uint32_t>(n_items), aq_p = L.take<uint32_t>(n_items), at_p = L.take<uint32_t>(n_items);
    const auto adm_p = carve(L, n_items, nt), hd_p = carve(L, n_items, nt);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(std::max(std::max(n_steps, n_src_steps), nt)));
    char *w = L.alloc(ctx); // the workspace may move: nothing of the first part is kept
    if (!w) return c.nomem();
    unsigned long long *words = words_p(w);
    uint32_t *bad = (uint32_t *)words;
    // the chosen anchors reuse the scanned words, which sg_keep_kernel reads last: 12 B per anchor in 16 B per item
    const SgWs ws{stepw_p(w), stepj_p(w), C_p(w),  tp.G(w), KQ_p(w), KT_p(w), TQ_p(w), TT_p(w), aw_p(w), aq_p(w), at_p(w), (uint32_t *)KQ_p(w),
                  (uint32_t *)KQ_p(w) + n_items, (uint32_t *)KT_p(w), soff_p(w)};
    const CompactWs adm = adm_p(w), hd = hd_p(w);
    c.zero(words, SG_WORDS * 8);
    c.scan(src->count, n_src_steps, ws.C, tmp_p(w));
    launch_tg_steps(c, tg, tp, w, tmp_p(w));
    if (n_src_steps) c.launch(sg_steps_kernel, grid_for(n_src_steps), UT, sg, ws, bad);
    uint32_t hbad = 0;
    c.fetch(&hbad, bad, 4);
    if (!c.sync()) return c.device_error(); // before an item is read through a source step
    if (hbad)
        return c.invalid("items of a source step outside its read, src_step that is neither below n_steps nor S2K_NO_STEP, that lies in a walk of another "
                         "read, or that decreases inside a read");
    uint64_t n_adm = 0, n_chosen = 0;
    unsigned long long h[SG_WORDS] = {0};
    if (n_items) {
        c.launch(sg_items_kernel, (unsigned)nt, TB_THREADS, sg, v, ws, n_items, words);
        c.launch(sg_tiles_kernel, 1, TB_THREADS, ws, nt);
        c.launch(sg_admit_kernel, (unsigned)nt, TB_THREADS, sg, ws, n_items, adm, words);
        c.scan(adm.tile_kept, nt, adm.tile_off, adm_p.scan_tmp(w));
        c.fetch(&n_adm, adm.tile_off + nt, 8);
        c.fetch(h, words, sizeof h);
        if (!c.sync()) return c.device_error();
        if ((uint32_t)h[SW_BAD]) return c.invalid("a candidate whose walk lies before the walk of an earlier candidate");
    }
    const uint64_t nta = (n_adm + TB_TILE - 1) / TB_TILE;
    if (n_adm) {
        c.launch(sg_keep_kernel, (unsigned)nt, TB_THREADS, ws, n_items, adm);
        c.launch(sg_heads_kernel, (unsigned)nta, TB_THREADS, ws, n_adm, seg_len, hd);
        c.scan(hd.tile_kept, nta, hd.tile_off, hd_p.scan_tmp(w));
        c.fetch(&n_chosen, hd.tile_off + nta, 8);
        if (!c.sync()) return c.device_error();
    }
    const uint64_t total = n_walks + n_chosen;
    *n_segments = total;
    if (records && total > out->capacity) return S2K_ERR_CAPACITY;
    if (n_chosen) c.launch(sg_chosen_kernel, (unsigned)nta, TB_THREADS, ws, n_adm, hd);
    c.launch(sg_off_kernel, grid_for(n_walks + 1), UT, ws, n_walks, n_chosen, words);
    if (out && out->seg_off) c.copy(out->seg_off, ws.seg_off, (n_walks + 1) * 8, hipMemcpyDeviceToDevice);
    if (records && total) c.launch(sg_segments_kernel, grid_for(total), UT, sg, ws, total, *out);
    c.fetch(&h[SW_CUT], words + SW_CUT, 8);
    if (!c.sync()) return c.device_error();
    stats[0] = h[SW_CAND], stats[1] = h[SW_OUTSIDE], stats[2] = h[SW_ADM], stats[3] = n_chosen, stats[4] = h[SW_CUT];
    return S2K_OK;
}

s2k_status s2k_align_join(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_seg_off, const uint8_t *d_bad, uint64_t n_segments, const s2k_align_out *seg,
                          const s2k_align_out *out, uint64_t *n_ops_total) {
    if (n_ops_total) *n_ops_total = 0;
    if (!ctx || !n_ops_total || !d_seg_off || !seg || !seg->ops_off) return S2K_ERR_INVALID_ARG;
    if ((n_walks && !d_bad) || (n_segments && (!seg->edits || !seg->flags || !seg->n_ops || !seg->matches)) || (seg->capacity && !seg->ops))
        return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_align_join");
    if (n_walks >= (1ull << 32) || n_segments >= (1ull << 32) || seg->capacity >= (1ull << 40)) return c.invalid("2^32 walks or segments or more, or too many runs");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const JnIn in{d_seg_off, d_bad, n_walks, n_segments, seg->edits, seg->flags, seg->n_ops, seg->matches, seg->ops, seg->ops_off, seg->capacity};
    Layout L;
    const auto words_p = L.bytes<uint32_t>(16);
    const auto ov_p = L.take<uint32_t>(n_segments);
    const auto E_p = L.take<uint64_t>(n_segments + 1), M_p = L.take<uint64_t>(n_segments + 1), OV_p = L.take<uint64_t>(n_segments + 1);
    uint64_t r0 = 0, r1 = 0;
    uint32_t hbad = 0;
    {
        char *w = L.alloc(ctx);
        if (!w) return c.nomem();
        uint32_t *bad = words_p(w);
        hbad = c.check(
            bad, 16, bad, [&] { c.launch(jn_check_kernel, grid_for(std::max(n_walks + 1, n_segments)), UT, in, bad); },
            [&] { fetch_ops_ends(c, seg->ops_off, n_segments, &r0, &r1); });
        if (!c.ok()) return c.device_error();
        if (hbad)
            return c.invalid("seg_off that does not run from 0 to n_segments without decreasing, ops_off that decreases or passes the runs there are, or "
                             "n_ops above a segment's slots");
    }
    const uint64_t n_slots = r1 - r0, nt = (n_slots + TB_TILE - 1) / TB_TILE; // the check pass: r0 <= r1 <= capacity < 2^40
    const auto len_p = L.take<uint32_t>(n_slots);
    const auto LP_p = L.take<uint64_t>(n_slots + 1), HLP_p = L.take<uint64_t>(n_slots + 1);
    const auto hop_p = L.take<uint32_t>(n_slots);
    const auto hd_p = carve(L, n_slots, nt);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(std::max(n_segments, n_slots)));
    char *w = L.alloc(ctx); // the workspace may move: nothing of the first part is kept
    if (!w) return c.nomem();
    uint32_t *bad = words_p(w);
    const JnWs ws{ov_p(w), E_p(w), M_p(w), OV_p(w), len_p(w), LP_p(w), HLP_p(w), hop_p(w)};
    const CompactWs hd = hd_p(w);
    c.zero(bad, 16);
    if (n_segments) c.launch(jn_over_kernel, grid_for(n_segments), UT, in, ws.ov);
    c.scan(seg->edits, n_segments, ws.E, tmp_p(w));
    c.scan(seg->matches, n_segments, ws.M, tmp_p(w));
    c.scan(ws.ov, n_segments, ws.OV, tmp_p(w));
    // (slots: there are segments, and with the check pass walks that hold them)
    if (n_slots) c.launch(jn_slots_kernel, (unsigned)nt, TB_THREADS, in, ws, r0, n_slots, hd, bad);
    c.scan(ws.len, n_slots, ws.LP, tmp_p(w));
    c.scan(hd.tile_kept, nt, hd.tile_off, hd_p.scan_tmp(w));
    uint64_t n_heads = 0;
    c.fetch(&n_heads, hd.tile_off + nt, 8);
    if (!c.sync()) return c.device_error();
    if (n_heads) c.launch(jn_heads_kernel, (unsigned)nt, TB_THREADS, in, ws, r0, n_slots, hd);
    c.copy(ws.HLP + n_heads, ws.LP + n_slots, 8, hipMemcpyDeviceToDevice);
    if (n_heads || n_walks) c.launch(jn_lens_kernel, grid_for(std::max(n_heads, n_walks)), UT, in, ws, n_heads, bad);
    c.fetch(&hbad, bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad & 1u) return c.invalid("a run of length 0 or with an unknown code in a walk that is joined");
    if (hbad) return c.invalid("a joined run of 2^28 bases or more, or a walk whose edits or matches sum to 2^32 or more");
    *n_ops_total = n_heads;
    if (!out) return S2K_OK;
    if (out->ops && n_heads > out->capacity) return S2K_ERR_CAPACITY;
    c.launch(jn_walks_kernel, grid_for(n_walks + 1), UT, in, ws, r0, n_slots, nt, hd, *out);
    if (out->ops && n_heads) c.launch(jn_ops_kernel, grid_for(n_heads), UT, ws, n_heads, out->ops);
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

// s2k_pileup.hip -- the aligned walks of a batch piled up on the unitigs' forward strands, and the per-base call that polishes them
// (include/s2k.h: s2k_walks_pileup, s2k_pileup_consensus).
//
// s2k_walks_pileup, one lane per run slot of the batch's CIGARs (no lane walks a match run):
//  1. tg_check_kernel (s2k_targets_dev.h, with the host side of this prelude and the step cursor) and pl_offsets_kernel: the checks of
//     s2k_walks_targets; ops_off does not decrease, ends inside the n_ops_total runs, n_ops[w] fits walk w's slots (ops_off_ok,
//     s2k_cigar_dev.h, which also has the run word).  One flag word; the host also takes ops_off[0] and ops_off[n_walks].
//  2. tg_steps_kernel, two scans, tg_len_kernel: every walk's target length as s2k_walks_targets has it (0 for a bad walk).
//  3. pl_slots_kernel, one lane per slot: its walk (a search of ops_off), and the target and query bytes its run consumes (0 for a
//     slot behind a walk's runs or of a walk that does not vote); a run of length 0 or with an unknown code raises the flag.  Two
//     scans give every run its offsets in target and query as differences of two entries.
//  4. pl_walks_kernel, one lane per walk: a voting walk's runs consume exactly its target, its query interval lies in the pool; walks
//     used and skipped.  The host reads the flag: up to here only the workspace was written.
//  5. pl_vote_kernel, one lane per run: the step of the run's first target byte by a search of the walk's per-step prefix, then from
//     step to step.  '=' and D pieces add +1 at their first forward position and -1 behind their last one to two difference planes of
//     the workspace (32-bit wrap-around); a gap run reads its forward-left neighbour from the slot before or behind it, finds its
//     shift against d_out and, for D, moves the neighbour's match votes by four more entries of the difference plane; X bytes and I
//     runs go to their planes by one 32-bit atomic add each.  (With S2K_DEBUG_KNOBS and S2K_PILEUP_ROUTE=B in the environment the '='
//     pieces go to `match` by one atomic add per base instead, consecutive lanes on consecutive positions: pl_match_b_kernel.)
//  6. launch_scan_u32 over each difference plane and pl_apply_kernel: match[p] += the running sum, del[p] likewise.
// Every sum is an integer sum: the pile is a function of the multiset of walks.
// s2k_walks_pileup_ex, the same passes and the vote keys of long insertions: pl_slots_kernel also counts the I runs of
// 2 .. 12 bytes of voting walks (n_candidates, known before anything is written); with a key buffer pl_vote_kernel<.., true> leaves
// every run slot a flag and, for a keyed run, its key; launch_scan_u32 over the flags (into QP, which the vote no longer needs) and
// pl_keys_kernel write the keys compact, in run-slot order.  No atomic cursor: the order is a function of the input.
//
// s2k_pileup_consensus: cs_call_kernel (one lane per position: the emitted bytes, 0 to 2 of them, in 16 bits, and their number),
// launch_scan_u32 over the numbers (pos_map), cs_write_kernel (input-ordered: lane p stores its bytes at pos_map[p]; neighbouring lanes
// store neighbouring bytes), cs_units_kernel (new_out_off and new_overlap).
// s2k_pileup_consensus_ex with a table of long-insertion keys: cs_keys_kernel checks the table; cs_call_kernel<true> searches it at a
// position with 2 ins_long > depth and leaves the called candidate's index + 1 per position (0: none) beside the 0 to 1 bytes of the
// base; cs_write_kernel<true> decodes the candidate's 2 to 12 letters from its key, so a position emits 0 to 13 bytes.
//
// Workspace (the context's grow-only count workspace): pile-up 24 B per step, 13 B per walk, 28 B per run slot and 16 B per base,
// with a key buffer 12 B more per run slot; consensus 14 B per base, with a table 18 B.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_cigar_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_targets_dev.h"

namespace s2k {
namespace {

constexpr int PL_WORDS = 8; // the flag word, then the counters of a call
enum { PW_BAD = 0, PW_USED, PW_SKIPPED, PW_OTHER, PW_END_INS, PW_SHIFTED, PW_EMPTY_INS, PW_CAND };
static_assert(PW_CAND < PL_WORDS && S2K_PILEUP_STATS <= PL_WORDS && S2K_CONSENSUS_STATS <= PL_WORDS, "the counters fit the words");

struct PlIn {
    TgIn tg;
    const uint8_t *q;
    uint64_t nq;
    const uint64_t *qb;
    const uint32_t *aflags;
    const uint64_t *ops_off;
    const uint32_t *n_ops, *ops;
    uint64_t n_ops_total;
};

// A/a 0, C/c 1, G/g 2, T/t 3, anything else 4
__device__ __forceinline__ uint32_t code_of(uint32_t c) {
    c &= 0xDFu;
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}
// ACGTacgt -> TGCAtgca, every other byte as it is
__device__ __forceinline__ uint32_t comp_byte(uint32_t c) {
    const uint32_t k = code_of(c);
    return k == 4 ? c : (c & 0x20u) | ((0x41434754u >> (8 * k)) & 0xFFu);
}

// ACGT of a code below 4
__device__ __forceinline__ uint32_t letter_of(uint32_t k) { return (0x54474341u >> (8 * k)) & 0xFFu; }

__global__ __launch_bounds__(UT) void pl_offsets_kernel(PlIn in, uint32_t *__restrict__ bad) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    if (!ops_off_ok(in.ops_off, in.n_ops, in.tg.n_walks, in.n_ops_total, i0, stride)) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void pl_slots_kernel(PlIn in, uint64_t r0, uint64_t n_slots, uint32_t *__restrict__ wk, uint32_t *__restrict__ tl,
                                                      uint32_t *__restrict__ ql, unsigned long long *__restrict__ words) {
    bool ok = true;
    unsigned long long cand = 0; // I runs of S2K_LONG_INS_MIN .. S2K_LONG_INS_MAX bytes of voting walks
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t i = i0; i < n_slots; i += stride) {
        const uint64_t r = r0 + i, w = last_le(in.ops_off, 0, in.tg.n_walks - 1, r);
        uint32_t t = 0, q = 0;
        if (in.aflags[w] == 0 && r - in.ops_off[w] < in.n_ops[w]) {
            const uint32_t v = in.ops[r];
            if (!run_legal(v)) ok = false;
            t = run_target(v);
            q = run_query(v);
            cand += run_op(v) == S2K_CIGAR_I && run_len(v) >= S2K_LONG_INS_MIN && run_len(v) <= S2K_LONG_INS_MAX;
        }
        wk[i] = (uint32_t)w;
        tl[i] = t;
        ql[i] = q;
    }
    if (!ok) atomicOr((uint32_t *)(words + PW_BAD), 1u);
    block_add(cand, words + PW_CAND);
}

__global__ __launch_bounds__(UT) void pl_walks_kernel(PlIn in, uint64_t r0, const uint64_t *__restrict__ TP, const uint64_t *__restrict__ QP,
                                                      const uint32_t *__restrict__ len, unsigned long long *__restrict__ words) {
    bool ok = true;
    unsigned long long n[2] = {0, 0}; // used, skipped
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t w = i0; w < in.tg.n_walks; w += stride) {
        if (in.aflags[w]) {
            n[1]++;
            continue;
        }
        n[0]++;
        const uint64_t a = in.ops_off[w] - r0, b = a + in.n_ops[w], qb = in.qb[w];
        if (TP[b] - TP[a] != len[w] || qb > in.nq || QP[b] - QP[a] > in.nq - qb) ok = false;
    }
    if (!ok) atomicOr((uint32_t *)(words + PW_BAD), 4u);
    block_add(n, words + PW_USED);
}

// The bytes of a walk's stitched path that one step gives (on a circular walk: one round): path coordinates [lo, hi), byte X lies
// at offset X - start of the step's string.  (Walk, walk_of, end_of, owner_step: s2k_targets_dev.h.)
struct Seg {
    uint64_t j, start, lo, hi, L, off;
    uint32_t U;
};

// step j (round j of a circular walk)
__device__ __forceinline__ Seg seg_at(const TgIn &in, const uint64_t *__restrict__ G, const Walk &k, uint64_t j) {
    Seg s;
    s.j = j;
    s.U = in.unitig[k.circ ? k.f : k.f + j];
    s.L = unitig_len(in, s.U);
    s.off = in.out_off[s.U >> 1];
    if (k.circ) {
        s.start = s.lo = j * s.L;
        s.hi = s.lo + s.L;
    } else {
        s.start = G[k.f + j] - k.g0;
        s.lo = j ? end_of(in, G, k, j - 1) : 0;
        s.hi = s.start + s.L;
    }
    return s;
}
// the step that owns byte X of the path (the round, on a circular walk)
__device__ __forceinline__ Seg locate(const TgIn &in, const uint64_t *__restrict__ G, const Walk &k, uint64_t X) {
    return seg_at(in, G, k, k.circ ? X / unitig_len(in, in.unitig[k.f]) : owner_step(in, G, k, X));
}
// the forward position of byte X of the path, which lies in s
__device__ __forceinline__ uint64_t fwd_pos(const Seg &s, uint64_t X) { return (s.U & 1u) ? s.off + s.L - 1 - (X - s.start) : s.off + (X - s.start); }
// the target bytes [*x, x1) cut at the steps: the next piece [*x, xe) and its forward interval [*a, *b); s moves on.  false: none left
__device__ __forceinline__ bool next_piece(const TgIn &in, const uint64_t *__restrict__ G, const Walk &k, Seg &s, uint64_t *x, uint64_t x1, uint64_t *xe,
                                           uint64_t *a, uint64_t *b) {
    for (;;) {
        if (*x >= x1) return false;
        const uint64_t X = k.ps + *x;
        if (X < s.hi) break;
        if (!k.circ && s.j + 1 >= k.n) return false; // (the walk's runs consume its target, which ends inside the path)
        s = seg_at(in, G, k, s.j + 1);
    }
    const uint64_t Xa = k.ps + *x, Xe = std::min(k.ps + x1, s.hi);
    *xe = Xe - k.ps;
    if (s.U & 1u) *a = fwd_pos(s, Xe - 1), *b = fwd_pos(s, Xa) + 1;
    else *a = fwd_pos(s, Xa), *b = fwd_pos(s, Xe - 1) + 1;
    return true;
}

struct Planes {
    s2k_pile pile;
    uint32_t *dm, *dd; // the difference planes of match and del, n_bases + 1 entries
};

__device__ __forceinline__ void interval(uint32_t *__restrict__ d, uint64_t a, uint64_t b) {
    atomicAdd(d + a, 1u);
    atomicAdd(d + b, 0xFFFFFFFFu);
}

// The key of a keyed run (include/s2k.h): n bytes at q + qo, inserted before forward position at after a shift of d; false: a byte
// without a code.  s[i] = c[(i - d) mod n], c the bytes in forward orientation: byte j of c lands at i = (j + d) mod n.
__device__ __forceinline__ bool long_key(const uint8_t *__restrict__ q, uint64_t qo, uint32_t n, bool odd, uint32_t d, uint64_t at, uint64_t *key) {
    uint64_t bits = 0;
    uint32_t i = d % n;
    for (uint32_t j = 0; j < n; j++) { // n <= S2K_LONG_INS_MAX
        uint32_t c = code_of(q[qo + (odd ? n - 1 - j : j)]);
        if (c == 4) return false;
        if (odd) c = 3 - c;
        bits |= (uint64_t)c << (22 - 2 * i);
        i = i + 1 == n ? 0 : i + 1;
    }
    *key = (__brevll(at) >> 28) << 28 | (uint64_t)n << 24 | bits;
    return true;
}

// kf, kk (KEYS): every slot's flag, and the key of a keyed run
template <bool ROUTE_B, bool KEYS>
__global__ __launch_bounds__(UT) void pl_vote_kernel(PlIn in, uint64_t r0, uint64_t n_slots, const uint32_t *__restrict__ wk, const uint32_t *__restrict__ tl,
                                                     const uint32_t *__restrict__ ql, const uint64_t *__restrict__ TP, const uint64_t *__restrict__ QP,
                                                     const uint64_t *__restrict__ G, const uint32_t *__restrict__ len, uint32_t max_shift, Planes pl,
                                                     unsigned long long *__restrict__ words, uint32_t *__restrict__ kf, uint64_t *__restrict__ kk) {
    unsigned long long cnt[4] = {0, 0, 0, 0}; // other, end_ins, shifted, empty_ins
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t i = i0; i < n_slots; i += stride) {
        if (KEYS) kf[i] = 0;
        if (tl[i] == 0 && ql[i] == 0) continue; // no run of a voting walk
        const uint64_t w = wk[i], first = in.ops_off[w] - r0;
        const uint32_t v = in.ops[r0 + i], op = run_op(v), n = run_len(v);
        const Walk k = walk_of(in.tg, G, w);
        const uint64_t T = len[w], x0 = TP[i] - TP[first], qo = in.qb[w] + (QP[i] - QP[first]);
        const bool has_prev = i > first, has_next = i + 1 - first < in.n_ops[w];
        if (op == S2K_CIGAR_I) {
            if (T == 0) {
                cnt[3]++;
                continue;
            }
            const uint64_t xb = x0 ? x0 - 1 : 0;
            const Seg s = locate(in.tg, G, k, k.ps + xb);
            const bool odd = s.U & 1u;
            const uint64_t pb = fwd_pos(s, k.ps + xb);
            const uint64_t g = odd ? (x0 ? pb : pb + 1) : (x0 ? pb + 1 : pb);
            uint64_t e = 0;
            if (odd ? has_next : has_prev) {
                const uint32_t nb = in.ops[r0 + (odd ? i + 1 : i - 1)];
                if (run_op(nb) == S2K_CIGAR_EQ) {
                    const uint64_t room = odd ? std::min(s.hi, k.pe) - k.ps - x0 : x0 - (std::max(s.lo, k.ps) - k.ps);
                    e = std::min<uint64_t>(run_len(nb), room);
                }
            }
            const uint32_t lim = (uint32_t)std::min<uint64_t>(e, max_shift);
            uint32_t d = 0;
            while (d < lim) { // out[g - i] == c[n - 1 - ((i - 1) mod n)], c the inserted bytes in forward orientation, i = d + 1
                const uint32_t m = d % n;
                const uint32_t c = odd ? comp_byte(in.q[qo + m]) : in.q[qo + (n - 1 - m)];
                if (in.tg.out[g - (d + 1)] != c) break;
                d++;
            }
            cnt[2] += d != 0;
            const uint64_t at = g - d;
            if (at == s.off + s.L) {
                cnt[1]++;
                continue;
            }
            uint32_t c = n == 1 ? code_of(in.q[qo]) : 4u;
            if (c < 4 && odd) c = 3 - c;
            atomicAdd((c < 4 ? pl.pile.ins[c] : pl.pile.ins_long) + at, 1u);
            if (KEYS && n >= S2K_LONG_INS_MIN && n <= S2K_LONG_INS_MAX) {
                uint64_t key;
                if (long_key(in.q, qo, n, odd, d, at, &key)) {
                    kf[i] = 1;
                    kk[i] = key;
                }
            }
            continue;
        }
        const uint64_t x1 = x0 + n;
        uint64_t x = x0, xe, a, b;
        Seg s = locate(in.tg, G, k, k.ps + x0);
        if (op == S2K_CIGAR_X) {
            while (next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b)) {
                const bool odd = s.U & 1u;
                for (uint64_t y = x; y < xe; y++) {
                    uint32_t c = code_of(in.q[qo + (y - x0)]);
                    if (c == 4) {
                        cnt[0]++;
                        continue;
                    }
                    if (odd) c = 3 - c;
                    atomicAdd(pl.pile.sub[c] + fwd_pos(s, k.ps + y), 1u);
                }
                x = xe;
            }
            continue;
        }
        if (op == S2K_CIGAR_EQ) {
            if (ROUTE_B) continue; // pl_match_b_kernel
            while (next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b)) {
                interval(pl.dm, a, b);
                x = xe;
            }
            continue;
        }
        // D
        if (!next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b)) continue;
        if (xe < x1) { // more than one piece: no shift
            do {
                interval(pl.dd, a, b);
                x = xe;
            } while (next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b));
            continue;
        }
        const bool odd = s.U & 1u;
        uint64_t e = 0;
        if (odd ? has_next : has_prev) {
            const uint32_t nb = in.ops[r0 + (odd ? i + 1 : i - 1)];
            if (run_op(nb) == S2K_CIGAR_EQ) {
                const uint64_t room = odd ? std::min(s.hi, k.pe) - k.ps - x1 : x0 - (std::max(s.lo, k.ps) - k.ps);
                e = std::min<uint64_t>(run_len(nb), room);
            }
        }
        const uint32_t lim = (uint32_t)std::min<uint64_t>(e, max_shift);
        uint32_t d = 0;
        while (d < lim && in.tg.out[a - (d + 1)] == in.tg.out[b - (d + 1)]) d++;
        interval(pl.dd, a - d, b - d);
        if (d) {
            cnt[2]++;
            if (ROUTE_B) {
                for (uint32_t y = 1; y <= d; y++) {
                    atomicAdd(pl.pile.match + (a - y), 0xFFFFFFFFu);
                    atomicAdd(pl.pile.match + (b - y), 1u);
                }
            } else {
                interval(pl.dm, a, a - d); // -[a - d, a)
                interval(pl.dm, b - d, b); // +[b - d, b)
            }
        }
    }
    block_add(cnt, words + PW_OTHER);
}

// Route B: the '=' pieces by one atomic add per base.  A wave takes 64 run slots; the pieces of its lanes are added one after the
// other, by all 64 lanes on consecutive positions.
__global__ __launch_bounds__(UT) void pl_match_b_kernel(PlIn in, uint64_t r0, uint64_t n_slots, const uint32_t *__restrict__ wk, const uint32_t *__restrict__ tl,
                                                        const uint64_t *__restrict__ TP, const uint64_t *__restrict__ G, Planes pl) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    const int lane = threadIdx.x & 63;
    for (uint64_t base = i0 - lane; base < n_slots; base += stride) {
        const uint64_t i = base + lane;
        bool mine = false;
        Walk k{};
        Seg s{};
        uint64_t x = 0, x1 = 0, xe = 0, a = 0, b = 0;
        if (i < n_slots && tl[i]) {
            const uint32_t v = in.ops[r0 + i];
            if (run_op(v) == S2K_CIGAR_EQ) {
                const uint64_t w = wk[i];
                k = walk_of(in.tg, G, w);
                x = TP[i] - TP[in.ops_off[w] - r0];
                x1 = x + run_len(v);
                s = locate(in.tg, G, k, k.ps + x);
                mine = next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b);
            }
        }
        for (unsigned long long left = __ballot(mine); left; left = __ballot(mine)) {
            for (unsigned long long m = left; m; m &= m - 1) {
                const int src = __builtin_ctzll(m);
                const uint64_t pa = __shfl(a, src, 64), pb = __shfl(b, src, 64);
                for (uint64_t p = pa + lane; p < pb; p += 64) atomicAdd(pl.pile.match + p, 1u);
            }
            if (mine) {
                x = xe;
                mine = next_piece(in.tg, G, k, s, &x, x1, &xe, &a, &b);
            }
        }
    }
}

// plane[p] += the sum of the difference plane up to and including p: pre = the exclusive prefix, n + 1 entries
__global__ __launch_bounds__(UT) void pl_apply_kernel(const uint64_t *__restrict__ pre, uint64_t n, uint32_t *__restrict__ plane) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t p = i0; p < n; p += stride) {
        const uint32_t v = (uint32_t)pre[p + 1];
        if (v) plane[p] += v;
    }
}

// the keys of the flagged slots, compact: pre = the exclusive prefix of the flags
__global__ __launch_bounds__(UT) void pl_keys_kernel(const uint32_t *__restrict__ kf, const uint64_t *__restrict__ kk, const uint64_t *__restrict__ pre,
                                                     uint64_t n_slots, uint64_t *__restrict__ keys) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t i = i0; i < n_slots; i += stride)
        if (kf[i]) keys[pre[i]] = kk[i];
}

// ---- consensus -----------------------------------------------------------------------------------------------------------------------
enum { CW_BAD = 0, CW_LOW, CW_SUB, CW_DEL, CW_INS, CW_LONG, CW_INS_LONG, CW_INS_LONG_BASES };
static_assert(CW_INS_LONG_BASES < PL_WORDS, "the counters fit the words");

// the table of long-insertion keys (s2k_pileup_consensus_ex): ascending keys and their counts
struct LongTable {
    const uint64_t *keys;
    const uint32_t *counts;
    uint64_t n;
};

// keys strictly ascending, every n field in S2K_LONG_INS_MIN .. S2K_LONG_INS_MAX
__global__ __launch_bounds__(UT) void cs_keys_kernel(LongTable t, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t i = i0; i < t.n; i += stride) {
        const uint64_t k = t.keys[i];
        const uint32_t n = (uint32_t)(k >> 24) & 15u;
        if (n < S2K_LONG_INS_MIN || n > S2K_LONG_INS_MAX || (i && t.keys[i - 1] >= k)) ok = false;
    }
    if (!ok) atomicOr(bad, 2u);
}

// the candidate of position p with the largest count, the smallest key among equals: its index + 1 and *cl its count; 0: none
__device__ __forceinline__ uint32_t best_long(const LongTable &t, uint64_t p, uint32_t *cl) {
    const uint64_t want = __brevll(p) >> 28;
    uint64_t lo = 0, hi = t.n;
    while (lo < hi) { // the first key with key >> 28 >= want
        const uint64_t mid = (lo + hi) >> 1;
        if ((t.keys[mid] >> 28) < want) lo = mid + 1;
        else hi = mid;
    }
    uint32_t sel = 0;
    *cl = 0;
    for (uint64_t i = lo; i < t.n && (t.keys[i] >> 28) == want; i++) {
        const uint32_t c = t.counts[i];
        if (c > *cl) *cl = c, sel = (uint32_t)i + 1;
    }
    return sel;
}

__global__ __launch_bounds__(UT) void cs_check_kernel(const uint64_t *__restrict__ out_off, uint64_t n_unitigs, uint64_t n_bases, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t t = i0; t < n_unitigs; t += stride) {
        const uint64_t a = out_off[t], b = out_off[t + 1];
        if (a > b || b > n_bases || b - a >= (1ull << 31)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

// LONG: with a table; sel[p] = the called candidate's index + 1, 0 for none; cnt counts its letters too
template <bool LONG>
__global__ __launch_bounds__(UT) void cs_call_kernel(s2k_pile pile, const uint8_t *__restrict__ out, uint64_t lo, uint64_t hi, uint64_t n_bases, uint32_t min_cov,
                                                     uint32_t *__restrict__ cnt, uint16_t *__restrict__ byt, unsigned long long *__restrict__ words, LongTable tab,
                                                     uint32_t *__restrict__ sel) {
    unsigned long long n[LONG ? 7 : 5] = {}; // low, sub, del, ins, long, ins_long, ins_long_bases
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t p = i0; p < n_bases; p += stride) {
        uint32_t c = 0, bytes = 0, extra = 0, pick = 0;
        if (p >= lo && p < hi) {
            const uint32_t cur_byte = out[p], cur = code_of(cur_byte);
            const uint64_t match = pile.match[p], del = pile.del[p];
            uint64_t tot[5], depth = match + del;
            for (int k = 0; k < 4; k++) {
                tot[k] = pile.sub[k][p];
                depth += tot[k];
            }
            tot[4] = 0;
            tot[cur] += match;
            if (depth < min_cov) {
                n[0]++;
                bytes = cur_byte;
                c = 1;
            } else {
                uint32_t best = 0;
                for (uint32_t k = 1; k < 4; k++)
                    if (pile.ins[k][p] > pile.ins[best][p]) best = k;
                const bool many = 2 * (uint64_t)pile.ins_long[p] > depth;
                if constexpr (LONG) if (many) { // cl <= ins_long[p]: no candidate can be called anywhere else
                    uint32_t cl;
                    const uint32_t s = best_long(tab, p, &cl);
                    if (cl > pile.ins[best][p] && 2 * (uint64_t)cl > depth) {
                        pick = s;
                        extra = (uint32_t)(tab.keys[s - 1] >> 24) & 15u;
                        n[5]++;
                        n[6] += extra;
                    }
                }
                if (!pick && 2 * (uint64_t)pile.ins[best][p] > depth) {
                    bytes = letter_of(best);
                    c = 1;
                    n[3]++;
                }
                if (many && !pick) n[4]++;
                uint32_t top = 0;
                for (uint32_t k = 1; k < 5; k++)
                    if (tot[k] > tot[top]) top = k; // the smallest code among equals; the fifth candidate only for a byte without a code
                if (del > tot[top]) n[2]++;
                else {
                    uint32_t b = cur_byte;
                    if (tot[cur] != tot[top]) { // then top < 4: the fifth candidate is the current byte's
                        b = letter_of(top);
                        n[1]++;
                    }
                    bytes |= b << (8 * c);
                    c++;
                }
            }
        }
        cnt[p] = c + extra;
        byt[p] = (uint16_t)bytes;
        if (LONG) sel[p] = pick;
    }
    block_add(n, words + CW_LOW);
}

// LONG: a position with sel[p] stores the 2 to 12 letters of its candidate first (decoded from the key), then its 0 to 1 bytes
template <bool LONG>
__global__ __launch_bounds__(UT) void cs_write_kernel(const uint32_t *__restrict__ cnt, const uint16_t *__restrict__ byt, const uint64_t *__restrict__ pm, uint64_t n_bases,
                                                      uint8_t *__restrict__ out, LongTable tab, const uint32_t *__restrict__ sel) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t p = i0; p < n_bases; p += stride) {
        uint32_t c = cnt[p];
        const uint32_t b = byt[p];
        uint64_t o = pm[p];
        if (LONG && sel[p]) {
            const uint64_t key = tab.keys[sel[p] - 1];
            const uint32_t n = (uint32_t)(key >> 24) & 15u;
            for (uint32_t i = 0; i < n; i++) out[o + i] = (uint8_t)letter_of((uint32_t)(key >> (22 - 2 * i)) & 3u);
            o += n;
            c -= n;
        }
        if (c > 0) out[o] = (uint8_t)(b & 0xFFu);
        if (c > 1) out[o + 1] = (uint8_t)(b >> 8);
    }
}

__global__ __launch_bounds__(UT) void cs_units_kernel(const uint64_t *__restrict__ out_off, const uint32_t *__restrict__ overlap, uint64_t n_unitigs,
                                                      const uint64_t *__restrict__ pm, uint64_t *__restrict__ new_off, uint32_t *__restrict__ new_overlap) {
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t t = i0; t <= n_unitigs; t += stride) {
        // (no unitig: out_off[0] alone; the positions before it emit nothing)
        if (new_off) new_off[t] = n_unitigs ? pm[out_off[t]] : 0;
        if (t == n_unitigs || !new_overlap) continue;
        const uint64_t a = out_off[t], L = out_off[t + 1] - a;
        const uint64_t e = std::min<uint64_t>(overlap[2 * t], L), o = std::min<uint64_t>(overlap[2 * t + 1], L);
        new_overlap[2 * t] = (uint32_t)(pm[a + L] - pm[a + L - e]);
        new_overlap[2 * t + 1] = (uint32_t)(pm[a + o] - pm[a]);
    }
}

bool pile_complete(const s2k_pile *p) {
    if (!p || !p->match || !p->del || !p->ins_long) return false;
    for (int k = 0; k < 4; k++)
        if (!p->sub[k] || !p->ins[k]) return false;
    return true;
}

bool route_b() {
#ifdef S2K_DEBUG_KNOBS
    const char *e = getenv("S2K_PILEUP_ROUTE");
    return e && (e[0] == 'B' || e[0] == 'b');
#else
    return false;
#endif
}

} // namespace
} // namespace s2k

using namespace s2k;

// both pile-up entries; entry: the one the error texts name
static s2k_status walks_pileup(const char *entry, s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                            const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off,
                            const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const uint8_t *d_query,
                            uint64_t n_query_bytes, const uint64_t *d_q_begin, const uint32_t *d_align_flags, const uint64_t *d_ops_off,
                            const uint32_t *d_n_ops, const uint32_t *d_ops, uint64_t n_ops_total, uint32_t max_shift, const s2k_pile *pile, uint64_t *stats,
                               uint64_t *d_long_keys, uint64_t capacity, uint64_t *n_candidates, uint64_t *n_long_keys) {
    if (stats) memset(stats, 0, S2K_PILEUP_STATS * sizeof(uint64_t));
    if (n_candidates) *n_candidates = 0;
    if (n_long_keys) *n_long_keys = 0;
    if (!ctx || !stats || !d_out_off || !d_ops_off || !n_candidates || !n_long_keys) return S2K_ERR_INVALID_ARG;
    if (n_walks && (!d_first_step || !d_n_steps || !d_path_start || !d_path_end || !d_flags || !d_q_begin || !d_align_flags || !d_n_ops))
        return S2K_ERR_INVALID_ARG;
    if ((n_steps && !d_step_unitig) || (n_unitigs && !d_overlap) || (n_bases && !d_out) || (n_query_bytes && !d_query) || (n_ops_total && !d_ops))
        return S2K_ERR_INVALID_ARG;
    if (n_bases && !pile_complete(pile)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, entry);
    if (max_shift > S2K_PILEUP_MAX_SHIFT) return c.invalid("max_shift above S2K_PILEUP_MAX_SHIFT");
    if (d_long_keys && n_bases >= (1ull << 36)) return c.invalid("vote keys over 2^36 bases or more (a key holds 36 bits of the position)");
    if (n_unitigs >= (1ull << 31) || n_walks >= (1ull << 32) || n_steps >= (1ull << 40) || n_ops_total >= (1ull << 40))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), 2^32 walks or more, or too many steps or runs for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_walks == 0) return S2K_OK;
    const TgIn tg{d_first_step, d_path_start, d_path_end, d_n_steps, d_flags, d_step_unitig, d_out_off, d_out, d_overlap, n_walks, n_steps, n_unitigs, n_bases};
    const PlIn in{tg, d_query, n_query_bytes, d_q_begin, d_align_flags, d_ops_off, d_n_ops, d_ops, n_ops_total};
    // the walks' part of the workspace first: its size does not depend on the runs
    Layout L;
    const auto words_p = L.bytes<unsigned long long>(PL_WORDS * 8);
    const TgPieces tp = carve_targets(L, n_steps, n_walks, true);
    uint64_t r0 = 0, r1 = 0;
    uint32_t hbad = 0;
    {
        char *w = L.alloc(ctx);
        if (!w) return c.nomem();
        uint32_t *bad = (uint32_t *)words_p(w);
        hbad = c.check(
            bad, PL_WORDS * 8, bad,
            [&] {
                launch_tg_check(c, tg, bad);
                c.launch(pl_offsets_kernel, grid_for(n_walks), UT, in, bad);
            },
            [&] { fetch_ops_ends(c, d_ops_off, n_walks, &r0, &r1); });
        if (!c.ok()) return c.device_error();
        if (hbad)
            return c.invalid("a walk whose steps lie outside the paths, a step on a unitig >= n_unitigs, out_off that decreases or passes n_bases, a unitig of "
                             "2^32 bases or more, ops_off that decreases or passes n_ops_total, or n_ops above a walk's slots");
    }
    const uint64_t n_slots = r1 - r0; // the check pass: r0 <= r1 <= n_ops_total < 2^40
    const auto wk_p = L.take<uint32_t>(n_slots), tl_p = L.take<uint32_t>(n_slots), ql_p = L.take<uint32_t>(n_slots);
    const auto TP_p = L.take<uint64_t>(n_slots + 1), QP_p = L.take<uint64_t>(n_slots + 1);
    const auto dm_p = L.take<uint32_t>(n_bases + 1), dd_p = L.take<uint32_t>(n_bases + 1);
    const auto pre_p = L.take<uint64_t>(n_bases + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(std::max(std::max(n_steps, n_walks), std::max(n_slots, n_bases))));
    const auto kf_p = L.take<uint32_t>(d_long_keys ? n_slots : 0); // the keys' pieces last: without a key buffer the layout is the old one
    const auto kk_p = L.take<uint64_t>(d_long_keys ? n_slots : 0);
    char *w = L.alloc(ctx); // the workspace may move: nothing of the first part is kept
    if (!w) return c.nomem();
    unsigned long long *words = words_p(w);
    uint32_t *bad = (uint32_t *)words;
    c.zero(words, PL_WORDS * 8);
    launch_tg_steps(c, tg, tp, w, tmp_p(w));
    launch_tg_lens(c, tg, tp, w, bad);
    if (n_slots) c.launch(pl_slots_kernel, grid_for(n_slots), UT, in, r0, n_slots, wk_p(w), tl_p(w), ql_p(w), words);
    c.scan(tl_p(w), n_slots, TP_p(w), tmp_p(w));
    c.scan(ql_p(w), n_slots, QP_p(w), tmp_p(w));
    c.launch(pl_walks_kernel, grid_for(n_walks), UT, in, r0, TP_p(w), QP_p(w), tp.len(w), words);
    unsigned long long hcand = 0;
    c.fetch(&hbad, bad, 4);
    c.fetch(&hcand, words + PW_CAND, 8);
    if (!c.sync()) return c.device_error();
    if (hbad)
        return c.invalid("a target of 2^32 bytes or more, a run of length 0 or with an unknown code, a voting walk whose runs do not consume exactly its "
                         "target, or a query interval outside the pool");
    *n_candidates = hcand;
    if (d_long_keys && capacity < hcand) return S2K_ERR_CAPACITY;
    // from here on the pile is written
    const bool B = route_b(), K = d_long_keys != nullptr;
    const Planes pl{pile ? *pile : s2k_pile{}, dm_p(w), dd_p(w)}; // (without a base no run consumes a target byte: no plane is touched)
    if (n_slots) {
        c.zero(dm_p(w), (n_bases + 1) * 4);
        c.zero(dd_p(w), (n_bases + 1) * 4);
        c.launch(K ? (B ? pl_vote_kernel<true, true> : pl_vote_kernel<false, true>) : (B ? pl_vote_kernel<true, false> : pl_vote_kernel<false, false>),
                 grid_for(n_slots), UT, in, r0, n_slots, wk_p(w), tl_p(w), ql_p(w), TP_p(w), QP_p(w), tp.G(w), tp.len(w), max_shift, pl, words, kf_p(w), kk_p(w));
        if (B) c.launch(pl_match_b_kernel, grid_for(n_slots), UT, in, r0, n_slots, wk_p(w), tl_p(w), TP_p(w), tp.G(w), pl);
        for (int which = B ? 1 : 0; which < 2; which++) {
            c.scan(which ? dd_p(w) : dm_p(w), n_bases, pre_p(w), tmp_p(w));
            c.launch(pl_apply_kernel, grid_for(n_bases), UT, pre_p(w), n_bases, which ? pile->del : pile->match);
        }
    }
    uint64_t hkeys = 0;
    if (K && n_slots) { // the flags' prefix goes where QP was: the vote is done with it
        c.scan(kf_p(w), n_slots, QP_p(w), tmp_p(w));
        c.launch(pl_keys_kernel, grid_for(n_slots), UT, kf_p(w), kk_p(w), QP_p(w), n_slots, d_long_keys);
        c.fetch(&hkeys, QP_p(w) + n_slots, 8);
    }
    unsigned long long h[PL_WORDS];
    c.fetch(h, words, sizeof h);
    if (!c.sync()) return c.device_error();
    *n_long_keys = hkeys;
    stats[0] = h[PW_USED], stats[1] = h[PW_SKIPPED], stats[2] = h[PW_OTHER], stats[3] = h[PW_END_INS], stats[4] = h[PW_SHIFTED], stats[5] = h[PW_EMPTY_INS];
    return S2K_OK;
}

// both consensus entries; entry: the one the error texts name; tab.n == 0: no table, the kernels and the layout of s2k_pileup_consensus
static s2k_status pileup_consensus(const char *entry, s2k_ctx *ctx, const s2k_pile *pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases,
                                   const uint32_t *d_overlap, uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off, uint8_t *d_new_out, uint64_t capacity,
                                   uint64_t *d_pos_map, uint32_t *d_new_overlap, uint64_t *n_new_bases, uint64_t *stats, const LongTable tab) {
    if (n_new_bases) *n_new_bases = 0;
    if (stats) memset(stats, 0, S2K_CONSENSUS_STATS * sizeof(uint64_t));
    if (!ctx || !n_new_bases || !stats || !d_out_off) return S2K_ERR_INVALID_ARG;
    if ((n_bases && (!d_out || !pile_complete(pile))) || (n_unitigs && !d_overlap) || (tab.n && (!tab.keys || !tab.counts))) return S2K_ERR_INVALID_ARG;
    Call c(ctx, entry);
    if (n_unitigs >= (1ull << 31) || n_bases >= (1ull << 40)) return c.invalid("2^31 unitigs or more, or 2^40 bases or more");
    if (tab.n && (n_bases >= (1ull << 36) || tab.n >= 0xFFFFFFFFull)) return c.invalid("a table of long insertions over 2^36 bases or more, or of 2^32 - 1 keys or more");
    if ((uint64_t)d_new_out & 15u) return c.invalid("d_new_out not 16-byte aligned");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const bool T = tab.n != 0;
    Layout L;
    const auto words_p = L.bytes<unsigned long long>(PL_WORDS * 8);
    const auto cnt_p = L.take<uint32_t>(n_bases);
    const auto byt_p = L.take<uint16_t>(n_bases);
    const auto pm_p = L.take<uint64_t>(n_bases + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_bases));
    const auto sel_p = L.take<uint32_t>(T ? n_bases : 0);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *words = words_p(w);
    uint32_t *bad = (uint32_t *)words;
    uint64_t ends[2] = {0, 0};
    const uint32_t hbad = c.check(words, PL_WORDS * 8, bad, [&] {
        c.launch(cs_check_kernel, grid_for(std::max<uint64_t>(n_unitigs, 1)), UT, d_out_off, n_unitigs, n_bases, bad);
        if (T) c.launch(cs_keys_kernel, grid_for(tab.n), UT, tab, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad & 1u) return c.invalid("out_off that decreases or passes n_bases, or a unitig of 2^31 bases or more");
    if (hbad) return c.invalid("long-insertion keys that do not ascend strictly, or a key whose length is not S2K_LONG_INS_MIN .. S2K_LONG_INS_MAX");
    if (n_unitigs) {
        c.fetch(&ends[0], d_out_off, 8);
        c.fetch(&ends[1], d_out_off + n_unitigs, 8);
        if (!c.sync()) return c.device_error();
    }
    uint64_t total = 0;
    if (n_bases)
        c.launch(T ? cs_call_kernel<true> : cs_call_kernel<false>, grid_for(n_bases), UT, *pile, d_out, ends[0], ends[1], n_bases, min_cov, cnt_p(w), byt_p(w), words, tab,
                 sel_p(w));
    c.scan(cnt_p(w), n_bases, pm_p(w), tmp_p(w));
    unsigned long long h[PL_WORDS];
    c.fetch(&total, pm_p(w) + n_bases, 8);
    c.fetch(h, words, sizeof h);
    if (!c.sync()) return c.device_error();
    *n_new_bases = total;
    if (d_new_out && total > capacity) return S2K_ERR_CAPACITY;
    stats[0] = h[CW_LOW], stats[1] = h[CW_SUB], stats[2] = h[CW_DEL], stats[3] = h[CW_INS], stats[4] = h[CW_LONG];
    stats[5] = h[CW_INS_LONG], stats[6] = h[CW_INS_LONG_BASES];
    if (d_pos_map) c.copy(d_pos_map, pm_p(w), (n_bases + 1) * 8, hipMemcpyDeviceToDevice);
    if (d_new_out_off || (d_new_overlap && n_unitigs)) c.launch(cs_units_kernel, grid_for(n_unitigs + 1), UT, d_out_off, d_overlap, n_unitigs, pm_p(w), d_new_out_off, d_new_overlap);
    if (d_new_out && n_bases)
        c.launch(T ? cs_write_kernel<true> : cs_write_kernel<false>, grid_for(n_bases), UT, cnt_p(w), byt_p(w), pm_p(w), n_bases, d_new_out, tab, sel_p(w));
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

extern "C" {

s2k_status s2k_walks_pileup(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                            const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off,
                            const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const uint8_t *d_query,
                            uint64_t n_query_bytes, const uint64_t *d_q_begin, const uint32_t *d_align_flags, const uint64_t *d_ops_off,
                            const uint32_t *d_n_ops, const uint32_t *d_ops, uint64_t n_ops_total, uint32_t max_shift, const s2k_pile *pile, uint64_t *stats) {
    uint64_t n_cand = 0, n_keys = 0;
    return walks_pileup("s2k_walks_pileup", ctx, n_walks, d_first_step, d_n_steps, d_path_start, d_path_end, d_flags, d_step_unitig, n_steps, d_out_off,
                        d_out, n_bases, d_overlap, n_unitigs, d_query, n_query_bytes, d_q_begin, d_align_flags, d_ops_off, d_n_ops, d_ops, n_ops_total, max_shift, pile,
                        stats, nullptr, 0, &n_cand, &n_keys);
}

s2k_status s2k_walks_pileup_ex(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                            const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off,
                            const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const uint8_t *d_query,
                            uint64_t n_query_bytes, const uint64_t *d_q_begin, const uint32_t *d_align_flags, const uint64_t *d_ops_off,
                            const uint32_t *d_n_ops, const uint32_t *d_ops, uint64_t n_ops_total, uint32_t max_shift, const s2k_pile *pile, uint64_t *stats,
                               uint64_t *d_long_keys, uint64_t capacity, uint64_t *n_candidates, uint64_t *n_long_keys) {
    return walks_pileup("s2k_walks_pileup_ex", ctx, n_walks, d_first_step, d_n_steps, d_path_start, d_path_end, d_flags, d_step_unitig, n_steps, d_out_off,
                        d_out, n_bases, d_overlap, n_unitigs, d_query, n_query_bytes, d_q_begin, d_align_flags, d_ops_off, d_n_ops, d_ops, n_ops_total, max_shift, pile,
                        stats, d_long_keys, capacity, n_candidates, n_long_keys);
}

s2k_status s2k_pileup_consensus(s2k_ctx *ctx, const s2k_pile *pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap,
                                uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off, uint8_t *d_new_out, uint64_t capacity, uint64_t *d_pos_map,
                                uint32_t *d_new_overlap, uint64_t *n_new_bases, uint64_t *stats) {
    return pileup_consensus("s2k_pileup_consensus", ctx, pile, d_out_off, d_out, n_bases, d_overlap, n_unitigs, min_cov, d_new_out_off, d_new_out, capacity, d_pos_map,
                            d_new_overlap, n_new_bases, stats, LongTable{nullptr, nullptr, 0});
}

s2k_status s2k_pileup_consensus_ex(s2k_ctx *ctx, const s2k_pile *pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap,
                                   uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off, uint8_t *d_new_out, uint64_t capacity, uint64_t *d_pos_map,
                                   uint32_t *d_new_overlap, uint64_t *n_new_bases, uint64_t *stats, const uint64_t *d_long_keys, const uint32_t *d_long_counts,
                                   uint64_t n_long_keys) {
    return pileup_consensus("s2k_pileup_consensus_ex", ctx, pile, d_out_off, d_out, n_bases, d_overlap, n_unitigs, min_cov, d_new_out_off, d_new_out, capacity,
                            d_pos_map, d_new_overlap, n_new_bases, stats, LongTable{d_long_keys, d_long_counts, n_long_keys});
}

} // extern "C"

// s2k_align.hip -- read walks aligned to their paths: the bases of every walk's path interval, and the global unit-cost alignment of
// many pairs of byte intervals with edit count and CIGAR runs (include/s2k.h: s2k_walks_targets, s2k_align_pairs).
//
// s2k_walks_targets:
//  1. tg_check_kernel: every step's unitig < 2 n_unitigs; out_off does not decrease, ends inside the n_bases bytes and no unitig has
//     2^32 bases or more; every walk's steps lie inside the paths.  One flag word, read by the host before anything is written.
//  2. tg_steps_kernel, one lane per step g: adv[g] = L - min(overlap, L) as s2k_paths_walks has it, and whether the junction that
//     enters g breaks the rule (overlap of the step before it above either length).
//  3. launch_scan_u32 over both: G and J.  A walk's stitched length and its broken junctions are differences of two entries.
//  4. tg_len_kernel, one lane per walk: bad, and the target's length.
//  5. launch_scan_u32 over the lengths: tgt_off.  The host reads the flag and the total; tgt_off and bad leave by copies.
//  6. tg_copy_kernel, output-ordered as stitch_kernel (s2k_seq.hip): lane g of the grid writes bytes [16 g, 16 g + 16) of the targets
//     with one 16-byte store.  Two lanes find the block's first and last walk by a search of tgt_off, every lane searches that range
//     for its walk, the walk's steps (by G, from the walk's first step) for the step that holds its first byte, and walks on from
//     there.  Bytes come from fetch16; an odd unitig's from the far end, reversed and complemented in registers.
//
// s2k_align_pairs, furthest-reaching points (the rule is in the header).  One wave per pair; lane `lane` of chunk c holds diagonal
// k = 64 c + lane - E of the current wavefront in a register (E = the band: max_edits in the score pass, the pair's distance in the
// trace pass), AL_CH chunks cover 2 * 255 + 1 diagonals.  The neighbour diagonals come by __shfl_up / __shfl_down inside a chunk and
// from the next chunk's edge lane across one.  ext() compares eight bytes at a time (XOR, count of trailing zero bytes), clamped to
// both intervals; the last seven bytes of a pool are loaded bytewise, so no load touches a byte outside a pool.
//  1. al_check_kernel: begin <= end <= the pool's bytes, an interval below 2^31 bytes.  One flag word.
//  2. al_score_kernel: a bounded grid of waves, each takes the next pair off a counter in the workspace (which wave takes which pair
//     reaches no output: every pair's results depend on the pair alone).  Two wavefronts in registers, nothing stored: edits, flags
//     and the pair's run slots 2 edits + 1.
//  3. launch_scan_u32 over the slots: ops_off.  The host reads the total (and the largest distance) and refuses on capacity before
//     anything is written.
//  4. al_trace_kernel: the same grid.  The pair's wavefronts again with the band = its distance, every H[s][k] stored in the wave's
//     (e + 1)^2 words of workspace (row s at s^2); lane 0 walks back, recomputing v from row s - 1, and stages the merged runs from the
//     top of the same words downwards (rows >= s are dead by then); the wave copies them to the pair's slot in order.
//
// Workspace (the context's grow-only count workspace): targets 24 B per step and 13 B per walk; pairs 20 B per pair, then for the
// trace 4 (emax + 1)^2 B per wave in flight, emax the largest distance of a pair that is not over, at most S2K_ALIGN_WAVES waves.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_bytes_dev.h"
#include "s2k_call.h"
#include "s2k_cigar_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_targets_dev.h"

namespace s2k {
namespace {

constexpr int AL_T = 256;                      // threads per block
constexpr int AL_CH = 8;                       // chunks of 64 diagonals
constexpr int32_t AL_NONE = -(1 << 30);        // an H that does not exist
constexpr size_t AL_TRACE_BUDGET = 256u << 20; // bytes of wavefront storage over all waves in flight
static_assert(2 * S2K_ALIGN_MAX_EDITS + 1 <= 64 * AL_CH, "the chunks must cover every diagonal");
static_assert(S2K_ALIGN_WAVES % (AL_T / 64) == 0, "whole blocks");
static_assert(AL_T == TG_T, "the step and length passes are launched with AL_T threads");

// ---- targets (the inputs, the check, step and length passes: s2k_targets_dev.h) -------------------------------------------------------
__global__ __launch_bounds__(AL_T) void tg_copy_kernel(TgIn in, const uint64_t *__restrict__ G, const uint64_t *__restrict__ toff, uint8_t *__restrict__ tgt,
                                                       uint64_t total) {
    __shared__ uint64_t srange[2];
    const uint64_t b0 = (uint64_t)blockIdx.x * (AL_T * 16);
    if (threadIdx.x < 2) srange[threadIdx.x] = last_le(toff, 0, in.n_walks - 1, threadIdx.x ? std::min<uint64_t>(b0 + AL_T * 16, total) - 1 : b0);
    __syncthreads();
    uint64_t pos = b0 + (uint64_t)threadIdx.x * 16;
    if (pos >= total) return;
    const uint32_t want = (uint32_t)std::min<uint64_t>(16, total - pos);
    uint64_t w = last_le(toff, srange[0], srange[1], pos);
    uint64_t lo = 0, hi = 0, wbeg = toff[w], wend = toff[w + 1];
    uint64_t f = 0, n = 0, ps = 0, g0 = 0, j = 0;
    bool circ = false, fresh = true;
    uint32_t filled = 0;
    // the end of step g's string on the stitched path of the walk that starts at step f
    auto end_of = [&](uint64_t g) { return G[g] - g0 + unitig_len(in, in.unitig[g]); };
    while (filled < want) { // pos < total, so a walk with bytes left lies at or after w
        if (wend <= pos) {
            w++;
            wbeg = wend;
            wend = toff[w + 1];
            fresh = true;
            continue;
        }
        if (fresh) { // a walk with bytes is not bad
            f = in.first_step[w], n = in.n_steps[w], ps = in.path_start[w], g0 = G[f];
            circ = in.flags[w] & S2K_WALK_CIRCULAR;
        }
        const uint64_t x = ps + (pos - wbeg); // the byte of the stitched path
        if (fresh) {                          // its step: the last j with j == 0 or the end of step j - 1 <= x
            fresh = false;
            j = 0;
            for (uint64_t b = circ ? 0 : n - 1; j < b;) {
                const uint64_t mid = (j + b + 1) >> 1;
                if (end_of(f + mid - 1) <= x) j = mid;
                else b = mid - 1;
            }
        }
        const uint32_t U = in.unitig[f + j];
        const uint64_t L = unitig_len(in, U), o = in.out_off[U >> 1];
        uint64_t k; // the byte of the step's string
        if (circ) k = x % L;
        else {
            if (j + 1 < n && end_of(f + j) <= x) { // a later step; one that adds no byte is passed over the same way
                j++;
                continue;
            }
            k = x - (G[f + j] - g0);
        }
        const uint32_t c = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(want - filled, wend - pos), L - k);
        uint64_t a, b;
        if (!(U & 1u)) {
            fetch16(in.out + o + k, c, a, b);
            keep_low(c, a, b);
        } else { // bytes k .. k + c - 1 of the reverse complement: the unitig's bytes L - k - c .. L - k - 1, backwards
            fetch16(in.out + o + (L - k - c), c, a, b);
            revcomp_low(c, a, b);
        }
        shl_bytes(filled, a, b);
        lo |= a;
        hi |= b;
        filled += c;
        pos += c;
    }
    uint8_t *p = tgt + (pos - filled);
    if (want == 16) *(ulonglong2 *)p = make_ulonglong2(lo, hi);
    else
        for (uint32_t i = 0; i < want; i++) p[i] = (uint8_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFFu);
}

// ---- pairs ------------------------------------------------------------------------------------------------------------------------
struct Pairs {
    const uint8_t *q, *t;
    uint64_t nq, nt;
    const uint64_t *qb, *qe, *tb, *te;
    uint64_t n;
};

__global__ __launch_bounds__(UT) void al_check_kernel(Pairs p, uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t i = i0; i < p.n; i += stride) {
        const uint64_t a = p.qb[i], b = p.qe[i], c = p.tb[i], d = p.te[i];
        if (a > b || b > p.nq || c > d || d > p.nt || b - a >= (1ull << 31) || d - c >= (1ull << 31)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

// bytes [pos, pos + 8) of a pool of n bytes, little endian, zeros past the pool's end (pos < n): the last seven go bytewise
__device__ __forceinline__ uint64_t load8(const uint8_t *__restrict__ pool, uint64_t n, uint64_t pos) {
    uint64_t v = 0;
    if (pos + 8 <= n) __builtin_memcpy(&v, pool + pos, 8);
    else
        for (uint32_t b = 0; pos + b < n; b++) v |= (uint64_t)pool[pos + b] << (8 * b);
    return v;
}

// one pair on one wave
struct Pair {
    const uint8_t *q, *t;
    uint64_t nq, nt, qb, tb;
    int32_t m, n;
};

// i advanced along diagonal k while the bytes agree (i <= m, 0 <= i + k <= n on entry)
__device__ __forceinline__ int32_t extend(const Pair &p, int32_t i, int32_t k) {
    int32_t left = std::min(p.m - i, p.n - (i + k));
    while (left > 0) {
        const uint64_t x = load8(p.q, p.nq, p.qb + (uint32_t)i) ^ load8(p.t, p.nt, p.tb + (uint32_t)(i + k));
        const int32_t same = std::min<int32_t>(x ? (int32_t)(__builtin_ctzll(x) >> 3) : 8, left);
        i += same;
        left -= same;
        if (x) break;
    }
    return i;
}

__device__ __forceinline__ bool kept(const Pair &p, int32_t i, int32_t k) { return i >= 0 && i <= p.m && i + k >= 0 && i + k <= p.n; }

// v of (s, k) from H[s - 1][k], H[s - 1][k + 1], H[s - 1][k - 1] (AL_NONE: the source does not exist): the largest candidate that is
// kept, AL_NONE without one
__device__ __forceinline__ int32_t best(const Pair &p, int32_t own, int32_t right, int32_t left, int32_t k) {
    int32_t v = AL_NONE;
    if (kept(p, own + 1, k)) v = own + 1;
    if (kept(p, right + 1, k)) v = std::max(v, right + 1);
    if (kept(p, left, k)) v = std::max(v, left);
    return v;
}

// The wavefronts of a pair with band E (diagonal k lies at d = k + E, |n - m| <= smax <= E) up to the first s <= smax with
// H[s][n - m] == m, which is returned; smax + 1 when there is none.  TRACE: H[s][k] goes to ws[s * s + k + s].
template <bool TRACE>
__device__ __forceinline__ int32_t wavefronts(const Pair &p, int32_t E, int32_t smax, int32_t *__restrict__ ws, int lane) {
    int32_t H[AL_CH];
    const int32_t goal = p.n - p.m + E;
#pragma unroll
    for (int c = 0; c < AL_CH; c++) {
        H[c] = AL_NONE;
        if (c == (E >> 6) && lane == (E & 63)) {
            H[c] = extend(p, 0, 0);
            if (TRACE) ws[0] = H[c];
        }
    }
    for (int32_t s = 0;; s++) {
        int32_t g = AL_NONE;
#pragma unroll
        for (int c = 0; c < AL_CH; c++)
            if (c == (goal >> 6)) g = __shfl(H[c], goal & 63, 64);
        if (g == p.m) return s;
        if (s == smax) return smax + 1;
        const int32_t lo = E - (s + 1), hi = E + (s + 1);
        int32_t N[AL_CH];
#pragma unroll
        for (int c = 0; c < AL_CH; c++) {
            N[c] = AL_NONE;
            if (c * 64 + 63 < lo || c * 64 > hi) continue; // the same for the whole wave
            int32_t left = __shfl_up(H[c], 1, 64), right = __shfl_down(H[c], 1, 64);
            const int32_t below = c > 0 ? __shfl(H[c > 0 ? c - 1 : 0], 63, 64) : AL_NONE;
            const int32_t above = c + 1 < AL_CH ? __shfl(H[c + 1 < AL_CH ? c + 1 : c], 0, 64) : AL_NONE;
            if (lane == 0) left = below;
            if (lane == 63) right = above;
            const int32_t d = c * 64 + lane, k = d - E;
            int32_t v = best(p, H[c], right, left, k);
            if (v >= 0) v = extend(p, v, k);
            N[c] = v;
            if (TRACE && d >= lo && d <= hi) ws[(s + 1) * (s + 1) + (d - lo)] = v;
        }
#pragma unroll
        for (int c = 0; c < AL_CH; c++) H[c] = N[c];
    }
}

__device__ __forceinline__ Pair pair_of(const Pairs &ps, uint64_t i) {
    const uint64_t qb = ps.qb[i], tb = ps.tb[i];
    return Pair{ps.q, ps.t, ps.nq, ps.nt, qb, tb, (int32_t)(ps.qe[i] - qb), (int32_t)(ps.te[i] - tb)};
}

// the next pair of the wave: lane 0 draws, all lanes get it
__device__ __forceinline__ uint64_t next_pair(unsigned long long *ctr, int lane) {
    unsigned long long i = 0;
    if (lane == 0) i = atomicAdd(ctr, 1ull);
    return __shfl(i, 0, 64);
}

__global__ __launch_bounds__(AL_T) void al_score_kernel(Pairs ps, uint32_t max_edits, unsigned long long *__restrict__ ctr, uint32_t *__restrict__ emax,
                                                        uint32_t *__restrict__ edits, uint32_t *__restrict__ flags, uint32_t *__restrict__ slots) {
    const int lane = threadIdx.x & 63;
    for (uint64_t i = next_pair(ctr, lane); i < ps.n; i = next_pair(ctr, lane)) {
        const Pair p = pair_of(ps, i);
        const int32_t gap = p.n > p.m ? p.n - p.m : p.m - p.n;
        const int32_t e = gap > (int32_t)max_edits ? (int32_t)max_edits + 1 : wavefronts<false>(p, (int32_t)max_edits, (int32_t)max_edits, nullptr, lane);
        if (lane == 0) {
            const bool over = e > (int32_t)max_edits;
            edits[i] = (uint32_t)e;
            flags[i] = over ? S2K_ALIGN_OVER : 0u;
            slots[i] = over ? 0u : 2u * (uint32_t)e + 1u;
            if (!over) atomicMax(emax, (uint32_t)e); // sizes the trace's workspace; no output
        }
    }
}

// Orders one wave's own stores and loads to its private words of the workspace: lanes of the wave read what other lanes of it wrote.
// Workgroup scope is the narrowest a fence has; the words are never shared beyond the wave, so nothing wider is needed.
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// a run to the staging words, which grow downwards from top
__device__ __forceinline__ void flush_run(int32_t *__restrict__ ws, uint32_t top, uint32_t &n, uint32_t op, uint32_t len) {
    if (len) ws[top - 1 - n++] = (int32_t)run_pack(op, len);
}

__global__ __launch_bounds__(AL_T) void al_trace_kernel(Pairs ps, unsigned long long *__restrict__ ctr, int32_t *__restrict__ wave_ws, uint32_t ws_words,
                                                        const uint32_t *__restrict__ edits, const uint64_t *__restrict__ ops_off, uint32_t *__restrict__ ops, uint32_t *__restrict__ n_ops,
                                                        uint32_t *__restrict__ matches) {
    const int lane = threadIdx.x & 63;
    int32_t *ws = wave_ws + (size_t)(((uint64_t)blockIdx.x * AL_T + threadIdx.x) >> 6) * ws_words;
    for (uint64_t i = next_pair(ctr, lane); i < ps.n; i = next_pair(ctr, lane)) {
        const uint64_t o = ops_off[i];
        if (ops_off[i + 1] == o) { // no slot: the pair is over (every other pair has 2 edits + 1 >= 1)
            if (lane == 0) {
                if (n_ops) n_ops[i] = 0;
                if (matches) matches[i] = 0;
            }
            continue;
        }
        const Pair p = pair_of(ps, i);
        const int32_t e = (int32_t)edits[i]; // (e + 1)^2 <= ws_words: the score pass took the largest
        wavefronts<true>(p, e, e, ws, lane);
        wave_fence(); // lane 0 reads what the other lanes stored
        const uint32_t top = (uint32_t)(e + 1) * (uint32_t)(e + 1);
        uint32_t n = 0, eq = 0;
        if (lane == 0) {
            uint32_t op = S2K_CIGAR_EQ, len = 0; // the run being built, last run first
            int32_t s = e, k = p.n - p.m, at = p.m;
            for (;;) {
                int32_t own = AL_NONE, right = AL_NONE, left = AL_NONE, v = 0;
                if (s > 0) {
                    const int32_t *row = ws + (s - 1) * (s - 1) + (s - 1); // row[k] = H[s - 1][k], |k| <= s - 1
                    if (k > -s && k < s) own = row[k];
                    if (k + 1 > -s && k + 1 < s) right = row[k + 1];
                    if (k - 1 > -s && k - 1 < s) left = row[k - 1];
                    v = best(p, own, right, left, k);
                }
                const uint32_t same = (uint32_t)(at - v);
                if (same) {
                    if (op != S2K_CIGAR_EQ) flush_run(ws, top, n, op, len), op = S2K_CIGAR_EQ, len = 0;
                    len += same;
                    eq += same;
                }
                at = v;
                if (s == 0) break;
                uint32_t step;
                if (own + 1 == v) step = S2K_CIGAR_X, at -= 1;
                else if (right + 1 == v) step = S2K_CIGAR_I, at -= 1, k += 1;
                else step = S2K_CIGAR_D, k -= 1;
                if (op != step) flush_run(ws, top, n, op, len), op = step, len = 0;
                len += 1;
                s -= 1;
            }
            flush_run(ws, top, n, op, len);
            if (n_ops) n_ops[i] = n;
            if (matches) matches[i] = eq;
        }
        wave_fence(); // the wave reads what lane 0 staged
        n = __shfl(n, 0, 64);
        if (ops)
            for (uint32_t r = lane; r < n; r += 64) ops[o + r] = (uint32_t)ws[top - n + r];
        wave_fence(); // the next pair's wavefronts overwrite these words
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_walks_targets(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                             const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps,
                             const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs,
                             uint64_t *d_tgt_off, uint8_t *d_tgt, uint8_t *d_bad, uint64_t capacity, uint64_t *n_bytes) {
    if (n_bytes) *n_bytes = 0;
    if (!ctx || !n_bytes || !d_out_off) return S2K_ERR_INVALID_ARG;
    if (n_walks && (!d_first_step || !d_n_steps || !d_path_start || !d_path_end || !d_flags)) return S2K_ERR_INVALID_ARG;
    if ((n_steps && !d_step_unitig) || (n_unitigs && !d_overlap) || (n_bases && !d_out)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_walks_targets");
    if (n_unitigs >= (1ull << 31) || n_walks >= (1ull << 40) || n_steps >= (1ull << 40))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or too many walks or steps for one call");
    if (((uint64_t)d_tgt & 15u) || ((uint64_t)d_out & 7u)) return c.invalid("d_tgt not 16-byte aligned or d_out not 8-byte aligned");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const TgPieces tp = carve_targets(L, n_steps, n_walks, true);
    const auto off_p = L.take<uint64_t>(n_walks + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(std::max(n_steps, n_walks)));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint32_t *bad = flag(w);
    const TgIn in{d_first_step, d_path_start, d_path_end, d_n_steps, d_flags, d_step_unitig, d_out_off, d_out, d_overlap, n_walks, n_steps, n_unitigs, n_bases};
    uint32_t hbad = c.check(bad, 16, bad, [&] { launch_tg_check(c, in, bad); });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("a walk whose steps lie outside the paths, a step on a unitig >= n_unitigs, out_off that decreases or passes n_bases, or a unitig "
                         "of 2^32 bases or more");
    if (n_walks == 0) {
        if (d_tgt_off) {
            c.zero(d_tgt_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    launch_tg_steps(c, in, tp, w, tmp_p(w));
    launch_tg_lens(c, in, tp, w, bad);
    c.scan(tp.len(w), n_walks, off_p(w), tmp_p(w));
    uint64_t total = 0;
    c.fetch(&total, off_p(w) + n_walks, 8);
    c.fetch(&hbad, bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad) return c.invalid("a target of 2^32 bytes or more");
    *n_bytes = total;
    if (d_tgt && total > capacity) return S2K_ERR_CAPACITY;
    const uint64_t nb = (total + AL_T * 16 - 1) / (AL_T * 16);
    if (d_tgt && nb >= (1ull << 31)) return c.invalid("2^43 bytes or more");
    if (d_tgt_off) c.copy(d_tgt_off, off_p(w), (n_walks + 1) * 8, hipMemcpyDeviceToDevice);
    if (d_bad) c.copy(d_bad, tp.bad8(w), n_walks, hipMemcpyDeviceToDevice);
    if (d_tgt && total) c.launch(tg_copy_kernel, (unsigned)nb, AL_T, in, tp.G(w), off_p(w), d_tgt, total);
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_align_pairs(s2k_ctx *ctx, const uint8_t *d_query, uint64_t n_query_bytes, const uint8_t *d_target, uint64_t n_target_bytes,
                           const uint64_t *d_q_begin, const uint64_t *d_q_end, const uint64_t *d_t_begin, const uint64_t *d_t_end, uint64_t n_pairs,
                           uint32_t max_edits, const s2k_align_out *out, uint64_t *n_ops_bound) {
    if (n_ops_bound) *n_ops_bound = 0;
    if (!ctx || !n_ops_bound) return S2K_ERR_INVALID_ARG;
    if (n_pairs && (!d_q_begin || !d_q_end || !d_t_begin || !d_t_end)) return S2K_ERR_INVALID_ARG;
    if ((n_query_bytes && !d_query) || (n_target_bytes && !d_target)) return S2K_ERR_INVALID_ARG;
    const bool writing = out && (out->ops || out->n_ops || out->matches);
    if (writing && n_pairs && (!out->edits || !out->flags || !out->ops_off)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_align_pairs");
    if (max_edits > S2K_ALIGN_MAX_EDITS) return c.invalid("max_edits above S2K_ALIGN_MAX_EDITS");
    if (n_pairs >= (1ull << 32)) return c.invalid("2^32 pairs or more");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_pairs == 0) {
        if (out && out->ops_off) {
            c.zero(out->ops_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    const unsigned blocks = (unsigned)(std::min<uint64_t>(n_pairs, S2K_ALIGN_WAVES) + AL_T / 64 - 1) / (AL_T / 64);
    uint64_t total = 0;
    uint32_t emax = 0;
    const Pairs ps{d_query, d_target, n_query_bytes, n_target_bytes, d_q_begin, d_q_end, d_t_begin, d_t_end, n_pairs};
    {
        Layout L;
        const auto words = L.bytes<unsigned long long>(64); // the pair counter; then the check's flag and the largest distance
        const auto edits_p = L.take<uint32_t>(n_pairs), flags_p = L.take<uint32_t>(n_pairs), slots_p = L.take<uint32_t>(n_pairs);
        const auto off_p = L.take<uint64_t>(n_pairs + 1);
        const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_pairs));
        char *w = L.alloc(ctx);
        if (!w) return c.nomem();
        unsigned long long *ctr = words(w);
        uint32_t *bad = (uint32_t *)(ctr + 1), *dmax = bad + 1;
        const uint32_t hbad = c.check(ctr, 64, bad, [&] { c.launch(al_check_kernel, grid_for(n_pairs), UT, ps, bad); });
        if (!c.ok()) return c.device_error();
        if (hbad) return c.invalid("a begin above its end, an interval outside its pool, or an interval of 2^31 bytes or more");
        c.launch(al_score_kernel, blocks, AL_T, ps, max_edits, ctr, dmax, edits_p(w), flags_p(w), slots_p(w));
        c.scan(slots_p(w), n_pairs, off_p(w), tmp_p(w));
        c.fetch(&total, off_p(w) + n_pairs, 8);
        c.fetch(&emax, dmax, 4);
        if (!c.sync()) return c.device_error();
        *n_ops_bound = total;
        if (!out) return S2K_OK;
        if (writing && total > out->capacity) return S2K_ERR_CAPACITY;
        if (out->edits) c.copy(out->edits, edits_p(w), n_pairs * 4, hipMemcpyDeviceToDevice);
        if (out->flags) c.copy(out->flags, flags_p(w), n_pairs * 4, hipMemcpyDeviceToDevice);
        if (out->ops_off) c.copy(out->ops_off, off_p(w), (n_pairs + 1) * 8, hipMemcpyDeviceToDevice);
        if (!c.sync()) return c.device_error(); // the workspace may move below
    }
    if (!writing) return S2K_OK;
    // the trace reads edits and ops_off from the outputs: they are final, and the workspace now holds the wavefronts
    const uint32_t ws_words = (emax + 1) * (emax + 1);
    const uint64_t fit = std::max<uint64_t>(AL_TRACE_BUDGET / ((size_t)ws_words * 4), AL_T / 64);
    const unsigned tblocks = (unsigned)std::min<uint64_t>(blocks, fit / (AL_T / 64));
    Layout L;
    const auto words = L.bytes<unsigned long long>(64);
    const auto h_p = L.take<int32_t>((uint64_t)tblocks * (AL_T / 64) * ws_words);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    c.zero(words(w), 64);
    c.launch(al_trace_kernel, tblocks, AL_T, ps, words(w), h_p(w), ws_words, out->edits, out->ops_off, out->ops, out->n_ops, out->matches);
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

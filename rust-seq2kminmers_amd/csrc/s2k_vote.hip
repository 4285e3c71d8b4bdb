// s2k_vote.hip -- majority-vote representatives of the graph's nodes (include/s2k.h: s2k_table_vote_keys,
// s2k_table_vote_representatives, s2k_vote_ordinals).
//
// The fingerprint F(s) = sum (s_j + 1) M^(n-1-j) mod 2^64 satisfies F(a || b) = F(a) M^|b| + F(b), so the fingerprint of any stretch of
// the batch's bases is a difference of two prefix values, and the fingerprint of its reverse complement a difference of two suffix
// values of the complemented bases.  The stream is the batch's bases from the 16-byte boundary at or below its first byte, in chunks
// of 16 bytes; bytes of a chunk outside the batch count as 0.  P(p) = F(stream[0, p)), R(p) = sum over j >= p of (comp(u_j) + 1)
// M^(j-p); F(stream[a, b)) = P(b) - P(a) M^(b-a) and F(revcomp(stream[a, b))) = R(a) - M^(b-a) R(b).
//
// Both calls, per batch:
//  1. vote_reads_kernel: the count relation n + k - 1 of every read, km_off / mn_off / read_off non-decreasing (one flag word, read by
//     the host before a triple is indexed through the relation).
//  2. vote_count_kernel: tiles of TB_TILE items, the look-up fused in; every item whose hash is in the table has its four positions
//     checked against its read (flag word); per item its node (4 B), per 64 items the mask of such items, per tile their number.
//  3. launch_scan_u32 over the tiles; the host reads the flag and the total.
//  4. the fingerprints of the stream, three kernels, a lane takes 4 chunks (64 B), a workgroup 16 KiB: fp_block_kernel (each
//     workgroup's two aggregates: every byte is read once, both orientations from the same registers), fp_scan_kernel (one workgroup
//     scans the aggregates, a lane a run of them) and fp_write_kernel (the chunks again, now with the workgroup's prefix and suffix:
//     PF[c] = P(16 c), PR[c] = R(16 c), 8 B each per chunk).  The scans compose affine maps x -> x m + v, so no lane needs a power of
//     M that depends on its position.
//  5. per item (item_keys): P and R at its four positions -- a chunk value and at most 15 bytes of Horner steps each -- and three
//     powers M^len from the table of the 32 squarings M^(2^i).  No lane walks a node's bytes.
// s2k_table_vote_keys stages a tile's keys in LDS at three times the item's slot and lets them go as one run (leave_run).
// s2k_table_vote_representatives looks the three keys up in the vote table (lookup_many), keeps w << 52 | e << 40 per item (8 B),
// flags a missing key, and only after the host has seen the flag does one 64-bit atomicMax per item into d_best.
//
// Workspace (the context's grow-only count workspace): 4.2 B per item (12.2 B for the representatives) and 1 B per base.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

constexpr uint64_t VT_M = 0x9E3779B97F4A7C15ull;
constexpr uint32_t VT_NONE = 0xFFFFFFFFu;
constexpr uint64_t VT_ORD = (1ull << 40) - 1; // the ordinal's field of a d_best word
constexpr int VT_T = 256;                      // lanes of a fingerprint workgroup
constexpr int VT_CPL = 4;                      // chunks per lane
constexpr uint64_t VT_BLOCK = (uint64_t)VT_T * VT_CPL; // chunks per workgroup
constexpr uint64_t B01 = 0x0101010101010101ull;

constexpr uint64_t mpow(uint64_t e) { // M^e mod 2^64
    uint64_t r = 1, b = VT_M;
    for (; e; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}
#define VT_SQ4(i) mpow(1ull << (i)), mpow(1ull << ((i) + 1)), mpow(1ull << ((i) + 2)), mpow(1ull << ((i) + 3))
__constant__ uint64_t VT_SQ[32] = {VT_SQ4(0), VT_SQ4(4), VT_SQ4(8), VT_SQ4(12), VT_SQ4(16), VT_SQ4(20), VT_SQ4(24), VT_SQ4(28)};
#undef VT_SQ4
// M^e: one multiplication per set bit of e
__device__ __forceinline__ uint64_t mpow_dev(uint32_t e) {
    uint64_t r = 1;
    for (int i = 0; e; i++, e >>= 1)
        if (e & 1u) r *= VT_SQ[i];
    return r;
}
// the splitmix64 finaliser
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 0x80 in every byte of y that is zero, 0 elsewhere (exact: no carry leaves a byte)
__device__ __forceinline__ uint64_t zero_bytes(uint64_t y) { return ~(((y & (0x7F * B01)) + 0x7F * B01) | y | (0x7F * B01)); }
// ACGTacgt -> TGCAtgca in every byte, every other byte as it is (s2k_seq.hip: comp8)
__device__ __forceinline__ uint64_t comp_word(uint64_t x) {
    const uint64_t f = x & (0xDF * B01);
    const uint64_t at = zero_bytes(f ^ (0x41 * B01)) | zero_bytes(f ^ (0x54 * B01));
    const uint64_t cg = zero_bytes((f ^ (0x43 * B01)) & (0xFB * B01));
    return x ^ ((at >> 7) * 0x15) ^ ((cg >> 7) * 0x04);
}

// ---- the stream --------------------------------------------------------------------------------------------------------------------
struct Stream {
    const uint64_t *w; // the 16-byte boundary at or below the batch's first base
    uint64_t lead;     // the stream position of that base (0 .. 15)
    uint64_t end;      // one past the batch's last base
    uint64_t n_chunks; // ceil(end / 16)
};
// the 8 bytes at stream position 8 wi, those outside [lead, end) as 0; a word that holds none of the batch's bytes is not loaded
__device__ __forceinline__ uint64_t stream_word(const Stream &s, uint64_t wi) {
    const uint64_t p = wi * 8;
    if (p + 8 <= s.lead || p >= s.end) return 0;
    uint64_t v = s.w[wi];
    if (p < s.lead) v &= ~0ull << ((s.lead - p) * 8);
    if (p + 8 > s.end) v &= ~0ull >> ((p + 8 - s.end) * 8);
    return v;
}
__device__ __forceinline__ uint32_t byte_of(uint64_t w0, uint64_t w1, uint32_t j) { // byte j (0 .. 15) of a chunk
    return (uint32_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * (j - 8))) & 0xFFu);
}

#define VT_PW8(i) mpow(i), mpow((i) + 1), mpow((i) + 2), mpow((i) + 3), mpow((i) + 4), mpow((i) + 5), mpow((i) + 6), mpow((i) + 7)
// a chunk's bytes u_0 .. u_15: f = sum (u_j + 1) M^(15-j), g = sum (comp(u_j) + 1) M^j; a byte times a constant, no chain
__device__ __forceinline__ void chunk_fg(uint64_t w0, uint64_t w1, uint64_t &f, uint64_t &g) {
    constexpr uint64_t PW[16] = {VT_PW8(0), VT_PW8(8)};
    const uint64_t c0 = comp_word(w0), c1 = comp_word(w1);
    uint64_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        a += (uint64_t)(byte_of(w0, w1, j) + 1u) * PW[15 - j];
        b += (uint64_t)(byte_of(c0, c1, j) + 1u) * PW[j];
    }
    f = a;
    g = b;
}
#undef VT_PW8

// ---- scans of affine maps x -> x m + v ------------------------------------------------------------------------------------------
struct Aff {
    uint64_t m, v;
};
__device__ __forceinline__ Aff then(Aff a, Aff b) { return Aff{a.m * b.m, a.v * b.m + b.v}; } // first a, then b
template <bool UP>
__device__ __forceinline__ Aff shfl1(Aff x, int o) {
    Aff y;
    y.m = UP ? __shfl_up((unsigned long long)x.m, o) : __shfl_down((unsigned long long)x.m, o);
    y.v = UP ? __shfl_up((unsigned long long)x.v, o) : __shfl_down((unsigned long long)x.v, o);
    return y;
}
// UP: the maps of the lanes below this one in the workgroup, composed in ascending order; otherwise those of the lanes above it, in
// descending order.  *total: all of them in that order.  lds: one Aff per wave.  Ends with a barrier: lds may be used again.
template <bool UP>
__device__ inline Aff block_scan_excl(Aff x, Aff *lds, Aff *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Aff y = shfl1<UP>(x, o); // the o .. 2 o lanes applied before this one's
        if (UP ? lane >= o : lane + o < 64) x = then(y, x);
    }
    if (lane == (UP ? 63 : 0)) lds[w] = x;
    Aff ex = shfl1<UP>(x, 1);
    if (lane == (UP ? 0 : 63)) ex = Aff{1, 0};
    __syncthreads();
    Aff pre{1, 0}, tot{1, 0};
#pragma unroll
    for (int i = 0; i < VT_T / 64; i++) {
        const int j = UP ? i : VT_T / 64 - 1 - i;
        const Aff v = lds[j];
        if (UP ? j < w : j > w) pre = then(pre, v);
        tot = then(tot, v);
    }
    __syncthreads();
    *total = tot;
    return then(pre, ex);
}

// ---- the fingerprints of the stream ---------------------------------------------------------------------------------------------------
constexpr uint64_t VT_M16 = mpow(16), VT_MLANE = mpow(16 * VT_CPL), VT_MBLOCK = mpow(16 * VT_BLOCK);

// the lane's chunks c0 .. c0 + VT_CPL - 1: their values, and the lane's two maps
__device__ __forceinline__ void lane_values(const Stream &s, uint64_t c0, uint64_t (&f)[VT_CPL], uint64_t (&g)[VT_CPL], Aff *fwd, Aff *rev) {
#pragma unroll
    for (int q = 0; q < VT_CPL; q++) chunk_fg(stream_word(s, 2 * (c0 + q)), stream_word(s, 2 * (c0 + q) + 1), f[q], g[q]);
    uint64_t a = 0, b = 0;
#pragma unroll
    for (int q = 0; q < VT_CPL; q++) {
        a = a * VT_M16 + f[q];
        b = b * VT_M16 + g[VT_CPL - 1 - q];
    }
    *fwd = Aff{VT_MLANE, a};
    *rev = Aff{VT_MLANE, b};
}

__global__ __launch_bounds__(VT_T) void fp_block_kernel(Stream s, uint64_t *__restrict__ fb, uint64_t *__restrict__ gb) {
    __shared__ Aff lds[VT_T / 64];
    uint64_t f[VT_CPL], g[VT_CPL];
    Aff fwd, rev, tot;
    lane_values(s, ((uint64_t)blockIdx.x * VT_T + threadIdx.x) * VT_CPL, f, g, &fwd, &rev);
    block_scan_excl<true>(fwd, lds, &tot);
    if (threadIdx.x == 0) fb[blockIdx.x] = tot.v;
    block_scan_excl<false>(rev, lds, &tot);
    if (threadIdx.x == 0) gb[blockIdx.x] = tot.v;
}

// one workgroup; lane t takes the workgroups [t run, (t + 1) run): pfb[b] = P at the start of workgroup b's bytes, prb[b] = R at their end
__global__ __launch_bounds__(VT_T) void fp_scan_kernel(const uint64_t *__restrict__ fb, const uint64_t *__restrict__ gb, uint64_t nb, uint64_t run,
                                                       uint64_t *__restrict__ pfb, uint64_t *__restrict__ prb) {
    __shared__ Aff lds[VT_T / 64];
    const uint64_t lo = std::min<uint64_t>((uint64_t)threadIdx.x * run, nb), hi = std::min<uint64_t>(lo + run, nb);
    Aff a{1, 0}, tot;
    for (uint64_t b = lo; b < hi; b++) a = then(a, Aff{VT_MBLOCK, fb[b]});
    uint64_t cur = block_scan_excl<true>(a, lds, &tot).v; // the map applied to P(0) == 0
    for (uint64_t b = lo; b < hi; b++) {
        pfb[b] = cur;
        cur = cur * VT_MBLOCK + fb[b];
    }
    a = Aff{1, 0};
    for (uint64_t b = hi; b-- > lo;) a = then(a, Aff{VT_MBLOCK, gb[b]});
    cur = block_scan_excl<false>(a, lds, &tot).v; // applied to R(end of the padded stream) == 0
    for (uint64_t b = hi; b-- > lo;) {
        prb[b] = cur;
        cur = cur * VT_MBLOCK + gb[b];
    }
}

__global__ __launch_bounds__(VT_T) void fp_write_kernel(Stream s, const uint64_t *__restrict__ pfb, const uint64_t *__restrict__ prb,
                                                        uint64_t *__restrict__ pf, uint64_t *__restrict__ pr) {
    __shared__ Aff lds[VT_T / 64];
    uint64_t f[VT_CPL], g[VT_CPL];
    Aff fwd, rev, tot;
    const uint64_t c0 = ((uint64_t)blockIdx.x * VT_T + threadIdx.x) * VT_CPL;
    lane_values(s, c0, f, g, &fwd, &rev);
    const Aff ef = block_scan_excl<true>(fwd, lds, &tot), er = block_scan_excl<false>(rev, lds, &tot);
    uint64_t p = pfb[blockIdx.x] * ef.m + ef.v, r = prb[blockIdx.x] * er.m + er.v; // P at the lane's first byte, R past its last
#pragma unroll
    for (int q = 0; q < VT_CPL; q++) {
        if (c0 + q <= s.n_chunks) pf[c0 + q] = p;
        p = p * VT_M16 + f[q];
    }
#pragma unroll
    for (int q = VT_CPL - 1; q >= 0; q--) {
        r = r * VT_M16 + g[q];
        if (c0 + q <= s.n_chunks) pr[c0 + q] = r;
    }
}

struct Fp {
    Stream s;
    const uint64_t *pf, *pr; // n_chunks + 1 entries each
    uint64_t shift;          // stream position of byte x of d_bases = x + shift (mod 2^64)
};
// P(p) and R(p), p <= s.end: the chunk's value and the bytes between p and the chunk's boundary
__device__ inline uint64_t prefix_at(const Fp &fp, uint64_t p) {
    const uint64_t c = p >> 4;
    const uint32_t r = (uint32_t)(p & 15u);
    uint64_t acc = fp.pf[c];
    if (r) {
        const uint64_t w0 = stream_word(fp.s, 2 * c), w1 = r > 8 ? stream_word(fp.s, 2 * c + 1) : 0ull;
        for (uint32_t j = 0; j < r; j++) acc = acc * VT_M + byte_of(w0, w1, j) + 1u;
    }
    return acc;
}
__device__ inline uint64_t suffix_at(const Fp &fp, uint64_t p) {
    const uint64_t c = p >> 4;
    const uint32_t r = (uint32_t)(p & 15u);
    if (!r) return fp.pr[c];
    uint64_t acc = fp.pr[c + 1]; // r > 0: p lies inside chunk c < n_chunks
    const uint64_t w1 = comp_word(stream_word(fp.s, 2 * c + 1)), w0 = r < 8 ? comp_word(stream_word(fp.s, 2 * c)) : 0ull;
    for (uint32_t j = 16; j-- > r;) acc = acc * VT_M + byte_of(w0, w1, j) + 1u;
    return acc;
}

// ---- the items -------------------------------------------------------------------------------------------------------------------
struct VoteIn { // s2k_seq.hip: SeqIn
    const uint64_t *km_off, *hash, *mn_off;
    const uint32_t *mn_j, *mn_jend;
    const uint8_t *rev;
    const uint64_t *read_off;
    uint64_t n_reads, n_items;
    uint32_t k;
};

__global__ __launch_bounds__(VT_T) void vote_reads_kernel(VoteIn in, uint32_t *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * VT_T + threadIdx.x;
    if (r >= in.n_reads) return;
    const uint64_t a = in.km_off[r], b = in.km_off[r + 1], c = in.mn_off[r], d = in.mn_off[r + 1];
    bool ok = a <= b && c <= d && in.read_off[r] <= in.read_off[r + 1];
    if (r == 0) ok = ok && a == 0 && c == 0;
    if (ok && b > a) ok = d - c == (b - a) + in.k - 1;
    if (!ok) atomicOr(bad, 1u);
}

// what item x of read rd is made of (s2k_seq.hip: span_of, the same rules); false when a position breaks them
struct Span {
    uint32_t a, len, shift_fwd, shift_rev;
};
__device__ inline bool span_of(const VoteIn &in, uint64_t rd, uint64_t x, Span *s) {
    const uint64_t tj = in.mn_off[rd] + (x - in.km_off[rd]);
    const uint32_t a = in.mn_j[tj], a2 = in.mn_j[tj + 1], b2 = in.mn_jend[tj + in.k - 2], b = in.mn_jend[tj + in.k - 1];
    const uint64_t rl = in.read_off[rd + 1] - in.read_off[rd];
    if (!(a <= a2 && a2 <= b && a <= b2 && b2 <= b && (uint64_t)b < rl && b - a < 0xFFFFFFFFu)) return false;
    s->a = a;
    s->len = b - a + 1;
    s->shift_fwd = a2 - a;
    s->shift_rev = b - b2;
    return true;
}

__global__ __launch_bounds__(TB_THREADS) void vote_count_kernel(TableView tv, VoteIn in, uint32_t *__restrict__ node, CompactWs ws,
                                                                uint32_t *__restrict__ bad) {
    __shared__ uint32_t wc[TB_WORDS];
    __shared__ uint64_t sread[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, t1 = std::min<uint64_t>(t0 + TB_TILE, in.n_items);
    uint64_t q[TB_Q];
    uint32_t c[TB_Q], pos[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = in.hash[std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, in.n_items - 1)];
    if (tid < 2) sread[tid] = read_of(in.km_off, 0, in.n_reads - 1, tid == 0 ? t0 : t1 - 1);
    lookup_many<true>(tv, q, c, pos);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t x = t0 + (uint64_t)r * TB_THREADS + tid;
        bool kept = false;
        if (x < in.n_items && tv.keys[pos[r]] == q[r]) { // whatever its count
            Span s;
            kept = span_of(in, read_of(in.km_off, sread[0], sread[1], x), x, &s);
            if (!kept) atomicOr(bad, 2u);
        }
        if (x < in.n_items) node[x] = kept ? pos[r] : VT_NONE;
        const uint64_t m = __ballot(kept);
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64;
        if (lane == 0) {
            wc[r * 4 + wv] = (uint32_t)__popcll(m);
            if (w0 < in.n_items) ws.wmask[w0 >> 6] = m;
        }
    }
    __syncthreads();
    tile_prefixes(wc, t0, in.n_items, ws);
}

// the three vote keys of item x of read rd, node nd: whole, forward end, reverse end
__device__ inline void item_keys(const VoteIn &in, const Fp &fp, uint64_t rd, uint64_t x, uint32_t nd, uint64_t (&key)[3]) {
    Span sp;
    if (!span_of(in, rd, x, &sp)) { // the count pass accepted it
        key[0] = key[1] = key[2] = 0;
        return;
    }
    const uint32_t rev = in.rev[x] ? 1u : 0u;
    const uint64_t a = in.read_off[rd] + fp.shift + sp.a, e = a + sp.len;
    const uint64_t pa = prefix_at(fp, a), re = suffix_at(fp, e);
    const uint64_t ml = mpow_dev(sp.len);
    const uint64_t whole = rev ? suffix_at(fp, a) - ml * re : prefix_at(fp, e) - pa * ml;
    const uint64_t fwd = prefix_at(fp, a + sp.shift_fwd) - pa * mpow_dev(sp.shift_fwd);
    const uint64_t rve = suffix_at(fp, e - sp.shift_rev) - mpow_dev(sp.shift_rev) * re;
    const uint64_t tag = 4ull * nd;
    key[0] = mix64(whole ^ mix64(tag));
    key[1] = mix64(fwd ^ mix64(tag + 2 + rev));
    key[2] = mix64(rve ^ mix64(tag + 2 + (1 - rev)));
}

__global__ __launch_bounds__(TB_THREADS) void vote_keys_kernel(VoteIn in, Fp fp, const uint32_t *__restrict__ node, CompactWs ws,
                                                               uint64_t *__restrict__ out) {
    __shared__ uint4 stage[(3 * TB_TILE + STAGE_PAD) / 2]; // 16-byte aligned: leave_run reads it in 16-byte pieces
    __shared__ uint64_t sread[2];
    uint64_t *skey = (uint64_t *)stage;
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, t1 = std::min<uint64_t>(t0 + TB_TILE, in.n_items);
    const uint64_t base = ws.tile_off[blockIdx.x], tot = ws.tile_off[blockIdx.x + 1] - base;
    if (tot == 0) return;
    if (tid < 2) sread[tid] = read_of(in.km_off, 0, in.n_reads - 1, tid == 0 ? t0 : t1 - 1);
    uint32_t slot[TB_Q];
    const uint32_t keep = tile_slots(ws, t0, in.n_items, slot);
    uint64_t *dst = out + 3 * base;
    const uint32_t shift = shift_of(dst);
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < TB_Q; r++) {
        if (!(keep & (1u << r))) continue;
        const uint64_t x = t0 + (uint64_t)r * TB_THREADS + tid;
        uint64_t key[3];
        item_keys(in, fp, read_of(in.km_off, sread[0], sread[1], x), x, node[x], key);
        uint64_t *o = skey + shift + 3 * slot[r];
        o[0] = key[0];
        o[1] = key[1];
        o[2] = key[2];
    }
    __syncthreads();
    leave_run(dst, skey, shift, (uint32_t)(3 * tot));
}

// per item of the table its votes w << 52 | e << 40 (0: not an item of the table); a key that the vote table lacks sets the flag
__global__ __launch_bounds__(TB_THREADS) void vote_score_kernel(TableView vt, VoteIn in, Fp fp, const uint32_t *__restrict__ node,
                                                                unsigned long long *__restrict__ score, uint32_t *__restrict__ bad) {
    __shared__ uint64_t sread[2];
    const int tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, t1 = std::min<uint64_t>(t0 + TB_TILE, in.n_items);
    if (tid < 2) sread[tid] = read_of(in.km_off, 0, in.n_reads - 1, tid == 0 ? t0 : t1 - 1);
    __syncthreads();
    uint64_t kw[TB_Q], kf[TB_Q], kr[TB_Q];
    uint32_t item = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) kw[r] = kf[r] = kr[r] = 0;
#pragma unroll 1
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t x = t0 + (uint64_t)r * TB_THREADS + tid;
        const uint32_t nd = x < in.n_items ? node[x] : VT_NONE;
        if (nd == VT_NONE) continue;
        uint64_t key[3];
        item_keys(in, fp, read_of(in.km_off, sread[0], sread[1], x), x, nd, key);
#pragma unroll
        for (int z = 0; z < TB_Q; z++) // a register array takes constant indices
            if (z == r) {
                kw[z] = key[0];
                kf[z] = key[1];
                kr[z] = key[2];
            }
        item |= 1u << r;
    }
    uint32_t cw[TB_Q], cf[TB_Q], cr[TB_Q];
    lookup_many<false>(vt, kw, cw, nullptr);
    lookup_many<false>(vt, kf, cf, nullptr);
    lookup_many<false>(vt, kr, cr, nullptr);
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t x = t0 + (uint64_t)r * TB_THREADS + tid;
        if (x >= in.n_items) continue;
        unsigned long long s = 0;
        if (item & (1u << r)) {
            if (cw[r] == 0 || cf[r] == 0 || cr[r] == 0) atomicOr(bad, 4u);
            const uint64_t w = std::min<uint64_t>(cw[r], 2047), e = std::min<uint64_t>((uint64_t)cf[r] + cr[r], 4095);
            s = (w << 52) | (e << 40);
        }
        score[x] = s;
    }
}

__global__ __launch_bounds__(VT_T) void vote_max_kernel(const uint32_t *__restrict__ node, const unsigned long long *__restrict__ score,
                                                        uint64_t n_items, uint64_t ordinal_base, unsigned long long *__restrict__ best) {
    const uint64_t x = (uint64_t)blockIdx.x * VT_T + threadIdx.x;
    if (x >= n_items) return;
    const uint32_t nd = node[x];
    if (nd != VT_NONE) atomicMax(best + nd, score[x] | (VT_ORD - (ordinal_base + x)));
}

__global__ __launch_bounds__(VT_T) void vote_ordinals_kernel(const uint64_t *__restrict__ best, uint64_t n, uint64_t *__restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * VT_T + threadIdx.x;
    if (i < n) rep[i] = best[i] ? VT_ORD - (best[i] & VT_ORD) : ~0ull;
}

// ---- what both calls do up to the host's look at the flag --------------------------------------------------------------------------
struct Plan {
    VoteIn in;
    uint64_t n_tiles = 0, n_kept = 0, n_blocks = 0;
    bool nothing = false; // no items, or an empty table: nothing to read or write
    Fp fp{};
    uint32_t *bad = nullptr, *node = nullptr;
    CompactWs ws{};
    unsigned long long *score = nullptr;
    uint64_t *fb = nullptr, *gb = nullptr, *pfb = nullptr, *prb = nullptr, *pf = nullptr, *pr = nullptr;
};

s2k_status plan_call(Call &c, s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t k, const uint8_t *d_bases,
                     const uint64_t *d_read_off, bool want_score, uint64_t ordinal_base, Plan *p) {
    if (k < 2 || k > 4096) return c.invalid("k < 2 (a node has no second minimizer) or k > 4096");
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    uint64_t ro0 = 0, ro1 = 0;
    c.fetch(&ro0, d_read_off, 8);
    c.fetch(&ro1, d_read_off + n_reads, 8);
    const Ends ends = read_ends(c, in->km_off, in->mn_off, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ends.mn0 != 0 || ends.n_triples > in->mn_capacity || ro1 < ro0)
        return c.invalid("km_off and mn_off must start at 0, mn_capacity must cover mn_off[n_reads], and read_off must not decrease");
    if (ordinal_base > VT_ORD + 1 || ends.n_items > VT_ORD + 1 - ordinal_base) return c.invalid("ordinal_base + the batch's items pass 2^40");
    const uint64_t n_items = ends.n_items, nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads >= (1ull << 40)) return c.invalid("too many items for one call");
    p->nothing = true;
    if (n_reads == 0) return S2K_OK;
    const uint64_t first = (uint64_t)d_bases + ro0, lead = first & 15u, end = lead + (ro1 - ro0), n_chunks = (end + 15) / 16;
    const uint64_t nb = (n_chunks + 1 + VT_BLOCK - 1) / VT_BLOCK; // entry n_chunks has a writer
    if (nb >= (1ull << 31)) return c.invalid("too many bases for one call");
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const auto node_p = L.take<uint32_t>(n_items);
    const auto cw = carve(L, n_items, std::max<uint64_t>(nt, 1));
    const auto score_p = L.take<unsigned long long>(want_score ? n_items : 0);
    const auto fb_p = L.take<uint64_t>(nb), gb_p = L.take<uint64_t>(nb), pfb_p = L.take<uint64_t>(nb), prb_p = L.take<uint64_t>(nb);
    const auto pf_p = L.take<uint64_t>(n_chunks + 1), pr_p = L.take<uint64_t>(n_chunks + 1);
    char *w = L.alloc(t->ctx);
    if (!w) return c.nomem();
    p->in = VoteIn{in->km_off, in->hash, in->mn_off, in->mn_j, in->mn_jend, in->rev, d_read_off, n_reads, n_items, k};
    p->n_tiles = nt;
    p->n_blocks = nb;
    p->bad = flag(w);
    p->node = node_p(w);
    p->ws = cw(w);
    p->score = score_p(w);
    p->fb = fb_p(w), p->gb = gb_p(w), p->pfb = pfb_p(w), p->prb = prb_p(w), p->pf = pf_p(w), p->pr = pr_p(w);
    p->fp = Fp{Stream{(const uint64_t *)(first - lead), lead, end, n_chunks}, p->pf, p->pr, lead - ro0};
    // 1. the count relation of every read, before a triple is indexed through it
    uint32_t hbad = c.check(p->bad, 16, p->bad, [&] {
        hipLaunchKernelGGL(vote_reads_kernel, dim3((unsigned)((n_reads + VT_T - 1) / VT_T)), dim3(VT_T), 0, c.st, p->in, p->bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("a read with n > 0 items must have n + k - 1 minimizer triples (a wrong k, or triples of another call), and km_off / "
                         "mn_off / read_off must not decrease");
    if (n_items == 0 || t->n == 0) return S2K_OK;
    // 2. the items of the table and their positions, 3. their slots
    hipLaunchKernelGGL(vote_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), p->in, p->node, p->ws, p->bad);
    c.launched();
    c.scan(p->ws.tile_kept, nt, p->ws.tile_off, cw.scan_tmp(w));
    c.fetch(&p->n_kept, p->ws.tile_off + nt, 8);
    c.fetch(&hbad, p->bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad) return c.invalid("a minimizer position lies outside its read or out of order");
    p->nothing = p->n_kept == 0;
    return S2K_OK;
}

// 4. PF and PR of the batch's bases
void fingerprints(Call &c, const Plan &p) {
    if (!c.ok()) return;
    const unsigned nb = (unsigned)p.n_blocks;
    hipLaunchKernelGGL(fp_block_kernel, dim3(nb), dim3(VT_T), 0, c.st, p.fp.s, p.fb, p.gb);
    hipLaunchKernelGGL(fp_scan_kernel, dim3(1), dim3(VT_T), 0, c.st, p.fb, p.gb, p.n_blocks, (p.n_blocks + VT_T - 1) / VT_T, p.pfb, p.prb);
    hipLaunchKernelGGL(fp_write_kernel, dim3(nb), dim3(VT_T), 0, c.st, p.fp.s, p.pfb, p.prb, p.pf, p.pr);
    c.launched();
}

bool seq_in_missing(const s2k_device_out *in) { return !in->km_off || !in->hash || !in->rev || !in->mn_off || !in->mn_j || !in->mn_jend; }

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_table_vote_keys(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t k, const uint8_t *d_bases,
                               const uint64_t *d_read_off, uint64_t *d_keys, uint64_t capacity, uint64_t *n_keys) {
    if (n_keys) *n_keys = 0;
    if (!t || !in || !n_keys || seq_in_missing(in) || !d_read_off) return S2K_ERR_INVALID_ARG;
    Call c(t->ctx, "s2k_table_vote_keys");
    Plan p;
    const s2k_status s = plan_call(c, t, n_reads, in, k, d_bases, d_read_off, false, 0, &p);
    if (s != S2K_OK || p.nothing) return s;
    *n_keys = 3 * p.n_kept;
    if (!d_keys) return S2K_OK;
    if (*n_keys > capacity) return S2K_ERR_CAPACITY;
    if (!d_bases) return S2K_ERR_INVALID_ARG;
    fingerprints(c, p);
    if (c.ok()) {
        hipLaunchKernelGGL(vote_keys_kernel, dim3((unsigned)p.n_tiles), dim3(TB_THREADS), 0, c.st, p.in, p.fp, p.node, p.ws, d_keys);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_table_vote_representatives(s2k_table *t, s2k_table *vote_table, uint64_t n_reads, const s2k_device_out *in, uint32_t k,
                                          const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t ordinal_base, uint64_t *d_best) {
    if (!t || !vote_table || !in || seq_in_missing(in) || !d_read_off || (t->n && !d_best)) return S2K_ERR_INVALID_ARG;
    Call c(t->ctx, "s2k_table_vote_representatives");
    if (ctx_device(vote_table->ctx) != ctx_device(t->ctx)) return c.invalid("the two tables live on different devices");
    Plan p;
    const s2k_status s = plan_call(c, t, n_reads, in, k, d_bases, d_read_off, true, ordinal_base, &p);
    if (s != S2K_OK || p.nothing) return s;
    if (!d_bases) return S2K_ERR_INVALID_ARG;
    fingerprints(c, p);
    if (c.ok()) {
        hipLaunchKernelGGL(vote_score_kernel, dim3((unsigned)p.n_tiles), dim3(TB_THREADS), 0, c.st, vote_table->view(), p.in, p.fp, p.node, p.score,
                           p.bad);
        c.launched();
    }
    uint32_t hbad = 0;
    c.fetch(&hbad, p.bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad) return c.invalid("a vote key is not in vote_table: it is not the table counted from these batches' keys");
    hipLaunchKernelGGL(vote_max_kernel, dim3((unsigned)((p.in.n_items + VT_T - 1) / VT_T)), dim3(VT_T), 0, c.st, p.node, p.score, p.in.n_items,
                       ordinal_base, (unsigned long long *)d_best);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_vote_ordinals(s2k_ctx *ctx, const uint64_t *d_best, uint64_t n, uint64_t *d_rep) {
    if (!ctx || (n && (!d_best || !d_rep))) return S2K_ERR_INVALID_ARG;
    if (n == 0) return S2K_OK;
    Call c(ctx, "s2k_vote_ordinals");
    if (n >= (1ull << 39)) return c.invalid("too many nodes for one call");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    hipLaunchKernelGGL(vote_ordinals_kernel, dim3((unsigned)((n + VT_T - 1) / VT_T)), dim3(VT_T), 0, c.st, d_best, n, d_rep);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

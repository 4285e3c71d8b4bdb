// s2k_seq.hip -- base-space sequences for the graph's nodes and unitigs (include/s2k.h: s2k_table_representatives,
// s2k_table_node_sequences, s2k_unitig_sequences).
//
// Representatives: the filter's fused look-up with ranks (lookup_many<true>), then one 64-bit atomicMin per item that is in the
// table: d_rep[rank] = min(d_rep[rank], ordinal_base + x).  min does not depend on the order, so d_rep is a function of the input.
//
// Node sequences, per batch:
//  1. nodeseq_reads_kernel: per read, items n and triples m must satisfy n == 0 || m == n + k - 1 (src/lib.rs:231-258); km_off and
//     mn_off non-decreasing.  One flag word, read by the host before any triple is indexed through the relation.
//  2. nodeseq_count_kernel: tiles of TB_TILE items, the look-up fused in.  An item x is its node's representative when its hash is
//     key `rank` and d_rep[rank] == ordinal_base + x; then its read comes from a search of km_off narrowed to the tile's reads, its
//     first triple is mn_off[r] + (x - km_off[r]), and len = mn_jend[last] - mn_j[first] + 1.  Per item 4 B len (0: not a
//     representative) + 4 B rank.  Every position is checked against the read's length (flag word).
//  3. launch_scan_u32 over the lengths: the pool offset of every representative, in item order (so the pool is ordered by ordinal).
//  4. nodeseq_write_kernel (only when the pool has room): the item's lane writes the node's record; then the wave copies the bytes of
//     its representatives one after the other, 16 B per lane to 16-byte aligned pool addresses, each assembled from the two or three
//     aligned 8-byte words that hold the source bytes (fetch16); the unaligned head and tail of a copy go bytewise.
//
// Unitig sequences (the stitch):
//  1. piece_len_kernel, one lane per member p: two dependent gathers (members[p], then seq_len / shift / rev of its node) give the
//     bytes the member contributes, shift(u); every node record it touches is checked (flag word).
//  2. unitig_last_kernel, one lane per unitig: uni_off is checked; the last member of a unitig that is not circular contributes its
//     whole sequence.
//  3. launch_scan_u32 over the pieces -> piece_off; the host reads the flag and the total.
//  4. unitig_off_kernel: out_off[t] = piece_off[uni_off[t]], and the overlap that leaves each oriented unitig.
//  5. stitch_kernel, output-ordered: lane g of the grid writes bytes [16 g, 16 g + 16) of d_out with one 16-byte store.  A block
//     covers 4 KiB of output; two lanes find the block's first and last piece by a search of piece_off, every lane then searches
//     that range (a handful of steps) for the piece that holds its first byte and walks on from there.  The bytes of a piece come
//     from fetch16; a member read on the other strand takes them from the far end, byte-reversed (two v_perm-able 64-bit swaps and
//     a 128-bit shift) and complemented in registers (three SWAR byte tests per word; no table).  The last chunk of d_out, when it
//     is not whole, goes bytewise.
//
// Workspace (the context's grow-only count workspace): representatives none; node sequences 16 B per item; the stitch 12 B per
// member.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_bytes_dev.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_stitch_dev.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

constexpr uint32_t SQ_NONE = 0xFFFFFFFFu;

// ---- representatives --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB_THREADS) void rep_kernel(TableView tv, const uint64_t *__restrict__ hash, uint64_t n_items, uint64_t ordinal_base,
                                                         unsigned long long *__restrict__ rep) {
    const uint64_t base = (uint64_t)blockIdx.x * TB_TILE + threadIdx.x;
    uint64_t q[TB_Q];
    uint32_t c[TB_Q], pos[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = hash[std::min<uint64_t>(base + (uint64_t)r * TB_THREADS, n_items - 1)];
    lookup_many<true>(tv, q, c, pos);
    if (tv.n == 0) return;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t x = base + (uint64_t)r * TB_THREADS;
        if (x < n_items && tv.keys[pos[r]] == q[r]) atomicMin(rep + pos[r], (unsigned long long)(ordinal_base + x)); // whatever its count
    }
}

// ---- node sequences ---------------------------------------------------------------------------------------------------------------
struct SeqIn {
    const uint64_t *km_off, *hash, *mn_off;
    const uint32_t *mn_j, *mn_jend;
    const uint8_t *rev;
    const uint64_t *read_off;
    uint64_t n_reads, n_items;
    uint32_t k;
};

__global__ __launch_bounds__(SQ_T) void nodeseq_reads_kernel(SeqIn in, uint32_t *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * SQ_T + threadIdx.x;
    if (r >= in.n_reads) return;
    const uint64_t a = in.km_off[r], b = in.km_off[r + 1], c = in.mn_off[r], d = in.mn_off[r + 1];
    bool ok = a <= b && c <= d && in.read_off[r] <= in.read_off[r + 1];
    if (r == 0) ok = ok && a == 0 && c == 0;
    if (ok && b > a) ok = d - c == (b - a) + in.k - 1;
    if (!ok) atomicOr(bad, 1u);
}

// what the representative x of read rd is made of: first and last base inside the read, the two shifts; false when a position
// breaks the rules (then nothing may be read from the bases through it)
struct Span {
    uint32_t a, len, shift_fwd, shift_rev;
};
__device__ inline bool span_of(const SeqIn &in, uint64_t rd, uint64_t x, Span *s) {
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

__global__ __launch_bounds__(TB_THREADS) void nodeseq_count_kernel(TableView tv, SeqIn in, uint64_t ordinal_base,
                                                                   const unsigned long long *__restrict__ rep, uint32_t *__restrict__ len,
                                                                   uint32_t *__restrict__ node, uint32_t *__restrict__ bad) {
    __shared__ uint64_t sread[2];
    const int tid = threadIdx.x;
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
        if (x >= in.n_items) continue;
        uint32_t l = 0, nd = SQ_NONE;
        if (tv.n && tv.keys[pos[r]] == q[r] && rep[pos[r]] == ordinal_base + x) {
            Span s;
            if (span_of(in, read_of(in.km_off, sread[0], sread[1], x), x, &s)) {
                l = s.len;
                nd = pos[r];
            } else
                atomicOr(bad, 2u);
        }
        len[x] = l;
        node[x] = nd;
    }
}

struct NodeOut {
    uint64_t *seq_off;
    uint32_t *seq_len, *shift_fwd, *shift_rev;
    uint8_t *rev, *pool;
};

// the wave copies n bytes from src to dst: bytewise up to the first 16-byte aligned dst address, then 16 B per lane, then bytewise
__device__ inline void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, int lane) {
    const uint32_t head = std::min<uint32_t>(n, (uint32_t)((16u - ((uint64_t)dst & 15u)) & 15u));
    if ((uint32_t)lane < head) dst[lane] = src[lane];
    const uint32_t nc = (n - head) >> 4;
    for (uint32_t ch = lane; ch < nc; ch += 64) {
        uint64_t lo, hi;
        fetch16(src + head + 16ull * ch, 16, lo, hi);
        *(ulonglong2 *)(dst + head + 16ull * ch) = make_ulonglong2(lo, hi);
    }
    const uint32_t i = head + 16u * nc + (uint32_t)lane; // fewer than 16 bytes are left
    if (i < n) dst[i] = src[i];
}

__global__ __launch_bounds__(SQ_T) void nodeseq_write_kernel(SeqIn in, const uint8_t *__restrict__ bases, const uint32_t *__restrict__ len,
                                                             const uint32_t *__restrict__ node, const uint64_t *__restrict__ item_off,
                                                             uint64_t pool_used, NodeOut out) {
    const uint64_t x = (uint64_t)blockIdx.x * SQ_T + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t nd = x < in.n_items ? node[x] : SQ_NONE;
    uint64_t src = 0, dst = 0;
    uint32_t n = 0;
    if (nd != SQ_NONE) {
        const uint64_t rd = read_of(in.km_off, 0, in.n_reads - 1, x);
        Span s;
        if (span_of(in, rd, x, &s)) { // the count pass accepted it
            n = len[x];
            src = in.read_off[rd] + s.a;
            dst = pool_used + item_off[x];
            out.seq_off[nd] = dst;
            out.seq_len[nd] = s.len;
            out.shift_fwd[nd] = s.shift_fwd;
            out.shift_rev[nd] = s.shift_rev;
            out.rev[nd] = in.rev[x] ? 1 : 0;
        }
    }
    uint64_t m = __ballot(n != 0);
    while (m) {
        const int l = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const uint64_t s = __shfl(src, l, 64), d = __shfl(dst, l, 64);
        wave_copy(out.pool + d, bases + s, __shfl(n, l, 64), lane);
    }
}

// ---- the stitch ------------------------------------------------------------------------------------------------------------------
// the largest p in [lo, hi] with piece_off[p] <= pos (piece_off[lo] <= pos holds): the piece that holds byte pos when pos < total
__device__ inline uint64_t piece_of(const uint64_t *__restrict__ piece_off, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (piece_off[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(SQ_T) void stitch_kernel(const uint32_t *__restrict__ members, uint64_t n_members, const uint64_t *__restrict__ piece_off,
                                                      NodeView nv, uint8_t *__restrict__ out, uint64_t total) {
    __shared__ uint64_t srange[2];
    const uint64_t b0 = (uint64_t)blockIdx.x * (SQ_T * 16);
    if (threadIdx.x < 2) srange[threadIdx.x] = piece_of(piece_off, 0, n_members - 1, threadIdx.x ? std::min<uint64_t>(b0 + SQ_T * 16, total) - 1 : b0);
    __syncthreads();
    uint64_t pos = b0 + (uint64_t)threadIdx.x * 16;
    if (pos >= total) return;
    const uint32_t want = (uint32_t)std::min<uint64_t>(16, total - pos);
    uint64_t p = piece_of(piece_off, srange[0], srange[1], pos);
    uint64_t lo = 0, hi = 0, pe = piece_off[p + 1], ps = piece_off[p];
    uint32_t filled = 0;
    while (filled < want) { // pos < total, so a piece with bytes left lies at or after p
        if (pe <= pos) {
            p++;
            ps = pe;
            pe = piece_off[p + 1];
            continue;
        }
        const uint32_t n = (uint32_t)std::min<uint64_t>(want - filled, pe - pos);
        const uint32_t u = members[p], i = u >> 1;
        const bool fwd = (u & 1u) == nv.rev[i];
        const uint64_t so = nv.seq_off[i], k = pos - ps;
        uint64_t a, b;
        if (fwd) {
            fetch16(nv.pool + so + k, n, a, b);
            keep_low(n, a, b);
        } else { // bytes k .. k + n - 1 of the reverse complement: the node's bytes len - k - n .. len - k - 1, backwards
            fetch16(nv.pool + so + (nv.seq_len[i] - k - n), n, a, b);
            revcomp_low(n, a, b);
        }
        shl_bytes(filled, a, b);
        lo |= a;
        hi |= b;
        filled += n;
        pos += n;
    }
    uint8_t *o = out + (pos - filled);
    if (want == 16) *(ulonglong2 *)o = make_ulonglong2(lo, hi);
    else
        for (uint32_t x = 0; x < want; x++) o[x] = (uint8_t)((x < 8 ? lo >> (8 * x) : hi >> (8 * (x - 8))) & 0xFFu);
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_table_representatives(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint64_t ordinal_base, uint64_t *d_rep) {
    if (!t || !in || !in->km_off || !in->hash || (t->n && !d_rep)) return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Call c(t->ctx, "s2k_table_representatives");
    const Ends ends = read_ends(c, in->km_off, in->mn_off, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ordinal_base + ends.n_items < ordinal_base)
        return c.invalid("in->km_off must start at 0, and the ordinals must fit 64 bits");
    if (ends.n_items == 0 || t->n == 0) return S2K_OK;
    const uint64_t nt = (ends.n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32)) return c.invalid("too many items for one call");
    hipLaunchKernelGGL(rep_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), in->hash, ends.n_items, ordinal_base,
                       (unsigned long long *)d_rep);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_table_node_sequences(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t k, const uint8_t *d_bases,
                                    const uint64_t *d_read_off, uint64_t ordinal_base, const uint64_t *d_rep, const s2k_node_seqs *nodes,
                                    uint64_t pool_used, uint64_t *n_bytes) {
    if (n_bytes) *n_bytes = 0;
    if (!t || !in || !n_bytes || !in->km_off || !in->hash || !in->rev || !in->mn_off || !in->mn_j || !in->mn_jend || !d_read_off ||
        (t->n && !d_rep))
        return S2K_ERR_INVALID_ARG;
    Call c(t->ctx, "s2k_table_node_sequences");
    const bool want = nodes && nodes->pool;
    if (want && (!nodes->seq_off || !nodes->seq_len || !nodes->shift_fwd || !nodes->shift_rev || !nodes->rev)) return S2K_ERR_INVALID_ARG;
    if (k < 2 || k > 4096) return c.invalid("k < 2 (a node has no second minimizer) or k > 4096");
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const Ends ends = read_ends(c, in->km_off, in->mn_off, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ends.mn0 != 0 || ends.n_triples > in->mn_capacity || ordinal_base + ends.n_items < ordinal_base)
        return c.invalid("km_off and mn_off must start at 0, and mn_capacity must cover mn_off[n_reads]");
    const uint64_t n_items = ends.n_items;
    const uint64_t nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads >= (1ull << 40)) return c.invalid("too many items for one call");
    if (n_reads == 0) return S2K_OK;
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const auto len_p = L.take<uint32_t>(n_items), node_p = L.take<uint32_t>(n_items);
    const auto off_p = L.take<uint64_t>(n_items + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_items));
    char *w = L.alloc(t->ctx);
    if (!w) return c.nomem();
    uint32_t *bad = flag(w), *len = len_p(w), *node = node_p(w);
    uint64_t *item_off = off_p(w);
    const SeqIn si{in->km_off, in->hash, in->mn_off, in->mn_j, in->mn_jend, in->rev, d_read_off, n_reads, n_items, k};
    // 1. the count relation of every read, before a triple is indexed through it
    uint32_t hbad = c.check(bad, 16, bad, [&] {
        hipLaunchKernelGGL(nodeseq_reads_kernel, dim3((unsigned)((n_reads + SQ_T - 1) / SQ_T)), dim3(SQ_T), 0, c.st, si, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("a read with n > 0 items must have n + k - 1 minimizer triples (a wrong k, or triples of another call), and km_off / "
                         "mn_off / read_off must not decrease");
    if (n_items == 0 || t->n == 0) return S2K_OK;
    // 2. lengths, 3. offsets
    hipLaunchKernelGGL(nodeseq_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), si, ordinal_base,
                       (const unsigned long long *)d_rep, len, node, bad);
    c.launched();
    c.scan(len, n_items, item_off, tmp_p(w));
    uint64_t total = 0;
    c.fetch(&total, item_off + n_items, 8);
    c.fetch(&hbad, bad, 4);
    if (!c.sync()) return c.device_error();
    if (hbad) return c.invalid("a minimizer position lies outside its read or out of order");
    *n_bytes = total;
    if (!want || total == 0) return S2K_OK;
    if (pool_used > nodes->pool_capacity || total > nodes->pool_capacity - pool_used) return S2K_ERR_CAPACITY;
    if (!d_bases) return S2K_ERR_INVALID_ARG;
    // 4. records and bytes
    const NodeOut no{nodes->seq_off, nodes->seq_len, nodes->shift_fwd, nodes->shift_rev, nodes->rev, nodes->pool};
    hipLaunchKernelGGL(nodeseq_write_kernel, dim3((unsigned)((n_items + SQ_T - 1) / SQ_T)), dim3(SQ_T), 0, c.st, si, d_bases, len, node, item_off,
                       pool_used, no);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_unitig_sequences(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs,
                                uint64_t n_nodes, const s2k_node_seqs *nodes, uint64_t *d_out_off, uint8_t *d_out, uint32_t *d_overlap,
                                uint64_t capacity, uint64_t *n_bases) {
    if (n_bases) *n_bases = 0;
    if (!ctx || !n_bases || !d_uni_off || !nodes) return S2K_ERR_INVALID_ARG;
    if (n_unitigs && (!d_members || !d_circular || !nodes->seq_off || !nodes->seq_len || !nodes->shift_fwd || !nodes->shift_rev || !nodes->rev))
        return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_unitig_sequences");
    if (n_nodes >= (1ull << 31) || n_unitigs > n_nodes || ((uint64_t)d_out & 15u))
        return c.invalid("2^31 nodes or more, more unitigs than nodes, or d_out not 16-byte aligned");
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
    uint32_t *bad = flag(w), *len = len_p(w);
    uint64_t *piece_off = off_p(w);
    const NodeView nv{nodes->seq_off, nodes->seq_len, nodes->shift_fwd, nodes->shift_rev, nodes->rev, nodes->pool, nodes->pool_capacity, n_nodes};
    const unsigned gu = (unsigned)((n_unitigs + 1 + SQ_T - 1) / SQ_T);
    uint64_t total = 0;
    const uint32_t hbad = stitch_offsets(c, d_uni_off, d_members, d_circular, n_unitigs, n_members, nv, bad, len, piece_off, tmp_p(w), &total);
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("uni_off is not the offsets of n_unitigs non-empty unitigs over n_nodes members, a member names a node >= n_nodes, or a "
                         "node record is inconsistent (rev > 1, a shift above seq_len, bytes outside the pool)");
    *n_bases = total;
    if (d_out && total > capacity) return S2K_ERR_CAPACITY;
    if (d_out && total && !nodes->pool) return S2K_ERR_INVALID_ARG;
    if (d_out_off || d_overlap) {
        hipLaunchKernelGGL(unitig_off_kernel, dim3(gu), dim3(SQ_T), 0, c.st, d_uni_off, d_members, n_unitigs, nv, piece_off, d_out_off, d_overlap);
        c.launched();
    }
    if (c.ok() && d_out && total) {
        const uint64_t nb = (total + SQ_T * 16 - 1) / (SQ_T * 16);
        if (nb >= (1ull << 31)) return c.invalid("2^43 bases or more");
        hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)nb), dim3(SQ_T), 0, c.st, d_members, n_members, piece_off, nv, d_out, total);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

// s2k_untangle.hip -- the graph surgery behind a resolution: every resolved unitig duplicated once per matched in-edge / out-edge pair,
// and the contigs of the untangled graph expanded back to node members (include/s2k.h: s2k_graph_untangle, s2k_unitig_expand;
// DESIGN.md §3.15).
//
// s2k_graph_untangle:
//  1. untangle_check_kernel, one lane per oriented unitig V: the CSR rules of simplify_check_kernel with ids < 2 T; resolved bytes 0 / 1;
//     for a resolved unitig out(2 t) == out(2 t + 1) >= 2, every in-edge a of V (the twins of the row of V ^ 1) has its partner in
//     the row of V, no two in-edges share one, partner[tw(partner[a])] == tw(a).  Every read is clamped to the arrays whatever
//     they hold: a row bound past n_edges empties the row, an id or an edge index is compared before it indexes.  One flag word.
//  2. copies_kernel, one lane per unitig: ncopies; launch_scan_u32 gives copy_off, and T' with it.
//  3. degree_kernel, one lane per new oriented copy C = 2 c + s: origin[c] by a binary search of copy_off, the out-degree of C (1
//     for a copy of a resolved unitig, out(2 origin + s) otherwise), and, for s == 0, the copy's count.
//  4. launch_scan_u32 over the degrees: the new row offsets.  Rows come in the order of C, so the keys ascend between rows.
//  5. untangle_write_kernel, one lane per new oriented copy: a copy strand of a resolved unitig writes its one edge; an unresolved A
//     walks its old row, maps every destination and places the keys by repeated selection (the map is monotone between unitigs,
//     not between the two strands of one resolved unitig).  tw(e) is one search of one row, its bounds loaded before the probes.
//     Every slot has one writer: no atomic touches an output.
//
// s2k_unitig_expand:
//  1. expand_check_kernel: inner and outer uni_off strictly ascending from 0 to n_nodes / n_copies; per outer member (a piece) C <
//     2 T', origin < T, its length = the members of its origin, and its contig by a binary search of the outer uni_off.
//  2. launch_scan_u32 over the piece lengths: piece_off, and M with it.
//  3. expand_write_kernel, output-ordered: lane x of block b takes slot 256 b + x.  Two lanes search the pieces of the block's first
//     and last slot once, every lane then searches that short range, as stitch_kernel does.  contig_kernel: one lane per contig.
//
// Workspace (the context's grow-only count workspace).  Untangle, sized before T' is known by T' <= T + n_edges / 2 (the copies of a
// resolved unitig number half the edges of its two rows): 12 B per unitig (ncopies, copy_off) + 28 B per copy bound (origin, and per
// oriented copy the degree and the row offset) = 40 B per unitig + 14 B per edge, and the scans' block sums.  Expand: 16 B per
// copy (piece length, piece offset, contig).
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

// ---- the check: nothing here trusts what it reads ---------------------------------------------------------------------------------
struct Unchecked {
    Csr g;
    uint64_t n_ids, n_edges;
    const uint8_t *resolved;
    const uint32_t *partner;

    // the bounds of row u (u < n_ids), an empty row when they break the rules
    __device__ __forceinline__ bool row(uint64_t u, uint64_t *a, uint64_t *b) const {
        if (csr_row_ok(g.row_off, u, n_ids, n_edges, a, b)) return true;
        *a = *b = 0;
        return false;
    }
    __device__ __forceinline__ uint32_t find(uint32_t A, uint32_t B) const { // A < n_ids
        uint64_t lo, hi;
        row(A, &lo, &hi);
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint32_t v = g.dst[mid];
            if (v < B) lo = mid + 1;
            else if (v > B) hi = mid;
            else return (uint32_t)mid;
        }
        return NONE;
    }
    // the in-edge of V that is the twin of edge f of the row of V ^ 1, NONE when f names no id or the twin is missing
    __device__ __forceinline__ uint32_t in_edge(uint32_t V, uint64_t f) const {
        const uint32_t X = g.dst[f];
        return X < n_ids ? find(X ^ 1u, V) : NONE;
    }
    // the rules of one strand V of a resolved unitig
    __device__ bool strand_ok(uint32_t V) const {
        uint64_t ia, ib, oa, ob;
        row(V ^ 1u, &ia, &ib);
        row(V, &oa, &ob);
        if (ib - ia != ob - oa || ob - oa < 2) return false;
        for (uint64_t f = ia; f < ib; f++) {
            const uint32_t a = in_edge(V, f);
            if (a == NONE) return false;
            const uint32_t b = partner[a];
            if (b < oa || b >= ob) return false; // ob <= n_edges: b indexes dst
            for (uint64_t h = ia; h < f; h++) {  // quadratic in a hub's degree: slow, never wrong
                const uint32_t a2 = in_edge(V, h);
                if (a2 != NONE && partner[a2] == b) return false;
            }
            const uint32_t Y = g.dst[b], X = g.dst[f];
            if (Y >= n_ids) return false;
            const uint32_t tb = find(Y ^ 1u, V ^ 1u), ta = find(V ^ 1u, X); // tw(b) enters V ^ 1; tw(a) leaves it
            if (tb == NONE || ta == NONE || partner[tb] != ta) return false;
        }
        return true;
    }
};

__global__ __launch_bounds__(UT) void untangle_check_kernel(Unchecked c, uint32_t *__restrict__ bad) {
    bool ok = true;
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < c.n_ids; u += (uint64_t)gridDim.x * UT) {
        uint64_t a, b;
        if (!c.row(u, &a, &b)) ok = false;
        for (uint64_t e = a; e < b; e++)
            if (c.g.dst[e] >= c.n_ids) ok = false;
        const uint8_t r = c.resolved[u >> 1];
        if (r > 1) ok = false;
        else if (r && !c.strand_ok((uint32_t)u)) ok = false;
    }
    if (!ok) atomicOr(bad, 1u);
}

// ---- untangle: the input has passed the check --------------------------------------------------------------------------------------
struct Tangle {
    Csr g;
    const uint8_t *resolved;
    const uint32_t *partner;
    const uint64_t *copy_off; // T + 1

    __device__ __forceinline__ uint64_t base(uint64_t t) const { return g.row_off[2 * t + 1]; }
    __device__ __forceinline__ uint64_t deg(uint64_t t) const { return g.row_off[2 * t + 2] - g.row_off[2 * t + 1]; }
    // the new id of the destination of e = (A -> dst[e]).  A copy index outside its unitig can only come from an input whose twin
    // symmetry, which is trusted, does not hold: it becomes copy 0, and every write stays inside the arrays.
    __device__ __forceinline__ uint64_t new_dst(uint32_t A, uint64_t e) const {
        const uint32_t B = g.dst[e];
        const uint64_t tb = B >> 1;
        uint64_t j = 0;
        if (resolved[tb]) {
            const uint64_t x = (B & 1u) ? partner[e] : find_edge(g, B ^ 1u, A ^ 1u); // odd: the edge that leaves 2 tb + 1; even: tw(e)
            j = x - base(tb);
            if (j >= deg(tb)) j = 0;
        }
        return 2 * (copy_off[tb] + j) + (B & 1u);
    }
};

__global__ __launch_bounds__(UT) void copies_kernel(Csr g, const uint8_t *__restrict__ resolved, uint64_t n_unitigs, uint32_t *__restrict__ ncopies,
                                                    unsigned long long *__restrict__ n_duplicated) {
    unsigned long long dup = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * UT + threadIdx.x; t < n_unitigs; t += (uint64_t)gridDim.x * UT) {
        const bool r = resolved[t] != 0;
        ncopies[t] = r ? (uint32_t)(g.row_off[2 * t + 1] - g.row_off[2 * t]) : 1u;
        dup += r;
    }
    block_add(dup, n_duplicated);
}

// floor(cnt * w / S) for w <= S, S > 0, without floating point: (cnt / S) * w + ((cnt % S) * w) / S; the product passes 64 bits only
// when S does 32, and its quotient is below w
__device__ __forceinline__ uint64_t share_of(uint64_t cnt, uint64_t w, uint64_t S) {
    const uint64_t r = cnt % S;
    uint64_t hi = __umul64hi(r, w), lo = r * w, q = 0;
    if (hi == 0) q = lo / S;
    else
        for (int i = 0; i < 64; i++) { // hi < S: one quotient bit per step
            const bool carry = hi >> 63;
            hi = hi << 1 | lo >> 63;
            lo <<= 1;
            q <<= 1;
            if (carry || hi >= S) hi -= S, q |= 1u;
        }
    return (cnt / S) * w + q;
}

__global__ __launch_bounds__(UT) void degree_kernel(Tangle k, uint64_t n_unitigs, uint64_t n_new_ids, uint32_t *__restrict__ origin,
                                                    uint32_t *__restrict__ degree, const uint64_t *__restrict__ uni_count,
                                                    const uint32_t *__restrict__ edge_counts, uint64_t *__restrict__ copy_count) {
    for (uint64_t C = (uint64_t)blockIdx.x * UT + threadIdx.x; C < n_new_ids; C += (uint64_t)gridDim.x * UT) {
        const uint64_t c = C >> 1;
        uint64_t lo = 0, hi = n_unitigs - 1; // the largest t with copy_off[t] <= c
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (k.copy_off[mid] <= c) lo = mid;
            else hi = mid - 1;
        }
        const uint64_t t = lo, A = 2 * t + (C & 1);
        const bool r = k.resolved[t] != 0;
        degree[C] = r ? 1u : (uint32_t)(k.g.row_off[A + 1] - k.g.row_off[A]);
        if (C & 1) continue;
        origin[c] = (uint32_t)t;
        if (!copy_count) continue;
        uint64_t cnt = uni_count[t];
        if (r) { // w_j = the count of a_j = tw(base + j), S = their sum over the copies
            const uint64_t b = k.base(t), d = k.deg(t), j = c - k.copy_off[t];
            uint64_t S = 0, w = 0;
            for (uint64_t i = 0; i < d; i++) {
                const uint32_t a = find_edge(k.g, k.g.dst[b + i] ^ 1u, (uint32_t)(2 * t));
                const uint64_t x = a != NONE ? edge_counts[a] : 0;
                S += x;
                if (i == j) w = x;
            }
            cnt = S ? share_of(cnt, w, S) : 0;
        }
        copy_count[c] = cnt;
    }
}

__global__ __launch_bounds__(UT) void untangle_write_kernel(Tangle k, uint64_t n_new_ids, const uint32_t *__restrict__ origin,
                                                            const uint64_t *__restrict__ new_row, uint64_t *__restrict__ keys,
                                                            uint64_t *__restrict__ src_edge) {
    for (uint64_t C = (uint64_t)blockIdx.x * UT + threadIdx.x; C < n_new_ids; C += (uint64_t)gridDim.x * UT) {
        const uint64_t c = C >> 1, t = origin[c], o = new_row[C];
        const uint32_t A = (uint32_t)(2 * t + (C & 1));
        if (k.resolved[t]) { // copy j: its reverse strand leaves over base + j, its forward strand over the partner of that edge's twin
            uint64_t e = k.base(t) + (c - k.copy_off[t]);
            if (!(C & 1)) e = k.partner[find_edge(k.g, k.g.dst[e] ^ 1u, A)];
            if (keys) keys[o] = C << 32 | k.new_dst(A, e);
            if (src_edge) src_edge[o] = e;
            continue;
        }
        const uint64_t a = k.g.row_off[A], n = k.g.row_off[A + 1] - a;
        uint64_t floor_v = 0; // the row's keys in ascending new destination: the smallest one not yet written (they are distinct)
        for (uint64_t i = 0; i < n; i++) {
            uint64_t best = ~0ull, best_e = 0;
            for (uint64_t e = a; e < a + n; e++) {
                const uint64_t V = k.new_dst(A, e);
                if (V >= floor_v && V < best) best = V, best_e = e;
            }
            if (keys) keys[o + i] = C << 32 | best;
            if (src_edge) src_edge[o + i] = best_e;
            floor_v = best + 1;
        }
    }
}

// ---- expand -----------------------------------------------------------------------------------------------------------------------
constexpr int EX_T = 256; // lanes of a block of the write kernel, and the slots it takes

struct Decomp {
    const uint64_t *uni_off;
    const uint32_t *members;
    const uint8_t *circular;
    uint64_t n_unitigs, n_nodes;
};

struct Pieces {
    uint32_t *len;     // per outer member: the members of its origin
    uint32_t *contig;  // per outer member
    uint64_t *off;     // n_copies + 1
};

__device__ __forceinline__ bool offsets_ok(const Decomp &d, uint64_t t) { // entry t of d.uni_off, t <= n_unitigs
    const uint64_t a = d.uni_off[t];
    if (t == 0 && a != 0) return false;
    return t == d.n_unitigs ? a == d.n_nodes : a < d.uni_off[t + 1];
}

__global__ __launch_bounds__(UT) void expand_check_kernel(Decomp outer, Decomp inner, const uint32_t *__restrict__ origin, Pieces p,
                                                          uint32_t *__restrict__ bad) {
    bool ok = true;
    const uint64_t i0 = (uint64_t)blockIdx.x * UT + threadIdx.x, stride = (uint64_t)gridDim.x * UT;
    for (uint64_t t = i0; t <= inner.n_unitigs; t += stride)
        if (!offsets_ok(inner, t)) ok = false;
    for (uint64_t t = i0; t <= outer.n_unitigs; t += stride)
        if (!offsets_ok(outer, t)) ok = false;
    for (uint64_t x = i0; x < outer.n_nodes; x += stride) { // outer.n_nodes = T' pieces
        const uint32_t C = outer.members[x];
        uint32_t len = 0;
        if (C >= 2 * outer.n_nodes) ok = false;
        else {
            const uint32_t t = origin[C >> 1];
            if (t >= inner.n_unitigs) ok = false;
            else len = (uint32_t)(inner.uni_off[t + 1] - inner.uni_off[t]);
        }
        p.len[x] = len;
        uint64_t lo = 0, hi = outer.n_unitigs - 1; // the largest contig with uni_off <= x; the indices stay inside whatever it holds
        while (lo < hi) {
            const uint64_t mid = (lo + hi + 1) >> 1;
            if (outer.uni_off[mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        p.contig[x] = (uint32_t)lo;
    }
    if (!ok) atomicOr(bad, 1u);
}

// the largest p in [lo, hi] with off[p] <= pos (off[lo] <= pos holds)
__device__ inline uint64_t piece_of(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct Expanded {
    uint32_t *members, *node_unitig, *node_pos, *node_origin;
};

__global__ __launch_bounds__(EX_T) void expand_write_kernel(Decomp outer, Decomp inner, const uint32_t *__restrict__ origin, Pieces p, uint64_t total,
                                                            Expanded out) {
    __shared__ uint64_t srange[2];
    const uint64_t b0 = (uint64_t)blockIdx.x * EX_T;
    if (threadIdx.x < 2) srange[threadIdx.x] = piece_of(p.off, 0, outer.n_nodes - 1, threadIdx.x ? std::min<uint64_t>(b0 + EX_T, total) - 1 : b0);
    __syncthreads();
    const uint64_t m = b0 + threadIdx.x;
    if (m >= total) return;
    const uint64_t x = piece_of(p.off, srange[0], srange[1], m), i = m - p.off[x];
    const uint32_t C = outer.members[x], contig = p.contig[x];
    const uint64_t t = origin[C >> 1], a = inner.uni_off[t], len = inner.uni_off[t + 1] - a;
    const uint32_t u = (C & 1u) ? inner.members[a + (len - 1 - i)] ^ 1u : inner.members[a + i];
    if (out.members) out.members[m] = (uint32_t)(2 * m) | (u & 1u);
    if (out.node_origin) out.node_origin[m] = u >> 1;
    if (out.node_unitig) out.node_unitig[m] = contig;
    if (out.node_pos) out.node_pos[m] = (uint32_t)(m - p.off[outer.uni_off[contig]]);
}

__global__ __launch_bounds__(UT) void contig_kernel(Decomp outer, Decomp inner, const uint32_t *__restrict__ origin, const uint64_t *__restrict__ piece_off,
                                                    uint64_t *__restrict__ uni_off_out, uint8_t *__restrict__ circular_out) {
    for (uint64_t t = (uint64_t)blockIdx.x * UT + threadIdx.x; t <= outer.n_unitigs; t += (uint64_t)gridDim.x * UT) {
        const uint64_t a = outer.uni_off[t];
        if (uni_off_out) uni_off_out[t] = piece_off[a];
        if (!circular_out || t == outer.n_unitigs) continue;
        const bool alone = outer.uni_off[t + 1] - a == 1; // a single copy: circular when its origin is
        circular_out[t] = outer.circular[t] || (alone && inner.circular[origin[outer.members[a] >> 1]]);
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_graph_untangle(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                              const uint8_t *d_resolved, const uint32_t *d_partner, const uint64_t *d_uni_count, const uint32_t *d_edge_counts,
                              uint64_t *d_copy_off, uint32_t *d_origin, uint64_t *d_copy_count, uint64_t *d_keys, uint64_t *d_src_edge,
                              uint64_t capacity, uint64_t *n_copies, uint64_t *n_duplicated) {
    if (n_copies) *n_copies = 0;
    if (n_duplicated) *n_duplicated = 0;
    if (!ctx || !n_copies || !n_duplicated) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_untangle");
    if (n_unitigs >= (1ull << 31) || n_edges >= (1ull << 32))
        return c.invalid("2^31 unitigs or more (oriented ids are 32-bit), or 2^32 edges or more (a partner is a 32-bit edge index)");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_unitigs == 0) {
        if (n_edges) return c.invalid("edges without unitigs");
        if (d_copy_off) {
            c.zero(d_copy_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    if (!d_row_off || !d_resolved || (n_edges && (!d_dst || !d_partner))) return S2K_ERR_INVALID_ARG;
    const bool counts = d_copy_count && d_uni_count && d_edge_counts;
    const bool want = d_copy_off || d_origin || d_copy_count || d_keys || d_src_edge;
    const uint64_t n_ids = 2 * n_unitigs, bound = n_unitigs + n_edges / 2; // T' <= bound
    Layout L;
    const auto words = L.bytes<unsigned long long>(32); // the resolved unitigs; then the check's flag
    const auto nc_p = L.take<uint32_t>(n_unitigs);
    const auto coff_p = L.take<uint64_t>(n_unitigs + 1);
    const auto origin_p = L.take<uint32_t>(bound);
    const auto deg_p = L.take<uint32_t>(2 * bound);
    const auto row_p = L.take<uint64_t>(2 * bound + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(2 * bound));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *d_dup = words(w);
    uint32_t *bad = (uint32_t *)(d_dup + 1);
    uint32_t *ncopies = nc_p(w), *origin = origin_p(w), *degree = deg_p(w);
    uint64_t *copy_off = coff_p(w), *new_row = row_p(w);
    const Csr g{d_row_off, d_dst};
    const uint32_t hbad = c.check(d_dup, 32, bad, [&] {
        hipLaunchKernelGGL(untangle_check_kernel, dim3(grid_for(n_ids)), dim3(UT), 0, c.st, Unchecked{g, n_ids, n_edges, d_resolved, d_partner}, bad);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("not a CSR of 2 * n_unitigs rows that ends at n_edges, an id >= 2 * n_unitigs, a resolved byte above 1, a resolved unitig "
                         "without out(2 t) == out(2 t + 1) >= 2, a partner outside the row of the strand its edge enters, two in-edges with "
                         "one partner, or partner[tw(partner[a])] != tw(a)");
    hipLaunchKernelGGL(copies_kernel, dim3(grid_for(n_unitigs)), dim3(UT), 0, c.st, g, d_resolved, n_unitigs, ncopies, d_dup);
    c.launched();
    c.scan(ncopies, n_unitigs, copy_off, tmp_p(w));
    uint64_t total = 0;
    unsigned long long dup = 0;
    c.fetch(&total, copy_off + n_unitigs, 8);
    c.fetch(&dup, d_dup, 8);
    if (!c.sync()) return c.device_error();
    if (total > bound) return c.device_error("internal error (more copies than the edges allow)");
    if (total >= (1ull << 31)) return c.invalid("2^31 copies or more (oriented ids are 32-bit)");
    *n_copies = total;
    *n_duplicated = dup;
    if (!want) return S2K_OK;
    if (total > capacity) return S2K_ERR_CAPACITY;
    const Tangle k{g, d_resolved, d_partner, copy_off};
    const unsigned grid = grid_for(2 * total);
    hipLaunchKernelGGL(degree_kernel, dim3(grid), dim3(UT), 0, c.st, k, n_unitigs, 2 * total, origin, degree, d_uni_count, d_edge_counts,
                       counts ? d_copy_count : nullptr);
    c.launched();
    c.scan(degree, 2 * total, new_row, tmp_p(w));
    if (c.ok() && (d_keys || d_src_edge) && n_edges) {
        hipLaunchKernelGGL(untangle_write_kernel, dim3(grid), dim3(UT), 0, c.st, k, 2 * total, origin, new_row, d_keys, d_src_edge);
        c.launched();
    }
    if (d_copy_off) c.copy(d_copy_off, copy_off, (n_unitigs + 1) * 8, hipMemcpyDeviceToDevice);
    if (d_origin) c.copy(d_origin, origin, total * 4, hipMemcpyDeviceToDevice);
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_unitig_expand(s2k_ctx *ctx, const uint64_t *d_outer_off, const uint32_t *d_outer_members, const uint8_t *d_outer_circular,
                             uint64_t n_contigs, uint64_t n_copies, const uint32_t *d_origin, const uint64_t *d_uni_off, const uint32_t *d_members,
                             const uint8_t *d_circular, uint64_t n_unitigs, uint64_t n_nodes, uint64_t *d_uni_off_out, uint32_t *d_members_out,
                             uint32_t *d_node_unitig, uint32_t *d_node_pos, uint8_t *d_circular_out, uint32_t *d_node_origin, uint64_t capacity,
                             uint64_t *n_members) {
    if (n_members) *n_members = 0;
    if (!ctx || !n_members) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_unitig_expand");
    if (n_copies >= (1ull << 31) || n_nodes >= (1ull << 31) || n_contigs > n_copies || n_unitigs > n_nodes)
        return c.invalid("2^31 copies or nodes or more, more contigs than copies, or more unitigs than nodes");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_copies == 0) { // no copies: no contigs
        if (d_uni_off_out) {
            c.zero(d_uni_off_out, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    if (n_contigs == 0 || n_unitigs == 0) return c.invalid("copies without contigs or without unitigs");
    if (!d_outer_off || !d_outer_members || !d_outer_circular || !d_origin || !d_uni_off || !d_members || !d_circular) return S2K_ERR_INVALID_ARG;
    const bool want = d_uni_off_out || d_members_out || d_node_unitig || d_node_pos || d_circular_out || d_node_origin;
    Layout L;
    const auto flag = L.bytes<uint32_t>(16);
    const auto len_p = L.take<uint32_t>(n_copies);
    const auto contig_p = L.take<uint32_t>(n_copies);
    const auto off_p = L.take<uint64_t>(n_copies + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_copies));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint32_t *bad = flag(w);
    const Pieces p{len_p(w), contig_p(w), off_p(w)};
    const Decomp outer{d_outer_off, d_outer_members, d_outer_circular, n_contigs, n_copies};
    const Decomp inner{d_uni_off, d_members, d_circular, n_unitigs, n_nodes};
    uint64_t total = 0;
    const uint32_t hbad = c.check(bad, 16, bad, [&] {
        hipLaunchKernelGGL(expand_check_kernel, dim3(grid_for(std::max(n_copies, n_unitigs) + 1)), dim3(UT), 0, c.st, outer, inner, d_origin, p, bad);
        c.launched();
        c.scan(p.len, n_copies, p.off, tmp_p(w));
        c.fetch(&total, p.off + n_copies, 8);
    });
    if (!c.ok()) return c.device_error();
    if (hbad)
        return c.invalid("uni_off (inner or outer) that does not ascend strictly from 0 to its number of members, an outer member >= 2 * n_copies, "
                         "or an origin >= n_unitigs");
    if (total >= (1ull << 31)) return c.invalid("2^31 node instances or more (oriented ids are 32-bit)");
    *n_members = total;
    if (!want) return S2K_OK;
    if (total > capacity) return S2K_ERR_CAPACITY;
    if (d_members_out || d_node_unitig || d_node_pos || d_node_origin) {
        hipLaunchKernelGGL(expand_write_kernel, dim3((unsigned)((total + EX_T - 1) / EX_T)), dim3(EX_T), 0, c.st, outer, inner, d_origin, p, total,
                           Expanded{d_members_out, d_node_unitig, d_node_pos, d_node_origin});
        c.launched();
    }
    if (c.ok() && (d_uni_off_out || d_circular_out)) {
        hipLaunchKernelGGL(contig_kernel, dim3(grid_for(n_contigs + 1)), dim3(UT), 0, c.st, outer, inner, d_origin, p.off, d_uni_off_out, d_circular_out);
        c.launched();
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

// s2k_unitig.hip -- the unitigs of the minimizer-space graph: its non-branching paths compacted, and the graph between them
// (include/s2k.h: s2k_graph_unitigs, s2k_graph_unitig_edges).
//
// Input: the CSR of s2k_graph_adjacency over N = 2 * n_nodes oriented nodes; twin(u) = u ^ 1, twin((u, v)) = (v ^ 1, u ^ 1).
// Link: next(u) = v iff out(u) == 1, v its one destination, out(v ^ 1) == 1, v != u, v != u ^ 1.  With a twin-symmetric input
// next(u) = v <=> next(v ^ 1) = u ^ 1, so prev(u) = next(u ^ 1) ^ 1 and no reverse graph is needed.
//
// s2k_graph_unitigs, one lane per oriented node everywhere:
//  1. check_kernel: row_off[0] == 0, non-decreasing, row_off[N] == n_edges; every row strictly ascending with ids < N; for every
//     edge (u, v) a bounded binary search of row v ^ 1 for u ^ 1.  One flag word, read by the host before anything else runs.
//     Every read is clamped to the arrays whatever they hold.  A row of high degree is slow (one lane walks it), never wrong.
//  2. link_kernel: next[u] and the first ranking state; lanes u and u ^ 1 sit side by side in a wave, so prev comes from a
//     lane exchange.  n_links from one atomic per block on a workspace word.
//  3. jump_kernel: list ranking by pointer jumping towards the head.  State of u, one 8-byte word: ancestor : 32 | settled : 1 |
//     distance : 31 (a chain holds a node in one orientation only, so a distance is < n_nodes < 2^31).  A head starts as
//     (u, settled, 0), every other node as (prev(u), 1).  A round reads state[anc]: when that is settled (head, pos), u becomes
//     (head, settled, pos + distance); otherwise (anc's anc, distance + anc's distance).  Ping-pong buffers: an in-place jump
//     would race.  A settled lane copies its word and loads nothing else.  Every round counts the lanes it leaves unsettled
//     (one atomic per block); the host reads the counts after each of the first 8 rounds (a
//     round too many over 140 M slots costs 0.8 ms, a read 0.03 ms), then after 2, 2, 4, 4 ... rounds.  After round r the settled nodes of a
//     chain are those at positions < 2^(r+1), so the count falls strictly while a chain node is unsettled: 0 ends the ranking, and
//     two equal counts in a row mean that only cycles are left (no member of a cycle ever settles).
//  4. cycles (only when step 3 says so): cyc_init_kernel restarts the unsettled lanes as (prev(u), min(u >> 1, prev(u) >> 1));
//     cyc_min_kernel jumps with min() until a round changes no word -- then every lane holds the smallest node index of its
//     cycle (a cycle holds a node in one orientation only, so that is its smallest oriented id, and the index fits 31 bits);
//     cyc_cut_kernel makes that member a head, and step 3 runs again on what is now a chain.
//  5. head_kernel / len_kernel / scatter_kernel: strand u is kept iff head(u) < head(u ^ 1) (the head of the twin chain is the
//     twin of the tail; for a cycle, the twin cycle's smallest id).  Kept heads are numbered by launch_scan_u32 over the
//     oriented ids, their lengths (pos(h ^ 1) + 1; for a cycle pos(prev(h)) + 1) scanned into uni_off, and every kept node writes
//     itself to members[uni_off[t] + pos]: no sort, no atomics on an output.
//
// s2k_graph_unitig_edges, one lane per oriented unitig U = 2 t + s: its last member x (members[uni_off[t + 1] - 1], or
// members[uni_off[t]] ^ 1 for s = 1); every edge (x, v) of row x that is not a link goes to the oriented unitig V that starts
// with v.  uedge_count_kernel counts them, a scan gives the offsets, uedge_write_kernel writes a row's keys in ascending V by
// repeated selection (quadratic in the row's degree: rows are short; a row of high degree is slow, never wrong).
//
// Workspace (the context's grow-only count workspace): per oriented node 4 B next + 2 x 8 B ranking state (the idle one holds the
// numbering scan afterwards) + 4 B head flags, per node 8 B + 4 B for uni_off and the lengths: 60 B per node.  The edges call:
// 12 B per oriented unitig.
#include <algorithm>
#include <chrono>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

constexpr uint32_t SET = 0x80000000u; // the low word of a settled ranking state: SET | position
constexpr int MAX_ROUNDS = 32;        // a chain or a cut cycle has fewer than 2^31 members
constexpr int CNT_WORDS = MAX_ROUNDS + 8;

__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long pack(uint32_t hi, uint32_t lo) { return ((unsigned long long)hi << 32) | lo; }

// out-degree of u and, when it is 1, the link target (NONE: no link).  The CSR was checked.
__device__ __forceinline__ uint32_t link_of(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst, uint32_t u) {
    const uint64_t a = row_off[u];
    if (row_off[u + 1] - a != 1) return NONE;
    const uint32_t v = dst[a];
    if (v == u || v == (u ^ 1u)) return NONE;
    const uint32_t w = v ^ 1u;
    return row_off[w + 1] - row_off[w] == 1 ? v : NONE;
}

__global__ __launch_bounds__(UT) void check_kernel(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst, uint64_t n_ids,
                                                   uint64_t n_edges, uint32_t *__restrict__ bad) {
    bool ok = true;
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        uint64_t a, b;
        if (!csr_row_ok(row_off, u, n_ids, n_edges, &a, &b)) {
            ok = false;
            continue;
        }
        uint32_t last = 0;
        for (uint64_t e = a; e < b; e++) {
            const uint32_t v = dst[e];
            if (v >= n_ids || (e > a && v <= last)) {
                ok = false;
                break;
            }
            last = v;
            const uint32_t w = v ^ 1u, want = (uint32_t)u ^ 1u;
            uint64_t lo = row_off[w], hi = row_off[w + 1];
            if (lo > hi || hi > n_edges) {
                ok = false;
                break;
            }
            while (lo < hi) { // the first entry >= want; at most 64 steps whatever the row holds
                const uint64_t mid = lo + (hi - lo) / 2;
                if (dst[mid] < want) lo = mid + 1;
                else hi = mid;
            }
            if (lo >= row_off[w + 1] || row_off[w + 1] > n_edges || dst[lo] != want) {
                ok = false;
                break;
            }
        }
    }
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(UT) void link_kernel(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ dst, uint64_t n_ids,
                                                  uint32_t *__restrict__ next, unsigned long long *__restrict__ state,
                                                  unsigned long long *__restrict__ n_links) {
    unsigned long long links = 0;
    // n_ids is even and the stride a multiple of 64: lanes 2 j and 2 j + 1 of a wave hold u and u ^ 1, both in range or neither
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        const uint32_t nx = link_of(row_off, dst, (uint32_t)u);
        const uint32_t tw = __shfl_xor(nx, 1, 64); // next(u ^ 1)
        next[u] = nx;
        links += nx != NONE;
        state[u] = tw == NONE ? pack((uint32_t)u, SET) : pack(tw ^ 1u, 1u);
    }
    block_add(links, n_links);
}

__global__ __launch_bounds__(UT) void jump_kernel(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ out, uint64_t n_ids,
                                                  unsigned long long *__restrict__ unsettled) {
    unsigned long long open = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        unsigned long long s = src[u];
        const uint32_t lo = (uint32_t)s;
        if (!(lo & SET)) {
            const unsigned long long t = src[s >> 32];
            const uint32_t tlo = (uint32_t)t;
            if (tlo & SET) {
                s = pack((uint32_t)(t >> 32), tlo + lo); // SET | (pos(anc) + distance)
            } else {
                const uint64_t d = (uint64_t)lo + tlo; // (a cycle's distances saturate)
                s = pack((uint32_t)(t >> 32), d < SET ? (uint32_t)d : SET - 1u);
                open++;
            }
        }
        out[u] = s;
    }
    block_add(open, unsettled);
}

__global__ __launch_bounds__(UT) void cyc_init_kernel(unsigned long long *__restrict__ state, const uint32_t *__restrict__ next, uint64_t n_ids) {
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        if ((uint32_t)state[u] & SET) continue;
        const uint32_t p = next[u ^ 1] ^ 1u; // a member of a cycle has a prev
        state[u] = pack(p, umin32((uint32_t)u >> 1, p >> 1));
    }
}

__global__ __launch_bounds__(UT) void cyc_min_kernel(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ out, uint64_t n_ids,
                                                     unsigned long long *__restrict__ changed) {
    unsigned long long moved = 0;
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        unsigned long long s = src[u];
        const uint32_t lo = (uint32_t)s;
        if (!(lo & SET)) {
            const unsigned long long t = src[s >> 32];
            const uint32_t m = umin32(lo, (uint32_t)t);
            moved += m != lo;
            s = pack((uint32_t)(t >> 32), m);
        }
        out[u] = s;
    }
    block_add(moved, changed);
}

__global__ __launch_bounds__(UT) void cyc_cut_kernel(unsigned long long *__restrict__ state, const uint32_t *__restrict__ next, uint64_t n_ids) {
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        const uint32_t lo = (uint32_t)state[u];
        if (lo & SET) continue;
        state[u] = ((uint32_t)u >> 1) == lo ? pack((uint32_t)u, SET) : pack(next[u ^ 1] ^ 1u, 1u);
    }
}

// u is the head of a kept strand: -> its number of members, else 0
__device__ __forceinline__ uint32_t kept_head_len(const unsigned long long *__restrict__ rank, const uint32_t *__restrict__ next, uint32_t u) {
    const unsigned long long s = rank[u];
    if ((uint32_t)(s >> 32) != u) return 0;
    const unsigned long long t = rank[u ^ 1u];
    if (u >= (uint32_t)(t >> 32)) return 0;
    const uint32_t pv = next[u ^ 1u]; // a head with a prev: the cut of a cycle
    return (pv == NONE ? ((uint32_t)t & ~SET) : ((uint32_t)rank[pv ^ 1u] & ~SET)) + 1u;
}

__global__ __launch_bounds__(UT) void head_kernel(const unsigned long long *__restrict__ rank, const uint32_t *__restrict__ next, uint64_t n_ids,
                                                  uint32_t *__restrict__ flag) {
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT)
        flag[u] = kept_head_len(rank, next, (uint32_t)u) != 0;
}

__global__ __launch_bounds__(UT) void len_kernel(const unsigned long long *__restrict__ rank, const uint32_t *__restrict__ next, uint64_t n_ids,
                                                 const uint32_t *__restrict__ flag, const uint64_t *__restrict__ number, uint32_t *__restrict__ len) {
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT)
        if (flag[u]) len[number[u]] = kept_head_len(rank, next, (uint32_t)u);
}

__global__ __launch_bounds__(UT) void scatter_kernel(const unsigned long long *__restrict__ rank, const uint32_t *__restrict__ next, uint64_t n_ids,
                                                     const uint64_t *__restrict__ number, const uint64_t *__restrict__ uni_off,
                                                     uint32_t *__restrict__ members, uint32_t *__restrict__ node_unitig, uint32_t *__restrict__ node_pos,
                                                     uint8_t *__restrict__ circular) {
    for (uint64_t u = (uint64_t)blockIdx.x * UT + threadIdx.x; u < n_ids; u += (uint64_t)gridDim.x * UT) {
        const unsigned long long s = rank[u];
        const uint32_t h = (uint32_t)(s >> 32);
        if (h >= (uint32_t)(rank[u ^ 1] >> 32)) continue; // the other strand is the kept one
        const uint32_t pos = (uint32_t)s & ~SET;
        const uint64_t t = number[h];
        if (members) members[uni_off[t] + pos] = (uint32_t)u;
        if (node_unitig) node_unitig[u >> 1] = (uint32_t)t;
        if (node_pos) node_pos[u >> 1] = pos;
        if (circular && pos == 0) circular[t] = next[u ^ 1] != NONE;
    }
}

// ---- unitig edges ---------------------------------------------------------------------------------------------------------------
struct UnitigView {
    const uint64_t *row_off;
    const uint32_t *dst;
    const uint64_t *uni_off;
    const uint32_t *members, *node_unitig, *node_pos;
};

__device__ __forceinline__ uint32_t last_member(const UnitigView &g, uint64_t U) {
    const uint64_t t = U >> 1;
    return (U & 1) ? g.members[g.uni_off[t]] ^ 1u : g.members[g.uni_off[t + 1] - 1];
}
// the oriented unitig that starts with v (v enters a head: the first member of a kept strand, or the twin of its last)
__device__ __forceinline__ uint64_t unitig_from(const UnitigView &g, uint32_t v) {
    const uint64_t t = g.node_unitig[v >> 1];
    return 2 * t + (g.members[g.uni_off[t] + g.node_pos[v >> 1]] != v);
}

__global__ __launch_bounds__(UT) void uedge_count_kernel(UnitigView g, uint64_t n_orient, uint32_t *__restrict__ cnt) {
    for (uint64_t U = (uint64_t)blockIdx.x * UT + threadIdx.x; U < n_orient; U += (uint64_t)gridDim.x * UT) {
        const uint32_t x = last_member(g, U);
        const uint64_t deg = g.row_off[x + 1] - g.row_off[x];
        cnt[U] = (uint32_t)(deg - (deg == 1 && link_of(g.row_off, g.dst, x) != NONE));
    }
}

__global__ __launch_bounds__(UT) void uedge_write_kernel(UnitigView g, uint64_t n_orient, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off,
                                                         uint64_t *__restrict__ keys, uint64_t *__restrict__ src_edge) {
    for (uint64_t U = (uint64_t)blockIdx.x * UT + threadIdx.x; U < n_orient; U += (uint64_t)gridDim.x * UT) {
        const uint32_t c = cnt[U];
        if (!c) continue;
        const uint64_t a = g.row_off[last_member(g, U)], o = off[U];
        uint64_t floor_v = 0; // keys of the row in ascending V: the smallest V not yet written (they are distinct: one head each)
        for (uint32_t k = 0; k < c; k++) {
            uint64_t best = ~0ull, best_e = 0;
            for (uint64_t e = a; e < a + c; e++) {
                const uint64_t V = unitig_from(g, g.dst[e]);
                if (V >= floor_v && V < best) best = V, best_e = e;
            }
            keys[o + k] = U << 32 | best;
            if (src_edge) src_edge[o + k] = best_e;
            floor_v = best + 1;
        }
    }
}

// Runs the ranking rounds on the ping-pong pair until no lane is unsettled (-> 0) or only cycles are left (-> 1); *cur names the
// buffer that holds the result.  -1: a HIP error or more rounds than a valid input can need.
int rank_rounds(Call &c, unsigned long long *buf[2], int *cur, uint64_t n_ids, unsigned long long *cnt, uint32_t *rounds) {
    unsigned long long h[CNT_WORDS];
    c.zero(cnt, sizeof(h));
    if (!c.ok()) return -1;
    int r = 0;
    for (int group = 1; r < MAX_ROUNDS; group = r < 8 ? 1 : r < 12 ? 2 : 4) {
        const int first = r;
        for (int i = 0; i < group && r < MAX_ROUNDS; i++, r++) {
            hipLaunchKernelGGL(jump_kernel, dim3(grid_for(n_ids)), dim3(UT), 0, c.st, buf[*cur], buf[*cur ^ 1], n_ids, cnt + r);
            *cur ^= 1;
        }
        c.launched();
        c.fetch(h, cnt, sizeof(h));
        if (!c.sync()) return -1;
        *rounds += (uint32_t)(r - first);
        for (int i = first; i < r; i++) {
            if (h[i] == 0) return 0;
            if (i > 0 && h[i] == h[i - 1]) return 1;
        }
    }
    return -1;
}

} // namespace
} // namespace s2k

using namespace s2k;

namespace {
// what s2k_graph_unitigs_last_steps reports: host clock between the host waits that end the steps of the last call
double g_step_ms[4] = {0, 0, 0, 0};
uint32_t g_rounds = 0;
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} // namespace

extern "C" {

s2k_status s2k_graph_unitigs(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes,
                             const s2k_unitig_out *out, uint64_t *n_unitigs, uint64_t *n_links) {
    if (n_unitigs) *n_unitigs = 0;
    if (n_links) *n_links = 0;
    if (!ctx || !d_row_off || !n_unitigs || !n_links || (n_edges && !d_dst)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_unitigs");
    if (n_nodes >= (1ull << 31) || n_edges >= (1ull << 40))
        return c.invalid("2^31 nodes or more (oriented node ids are 32-bit), or 2^40 edges or more");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const uint64_t n_ids = 2 * n_nodes;
    const bool want = out && (out->uni_off || out->members || out->node_unitig || out->node_pos || out->circular);
    g_rounds = 0;
    g_step_ms[0] = g_step_ms[1] = g_step_ms[2] = g_step_ms[3] = 0;
    double t0 = now_ms(), t1;
#define STEP(i) (t1 = now_ms(), g_step_ms[i] = t1 - t0, t0 = t1)
    if (n_nodes == 0) {
        uint64_t first = 1;
        c.fetch(&first, d_row_off, 8);
        if (!c.sync()) return c.device_error();
        if (first != 0 || n_edges != 0) return c.invalid("row_off must start at 0 and end at n_edges");
        if (want && out->uni_off) {
            c.zero(out->uni_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    Layout L;
    const auto counters = L.bytes<unsigned long long>(CNT_WORDS * 8 + 16);
    const auto next_p = L.take<uint32_t>(n_ids);
    const auto buf_a = L.take<unsigned long long>(n_ids + 1), buf_b = L.take<unsigned long long>(n_ids + 1);
    const auto flag_p = L.take<uint32_t>(n_ids);
    const auto uoff_p = L.take<uint64_t>(n_nodes + 1);
    const auto len_p = L.take<uint32_t>(n_nodes);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_ids));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    unsigned long long *cnt = counters(w); // CNT_WORDS round counters, then n_links, then the check's flag
    unsigned long long *d_links = cnt + CNT_WORDS;
    uint32_t *bad = (uint32_t *)(cnt + CNT_WORDS + 1);
    uint32_t *next = next_p(w), *flag = flag_p(w), *len = len_p(w);
    unsigned long long *buf[2] = {buf_a(w), buf_b(w)};
    uint64_t *uoff = uoff_p(w), *scan_tmp = tmp_p(w);
    const unsigned grid = grid_for(n_ids);

    // 1. the input
    const uint32_t hbad = c.check(cnt, CNT_WORDS * 8 + 16, bad, [&] {
        hipLaunchKernelGGL(check_kernel, dim3(grid), dim3(UT), 0, c.st, d_row_off, d_dst, n_ids, n_edges, bad);
    });
    if (!c.ok()) return c.device_error();
    STEP(0);
    if (hbad)
        return c.invalid("not a CSR of 2 * n_nodes rows that ends at n_edges, a row that is not strictly ascending or names an id >= 2 * n_nodes, "
                         "or an edge whose twin is missing");
    // 2. links, 3. ranking
    hipLaunchKernelGGL(link_kernel, dim3(grid), dim3(UT), 0, c.st, d_row_off, d_dst, n_ids, next, buf[0], d_links);
    c.launched();
    if (!c.ok()) return c.device_error();
    int cur = 0;
    uint32_t rounds = 0;
    int left = rank_rounds(c, buf, &cur, n_ids, cnt, &rounds);
    if (left == 1) { // 4. cycles: cut each at its smallest member, rank again
        hipLaunchKernelGGL(cyc_init_kernel, dim3(grid), dim3(UT), 0, c.st, buf[cur], next, n_ids);
        c.zero(cnt, CNT_WORDS * 8);
        bool still = true;
        for (int r = 0; still && c.ok() && r < MAX_ROUNDS;) {
            unsigned long long h[4];
            const int first = r;
            for (int i = 0; i < 4 && r < MAX_ROUNDS; i++, r++) {
                hipLaunchKernelGGL(cyc_min_kernel, dim3(grid), dim3(UT), 0, c.st, buf[cur], buf[cur ^ 1], n_ids, cnt + r);
                cur ^= 1;
            }
            c.launched();
            c.fetch(h, cnt + first, (size_t)(r - first) * 8);
            c.sync();
            rounds += (uint32_t)(r - first);
            for (int i = 0; c.ok() && i < r - first; i++) still = still && h[i] != 0;
        }
        if (!c.ok() || still) return c.device_error();
        hipLaunchKernelGGL(cyc_cut_kernel, dim3(grid), dim3(UT), 0, c.st, buf[cur], next, n_ids);
        c.launched();
        if (!c.ok()) return c.device_error();
        left = rank_rounds(c, buf, &cur, n_ids, cnt, &rounds);
    }
    if (left != 0) return c.device_error("the list ranking did not end");
    g_rounds = rounds;
    STEP(1);
    // 5. numbering
    const unsigned long long *rank = buf[cur];
    uint64_t *number = (uint64_t *)buf[cur ^ 1];
    hipLaunchKernelGGL(head_kernel, dim3(grid), dim3(UT), 0, c.st, rank, next, n_ids, flag);
    c.launched();
    c.scan(flag, n_ids, number, scan_tmp);
    uint64_t total = 0, links = 0;
    c.fetch(&total, number + n_ids, 8);
    c.fetch(&links, d_links, 8);
    if (!c.sync()) return c.device_error();
    STEP(2);
    if (total > n_nodes) return c.device_error("internal error (more unitigs than nodes)"); // every unitig holds a node
    *n_unitigs = total;
    *n_links = links;
    if (!want) return S2K_OK;
    if (total > out->capacity) return S2K_ERR_CAPACITY;
    hipLaunchKernelGGL(len_kernel, dim3(grid), dim3(UT), 0, c.st, rank, next, n_ids, flag, number, len);
    c.launched();
    c.scan(len, total, uoff, scan_tmp);
    if (c.ok()) {
        hipLaunchKernelGGL(scatter_kernel, dim3(grid), dim3(UT), 0, c.st, rank, next, n_ids, number, uoff, out->members, out->node_unitig,
                           out->node_pos, out->circular);
        c.launched();
    }
    if (out->uni_off) c.copy(out->uni_off, uoff, (total + 1) * 8, hipMemcpyDeviceToDevice);
    if (!c.sync()) return c.device_error();
    STEP(3);
    return S2K_OK;
#undef STEP
}

void s2k_graph_unitigs_last_steps(double *ms, uint32_t *rounds) {
    for (int i = 0; ms && i < 4; i++) ms[i] = g_step_ms[i];
    if (rounds) *rounds = g_rounds;
}

s2k_status s2k_graph_unitig_edges(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes,
                                  const uint64_t *d_uni_off, const uint32_t *d_members, const uint32_t *d_node_unitig, const uint32_t *d_node_pos,
                                  uint64_t n_unitigs, uint64_t *d_keys, uint64_t *d_src_edge, uint64_t capacity, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!ctx || !n_out || !d_row_off || !d_uni_off || (n_edges && !d_dst)) return S2K_ERR_INVALID_ARG;
    if (n_unitigs && (!d_members || !d_node_unitig || !d_node_pos)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_unitig_edges");
    if (n_nodes >= (1ull << 31) || n_unitigs > n_nodes) return c.invalid("2^31 nodes or more, or more unitigs than nodes");
    if (n_unitigs == 0 || n_edges == 0) return S2K_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const uint64_t n_orient = 2 * n_unitigs;
    Layout L;
    const auto cnt_p = L.take<uint32_t>(n_orient);
    const auto off_p = L.take<uint64_t>(n_orient + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(n_orient));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint32_t *cnt = cnt_p(w);
    uint64_t *eoff = off_p(w);
    const UnitigView g{d_row_off, d_dst, d_uni_off, d_members, d_node_unitig, d_node_pos};
    const unsigned grid = grid_for(n_orient);
    hipLaunchKernelGGL(uedge_count_kernel, dim3(grid), dim3(UT), 0, c.st, g, n_orient, cnt);
    c.launched();
    c.scan(cnt, n_orient, eoff, tmp_p(w));
    uint64_t total = 0;
    c.fetch(&total, eoff + n_orient, 8);
    if (!c.sync()) return c.device_error();
    *n_out = total;
    if (!d_keys || total == 0) return S2K_OK;
    if (total > capacity) return S2K_ERR_CAPACITY;
    hipLaunchKernelGGL(uedge_write_kernel, dim3(grid), dim3(UT), 0, c.st, g, n_orient, cnt, eoff, d_keys, d_src_edge);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

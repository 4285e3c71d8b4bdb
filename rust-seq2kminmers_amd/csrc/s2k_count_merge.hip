// s2k_count_merge.hip -- s2k_count_merge_device: the union of two count tables that are strictly ascending by key, the counts of a
// key present in both added (saturated at 2^32-1), the pairs under min_count dropped; and the accumulating counter s2k_counter_*
// built on it and on s2k_count_device_ex (include/s2k.h).
//
// Merge path, two passes over fixed output tiles of MG_TILE items of the merged sequence (A and B items, duplicates included):
//  1. merge_split_kernel: the A/B split of every tile boundary by a binary search along its diagonal (ties: A before B).
//  2. merge_tile_kernel<false>: each workgroup stages its A and B slices (keys, and counts when the cutoff needs them) in LDS, each
//     lane finds its own 15 items by a second diagonal search in LDS and merges them serially, counting what survives; the
//     strictly-ascending check of every staged key runs in the same pass.  Per tile: kept pairs; per call: distinct keys, bad flag.
//  3. launch_scan_u32 over the per-tile kept counts: each tile's first output slot.
//  4. merge_tile_kernel<true>: the same merge again; the kept pairs go to LDS at their block-scanned offsets and leave the
//     workgroup as one contiguous, coalesced run.
// Duplicates: both inputs are strictly ascending and ties put A first, so a key in both tables is the adjacent pair A[i], B[j].  A
// B item is dropped when A[i-1] (the last A item before it) equals it; an A item adds B[j]'s count (the next B item) when equal.
// Each tile stages A[a0-1] in front of its A slice and B[b1] behind its B slice, so a pair that straddles a tile boundary reads its
// neighbour like any other.  No sentinel key: 2^64-1 is a key like the others and every read is bounded by index.
#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

constexpr int MG_THREADS = 256;
// merged items per lane: odd, so that the lanes' serial merges start 15 x 8 B = 30 dwords apart and a ds_read_b64 of 32 lanes covers
// the 64 banks once (16 items: 32 dwords apart, every fourth lane on the same banks, a 16-way conflict per read)
constexpr int MG_IPT = 15;
constexpr uint32_t MG_TILE = MG_THREADS * MG_IPT;  // 3 840 items per workgroup: 45 KiB of LDS -> 3 workgroups per CU
constexpr uint32_t SAT = 0xFFFFFFFFu;

struct MergeMeta {
    unsigned long long n_distinct;
    uint32_t bad; // an input that is not strictly ascending
    uint32_t pad;
};

__device__ inline uint32_t sat_add(uint32_t a, uint32_t b) {
    const uint64_t s = (uint64_t)a + b;
    return s > SAT ? SAT : (uint32_t)s;
}

// split[t] = A items among the first min(t * MG_TILE, na + nb) items of the merge (ties: A first), t = 0 .. n_tiles
__global__ __launch_bounds__(256) void merge_split_kernel(const uint64_t *__restrict__ ak, uint64_t na, const uint64_t *__restrict__ bk, uint64_t nb,
                                                          uint64_t n_tiles, uint64_t *__restrict__ split) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    const uint64_t d = std::min<uint64_t>(t * MG_TILE, na + nb);
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na; // lo <= mid < hi: a[mid] and b[d - 1 - mid] are in range
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ak[mid] <= bk[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    split[t] = lo;
}

// One workgroup per tile (see the header comment).  LDS: sk[0] = A[a0-1], sk[1 .. 1+nA) = the A slice, sk[1+nA .. 1+nA+nB) = the
// B slice, sk[1+nA+nB] = B[b1]; sc holds the counts at the same places.  WRITE = false: count pass; true: write pass.
template <bool WRITE>
__global__ __launch_bounds__(MG_THREADS) void merge_tile_kernel(const uint64_t *__restrict__ ak, const uint32_t *__restrict__ ac, uint64_t na,
                                                                const uint64_t *__restrict__ bk, const uint32_t *__restrict__ bc, uint64_t nb,
                                                                const uint64_t *__restrict__ split, uint32_t minc, uint32_t *__restrict__ tile_kept,
                                                                const uint64_t *__restrict__ tile_off, MergeMeta *meta, uint64_t *__restrict__ o_keys,
                                                                uint32_t *__restrict__ o_counts, uint64_t capacity) {
    __shared__ uint64_t sk[MG_TILE + 2];
    __shared__ uint32_t sc[MG_TILE + 2];
    __shared__ uint32_t wsum[MG_THREADS / 64];
    __shared__ uint32_t sbad;
    const uint64_t t = blockIdx.x, n = na + nb;
    const uint64_t d0 = t * MG_TILE, d1 = std::min<uint64_t>(d0 + MG_TILE, n);
    const uint64_t a0 = split[t], a1 = split[t + 1];
    if (a1 < a0 || d1 - a1 < d0 - a0) { // only an input that is not ascending moves the path backwards
        if (!WRITE && threadIdx.x == 0) {
            tile_kept[t] = 0;
            atomicOr(&meta->bad, 1u);
        }
        return;
    }
    const uint64_t b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t nA = (uint32_t)(a1 - a0), nB = (uint32_t)(b1 - b0), nT = nA + nB; // nT <= MG_TILE
    const bool need_c = WRITE || minc > 1;
    const bool has_prev = a0 > 0, has_next = b1 < nb;
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < MG_IPT; r++) { // every load of the lane in flight at once
        const uint32_t i = r * MG_THREADS + tid;
        if (i < nA) {
            sk[1 + i] = ak[a0 + i];
            if (need_c) sc[1 + i] = ac[a0 + i];
        } else if (i < nT) {
            sk[1 + i] = bk[b0 + (i - nA)];
            if (need_c) sc[1 + i] = bc[b0 + (i - nA)];
        }
    }
    if (tid == 0) {
        sbad = 0;
        sk[0] = has_prev ? ak[a0 - 1] : 0;
        sk[1 + nT] = has_next ? bk[b1] : 0;
        sc[1 + nT] = has_next && need_c ? bc[b1] : 0;
    }
    __syncthreads();
    if (!WRITE) { // every A key against the one before it, every B key against the one after it: together, every adjacent pair of each input
        bool bad = false;
#pragma unroll
        for (int r = 0; r < MG_IPT; r++) {
            const uint32_t i = r * MG_THREADS + tid, p = 1 + i;
            if (i < nA) bad |= (i > 0 || has_prev) && !(sk[p - 1] < sk[p]);
            else if (i < nT) bad |= (i + 1 < nT || has_next) && !(sk[p] < sk[p + 1]);
        }
        if (bad) sbad = 1;
    }

    // this lane's items: diagonal search inside the tile
    const uint64_t *A = sk + 1, *B = sk + 1 + nA;
    const uint32_t diag = std::min<uint32_t>((uint32_t)tid * MG_IPT, nT);
    uint32_t lo = diag > nB ? diag - nB : 0, hi = std::min(diag, nA);
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[diag - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    uint32_t ia = lo, ib = diag - lo;
    uint64_t key[MG_IPT];
    uint32_t cnt[MG_IPT];
    uint32_t keep = 0, n_keep = 0, n_dist = 0;
#pragma unroll
    for (int r = 0; r < MG_IPT; r++) {
        key[r] = 0;
        cnt[r] = 0;
        if (diag + r >= nT) continue;
        const bool takeA = ia < nA && (ib >= nB || A[ia] <= B[ib]);
        bool dup = false;
        if (takeA) {
            const uint64_t k = A[ia];
            uint32_t c = need_c ? sc[1 + ia] : 0u;
            if ((ib < nB || has_next) && B[ib] == k && need_c) c = sat_add(c, sc[1 + nA + ib]); // B[nB] is the staged B[b1]
            key[r] = k;
            cnt[r] = c;
            ia++;
        } else {
            const uint64_t k = B[ib];
            dup = (ia > 0 || has_prev) && sk[ia] == k; // sk[ia] = A[ia - 1]; sk[0] the staged A[a0-1]
            key[r] = k;
            cnt[r] = need_c ? sc[1 + nA + ib] : 0u;
            ib++;
        }
        const bool kept = !dup && (!need_c || cnt[r] >= minc);
        n_dist += dup ? 0u : 1u;
        n_keep += kept ? 1u : 0u;
        keep |= kept ? 1u << r : 0u;
    }

    uint32_t tot;
    const uint32_t pos = block_excl_scan<MG_THREADS / 64>(n_keep, wsum, &tot); // (its barriers also end every lane's reads of the staged slices)
    if (!WRITE) {
        uint32_t dist_tot;
        (void)block_excl_scan<MG_THREADS / 64>(n_dist, wsum, &dist_tot);
        if (tid == 0) {
            tile_kept[t] = tot;
            if (dist_tot) atomicAdd(&meta->n_distinct, (unsigned long long)dist_tot);
            if (sbad) atomicOr(&meta->bad, 1u);
        }
        return;
    }
    uint32_t q = pos;
#pragma unroll
    for (int r = 0; r < MG_IPT; r++)
        if (keep & (1u << r)) {
            sk[q] = key[r];
            sc[q] = cnt[r];
            q++;
        }
    __syncthreads();
    const uint64_t base = tile_off[t];
    for (uint32_t i = tid; i < tot; i += MG_THREADS) {
        if (base + i >= capacity) break; // the host checked n_kept <= capacity; never write past it
        if (o_keys) o_keys[base + i] = sk[i];
        if (o_counts) o_counts[base + i] = sc[i];
    }
}

struct Tab {
    const uint64_t *keys;
    const uint32_t *counts;
    uint64_t n;
};

// what the count pass leaves for the write pass (the context's count workspace must not be used in between)
struct MergeWs {
    uint64_t n_tiles = 0;
    uint64_t *split = nullptr, *tile_off = nullptr;
    uint32_t *tile_kept = nullptr;
    MergeMeta *meta = nullptr;
};

// count pass: sizes of the merge of a and b under cutoff minc (>= 1); S2K_ERR_INVALID_ARG when an input is not strictly ascending
s2k_status merge_count(s2k_ctx *ctx, const Tab &a, const Tab &b, uint32_t minc, MergeWs *ws, uint64_t *n_distinct, uint64_t *n_kept) {
    *n_distinct = *n_kept = 0;
    const uint64_t n = a.n + b.n;
    ws->n_tiles = 0;
    if (n == 0) return S2K_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Call c(ctx, "s2k_count_merge_device");
    const uint64_t nt = (n + MG_TILE - 1) / MG_TILE;
    if (nt * MG_THREADS >= (1ull << 32)) return c.invalid("more than 2^36 items"); // the grid's thread count must fit 32 bits: 2^36 items
    Layout L;
    const auto split = L.take<uint64_t>(nt + 1), tile_off = L.take<uint64_t>(nt + 1);
    const auto tile_kept = L.take<uint32_t>(nt);
    const auto scan_tmp = L.bytes<uint64_t>(scan_tmp_bytes(nt));
    const auto meta = L.take<MergeMeta>(1);
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    ws->n_tiles = nt;
    ws->split = split(w);
    ws->tile_off = tile_off(w);
    ws->tile_kept = tile_kept(w);
    ws->meta = meta(w);
    c.zero(ws->meta, sizeof(MergeMeta));
    hipLaunchKernelGGL(merge_split_kernel, dim3((unsigned)((nt + 1 + 255) / 256)), dim3(256), 0, c.st, a.keys, a.n, b.keys, b.n, nt, ws->split);
    hipLaunchKernelGGL(merge_tile_kernel<false>, dim3((unsigned)nt), dim3(MG_THREADS), 0, c.st, a.keys, a.counts, a.n, b.keys, b.counts, b.n,
                       ws->split, minc, ws->tile_kept, (const uint64_t *)nullptr, ws->meta, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint64_t)0);
    c.launched();
    c.scan(ws->tile_kept, nt, ws->tile_off, scan_tmp(w));
    MergeMeta hm{};
    uint64_t kept = 0;
    c.fetch(&hm, ws->meta, sizeof hm);
    c.fetch(&kept, ws->tile_off + nt, 8);
    if (!c.sync()) return c.device_error();
    if (hm.bad) return c.invalid("an input table is not strictly ascending by key");
    *n_distinct = hm.n_distinct;
    *n_kept = kept;
    return S2K_OK;
}

// write pass after merge_count with the same arguments: the n_kept pairs to o_keys / o_counts (either may be NULL)
s2k_status merge_write(s2k_ctx *ctx, const Tab &a, const Tab &b, uint32_t minc, const MergeWs &ws, uint64_t *o_keys, uint32_t *o_counts,
                       uint64_t n_kept) {
    if (ws.n_tiles == 0 || n_kept == 0 || (!o_keys && !o_counts)) return S2K_OK;
    Call c(ctx, "s2k_count_merge_device");
    hipLaunchKernelGGL(merge_tile_kernel<true>, dim3((unsigned)ws.n_tiles), dim3(MG_THREADS), 0, c.st, a.keys, a.counts, a.n, b.keys, b.counts,
                       b.n, ws.split, minc, ws.tile_kept, ws.tile_off, ws.meta, o_keys, o_counts, n_kept);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

bool overlaps(const void *p, size_t pb, const void *q, size_t qb) {
    if (!p || !q || !pb || !qb) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

} // namespace
} // namespace s2k

using namespace s2k;

// Runs of the counter: (keys, counts) tables, strictly ascending, in one device allocation each (keys, then counts).
struct s2k_counter {
    struct Run {
        uint64_t *keys;
        uint32_t *counts;
        uint64_t n;
    };
    s2k_ctx *ctx;
    std::vector<Run> runs; // the stack, oldest (largest) first
    void *scratch = nullptr;  // the pairs of the batch being added
    size_t scratch_bytes = 0;
};

namespace s2k {
s2k_ctx *counter_ctx(s2k_counter *c) { return c->ctx; }
} // namespace s2k

namespace {

bool run_alloc(uint64_t n, s2k_counter::Run *r) {
    void *p = nullptr;
    if (hipMalloc(&p, al(n * 8) + n * 4) != hipSuccess) return false;
    r->keys = (uint64_t *)p;
    r->counts = (uint32_t *)((char *)p + al(n * 8));
    r->n = n;
    return true;
}

void run_free(s2k_counter::Run &r) {
    if (r.keys) (void)hipFree(r.keys);
    r.keys = nullptr;
    r.counts = nullptr;
    r.n = 0;
}

// a (older) and b (newer) -> a new exact-size run with every pair (cutoff 1)
s2k_status merge_runs(s2k_counter *c, const s2k_counter::Run &a, const s2k_counter::Run &b, s2k_counter::Run *out) {
    const Tab ta{a.keys, a.counts, a.n}, tb{b.keys, b.counts, b.n};
    MergeWs ws;
    uint64_t nd = 0, nk = 0;
    s2k_status s = merge_count(c->ctx, ta, tb, 1, &ws, &nd, &nk);
    if (s != S2K_OK) return s;
    if (!run_alloc(nk, out)) {
        ctx_set_error(c->ctx, "s2k_counter: run allocation");
        return S2K_ERR_NOMEM;
    }
    s = merge_write(c->ctx, ta, tb, 1, ws, out->keys, out->counts, nk);
    if (s != S2K_OK) run_free(*out);
    return s;
}

// one piece (n < 2^32) of an add: counted into the scratch, then merged down the stack while it is at least half the run below
s2k_status counter_add_piece(s2k_counter *c, const uint64_t *d_hash, uint64_t n) {
    const size_t need = al(n * 8) + n * 4;
    if (need > c->scratch_bytes) {
        if (c->scratch) (void)hipFree(c->scratch);
        c->scratch = nullptr;
        c->scratch_bytes = 0;
        if (hipMalloc(&c->scratch, need) != hipSuccess) {
            ctx_set_error(c->ctx, "s2k_counter_add: scratch allocation");
            return S2K_ERR_NOMEM;
        }
        c->scratch_bytes = need;
    }
    s2k_counter::Run cur{(uint64_t *)c->scratch, (uint32_t *)((char *)c->scratch + al(n * 8)), 0};
    uint64_t nd = 0;
    s2k_status s = s2k_count_device_ex(c->ctx, d_hash, n, 1, S2K_COUNT_SORTED, cur.keys, cur.counts, n, &nd, &cur.n);
    if (s != S2K_OK || cur.n == 0) return s;
    bool owned = false; // cur lives in the scratch until its first merge
    while (!c->runs.empty() && 2 * cur.n >= c->runs.back().n) {
        s2k_counter::Run m{};
        s = merge_runs(c, c->runs.back(), cur, &m);
        if (s != S2K_OK) {
            if (owned) c->runs.push_back(cur); // keep what was merged so far (the stack is only unbalanced)
            return s;
        }
        run_free(c->runs.back());
        c->runs.pop_back();
        if (owned) run_free(cur);
        cur = m;
        owned = true;
    }
    if (!owned) { // pushed as it is: an exact-size copy of the scratch
        s2k_counter::Run r{};
        if (!run_alloc(cur.n, &r)) {
            ctx_set_error(c->ctx, "s2k_counter_add: run allocation");
            return S2K_ERR_NOMEM;
        }
        Call call(c->ctx, "s2k_counter_add");
        call.copy(r.keys, cur.keys, cur.n * 8, hipMemcpyDeviceToDevice);
        call.copy(r.counts, cur.counts, cur.n * 4, hipMemcpyDeviceToDevice);
        if (!call.sync()) {
            run_free(r);
            return call.device_error();
        }
        cur = r;
    }
    c->runs.push_back(cur);
    return S2K_OK;
}

} // namespace

extern "C" {

s2k_status s2k_count_merge_device(s2k_ctx *ctx, const uint64_t *d_a_keys, const uint32_t *d_a_counts, uint64_t n_a, const uint64_t *d_b_keys,
                                  const uint32_t *d_b_counts, uint64_t n_b, uint32_t min_count, uint64_t *d_keys, uint32_t *d_counts,
                                  uint64_t capacity, uint64_t *n_distinct, uint64_t *n_kept) {
    if (!ctx || !n_distinct || !n_kept || (n_a && (!d_a_keys || !d_a_counts)) || (n_b && (!d_b_keys || !d_b_counts)) || n_a + n_b < n_a)
        return S2K_ERR_INVALID_ARG;
    *n_distinct = *n_kept = 0;
    const bool want = d_keys || d_counts;
    const uint64_t span = std::min<uint64_t>(capacity, n_a + n_b); // what a call may write
    for (const auto &o : {std::make_pair((const void *)d_keys, (size_t)span * 8), std::make_pair((const void *)d_counts, (size_t)span * 4)})
        if (overlaps(o.first, o.second, d_a_keys, n_a * 8) || overlaps(o.first, o.second, d_a_counts, n_a * 4) ||
            overlaps(o.first, o.second, d_b_keys, n_b * 8) || overlaps(o.first, o.second, d_b_counts, n_b * 4)) {
            ctx_set_error(ctx, "s2k_count_merge_device: an output overlaps an input");
            return S2K_ERR_INVALID_ARG;
        }
    const Tab a{d_a_keys, d_a_counts, n_a}, b{d_b_keys, d_b_counts, n_b};
    const uint32_t minc = min_count ? min_count : 1u;
    MergeWs ws;
    uint64_t nd = 0, nk = 0;
    s2k_status s = merge_count(ctx, a, b, minc, &ws, &nd, &nk);
    if (s != S2K_OK) return s;
    *n_distinct = nd;
    *n_kept = nk;
    if (!want) return S2K_OK;
    if (nk > capacity) return S2K_ERR_CAPACITY;
    return merge_write(ctx, a, b, minc, ws, d_keys, d_counts, nk);
}

s2k_counter *s2k_counter_create(s2k_ctx *ctx, s2k_status *status) {
    if (!ctx) {
        if (status) *status = S2K_ERR_INVALID_ARG;
        return nullptr;
    }
    s2k_counter *c = new (std::nothrow) s2k_counter;
    if (!c) {
        if (status) *status = S2K_ERR_NOMEM;
        return nullptr;
    }
    c->ctx = ctx;
    if (status) *status = S2K_OK;
    return c;
}

void s2k_counter_destroy(s2k_counter *c) {
    if (!c) return;
    (void)hipSetDevice(ctx_device(c->ctx));
    for (auto &r : c->runs) run_free(r);
    if (c->scratch) (void)hipFree(c->scratch);
    delete c;
}

s2k_status s2k_counter_add(s2k_counter *c, const uint64_t *d_hash, uint64_t n) {
    if (!c || (n && !d_hash)) return S2K_ERR_INVALID_ARG;
    if (n == 0) return S2K_OK;
    if (hipSetDevice(ctx_device(c->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    constexpr uint64_t PIECE = 1ull << 31; // s2k_count_device_ex counts fewer than 2^32 keys per call
    for (uint64_t i = 0; i < n; i += PIECE) {
        const s2k_status s = counter_add_piece(c, d_hash + i, std::min(PIECE, n - i));
        if (s != S2K_OK) return s;
    }
    return S2K_OK;
}

s2k_status s2k_counter_finish(s2k_counter *c, uint32_t min_count, uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity, uint64_t *n_distinct,
                              uint64_t *n_kept) {
    if (!c || !n_distinct || !n_kept) return S2K_ERR_INVALID_ARG;
    *n_distinct = *n_kept = 0;
    if (hipSetDevice(ctx_device(c->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    while (c->runs.size() >= 2) { // one run, kept: add may go on, and a second finish is one filter pass
        s2k_counter::Run m{};
        const s2k_status s = merge_runs(c, c->runs[c->runs.size() - 2], c->runs.back(), &m);
        if (s != S2K_OK) return s;
        run_free(c->runs.back());
        c->runs.pop_back();
        run_free(c->runs.back());
        c->runs.back() = m;
    }
    if (c->runs.empty()) return S2K_OK;
    const s2k_counter::Run &r = c->runs[0];
    return s2k_count_merge_device(c->ctx, r.keys, r.counts, r.n, nullptr, nullptr, 0, min_count, d_keys, d_counts, capacity, n_distinct, n_kept);
}

} // extern "C"

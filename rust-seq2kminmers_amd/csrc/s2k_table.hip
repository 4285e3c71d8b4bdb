// s2k_table.hip -- look-ups against a count table that is strictly ascending by key (what s2k_count_device_ex(S2K_COUNT_SORTED),
// s2k_count_merge_device and s2k_counter_finish produce), and the per-read filter that keeps each read's solid k-min-mers
// (include/s2k.h: s2k_table_*).
//
// Index (once per table, table_index_kernel): one coalesced pass over the keys.  Each key is compared with the one before it (one
// flag word records a failure), and dir[p] = the first key index whose top B bits are at least p, for p = 0 .. 2^B (2^B + 1 u32
// entries; dir[2^B] = n).  Lane i writes the entries (prefix(key[i-1]), prefix(key[i])]; the last lane also the tail up to 2^B.
// B is chosen from n for 4-7 keys per bucket on average (TB_KEYS_PER_BUCKET, measured); buckets are not uniform and nothing depends
// on their size: a bucket that holds the whole table is searched the same way, only slower.
//
// Look-up (lookup_many): every lane takes TB_Q queries and issues all 2 x TB_Q directory loads before the first use; then the
// TB_Q binary searches over [dir[p], dir[p+1]) run interleaved, one key load per search per step (unconditional, at a clamped
// index, so the compiler keeps them in flight together); the count is loaded on a hit only.  No atomics.
//
// Filter, a stable stream compaction over the k-min-mer items, tiles of TB_TILE items (lane tid holds items r * 256 + tid):
//  1. filter_count_kernel: the look-up fused in; per item its count (4 B of workspace, so the write pass does not look up again),
//     per 64 items a kept mask (one wave's ballot) and the kept items before that word inside the tile; per tile the kept total.
//  2. launch_scan_u32 over the tile totals: each tile's first output slot.
//  3. filter_offsets_kernel: out->km_off[r] = kept items before input index km_off[r] (tile start + word prefix + mask popcount).
//  4. filter_write_kernel (only when item outputs are wanted and fit): each kept item goes to LDS at its tile-relative slot, one
//     output array at a time, and leaves the workgroup as one contiguous, coalesced run.  offset = item index - its read's first
//     item, the read found by a binary search of km_off narrowed to the reads that overlap the tile.
//
// Edges (s2k_table_edges), the same compaction with 0, 1 or 2 keys per item:
//  1. edges_count_kernel: the look-up fused in, returning each item's rank too; per item its oriented node (4 B of workspace), per
//     64 items the mask of items that start an adjacency and the keys before that word inside the tile; per tile the key total.  The
//     next tile's first item (the halo) is looked up once more by lane 0; read starts come from km_off, as in the filter.
//  2. launch_scan_u32 over the tile totals.
//  3. edges_write_kernel (only when keys are wanted and fit): each adjacency's key and its twin's to LDS at tile-relative slots; the
//     tile's keys leave as one contiguous run.
#include <algorithm>
#include <cstdlib>
#include <new>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_table_dev.h"

namespace s2k {
namespace {

__global__ __launch_bounds__(256) void table_index_kernel(const uint64_t *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t bits,
                                                          uint32_t *__restrict__ dir, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i], p = k >> shift;
    uint64_t from = 0;
    if (i > 0) {
        const uint64_t prev = keys[i - 1];
        if (!(prev < k)) {
            atomicOr(bad, 1u);
            return;
        }
        from = (prev >> shift) + 1;
    }
    for (uint64_t x = from; x <= p; x++) dir[x] = (uint32_t)i;
    if (i + 1 == n)
        for (uint64_t x = p + 1; x <= (1ull << bits); x++) dir[x] = n;
}

__global__ __launch_bounds__(TB_THREADS) void table_lookup_kernel(TableView tv, const uint64_t *__restrict__ query, uint64_t n,
                                                                  uint32_t *__restrict__ out) {
    const uint64_t base = (uint64_t)blockIdx.x * TB_TILE + threadIdx.x;
    uint64_t q[TB_Q];
    uint32_t c[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = query[std::min<uint64_t>(base + (uint64_t)r * TB_THREADS, n - 1)];
    lookup_many<false>(tv, q, c, nullptr);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if (base + (uint64_t)r * TB_THREADS < n) out[base + (uint64_t)r * TB_THREADS] = c[r];
}

struct FilterWs {
    uint32_t *cnt; // per item: its count
    CompactWs c;
};

__global__ __launch_bounds__(TB_THREADS) void filter_count_kernel(TableView tv, const uint64_t *__restrict__ hash, uint64_t n_items, uint32_t minc,
                                                                  FilterWs ws) {
    __shared__ uint32_t wc[TB_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint64_t q[TB_Q];
    uint32_t c[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = hash[std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, n_items - 1)];
    lookup_many<false>(tv, q, c, nullptr);
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        const bool valid = j < n_items;
        if (valid) ws.cnt[j] = c[r];
        const uint64_t m = __ballot(valid && c[r] >= minc);
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64; // first item of this wave's word
        if (lane == 0) {
            wc[r * 4 + wv] = (uint32_t)__popcll(m);
            if (w0 < n_items) ws.c.wmask[w0 >> 6] = m;
        }
    }
    __syncthreads();
    tile_prefixes(wc, t0, n_items, ws.c);
}

__global__ __launch_bounds__(256) void filter_offsets_kernel(const uint64_t *__restrict__ km_off, uint64_t n_reads, uint64_t n_items, uint64_t n_tiles,
                                                             FilterWs ws, uint64_t *__restrict__ o_km_off) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    o_km_off[r] = kept_before(ws.c, n_items, n_tiles, km_off[r]);
}

struct FilterIo {
    const uint64_t *km_off;
    uint64_t n_reads;
    const uint64_t *hash;
    const uint32_t *start, *end;
    const uint8_t *rev;
    uint64_t *o_hash;
    uint32_t *o_start, *o_end, *o_offset, *o_count;
    uint8_t *o_rev;
    uint64_t capacity;
};

__global__ __launch_bounds__(TB_THREADS) void filter_write_kernel(FilterIo io, uint64_t n_items, uint32_t minc, FilterWs ws) {
    __shared__ uint64_t s64[TB_TILE];
    __shared__ uint64_t sread[2];
    uint32_t *s32 = (uint32_t *)s64;
    uint8_t *s8 = (uint8_t *)s64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE, t1 = std::min<uint64_t>(t0 + TB_TILE, n_items);
    const uint64_t base = ws.c.tile_off[blockIdx.x], tot = ws.c.tile_off[blockIdx.x + 1] - base;
    if (tot == 0) return;
    if (tid < 2 && io.o_offset) // the reads that hold the tile's first and last item
        sread[tid] = read_of(io.km_off, 0, io.n_reads - 1, tid == 0 ? t0 : t1 - 1);
    uint32_t slot[TB_Q], cnt[TB_Q];
    uint32_t keep = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        cnt[r] = ws.cnt[std::min<uint64_t>(j, n_items - 1)];
        const bool kept = j < n_items && cnt[r] >= minc;
        const uint64_t m = __ballot(kept);
        const uint64_t w = (t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64) >> 6;
        slot[r] = (kept ? ws.c.wpre[w] : 0u) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        keep |= kept ? 1u << r : 0u;
    }
    __syncthreads();
    const uint64_t rlo = io.o_offset ? sread[0] : 0, rhi = io.o_offset ? sread[1] : 0;
#define TB_STAGE(ARR, VAL)                                                                  \
    do {                                                                                    \
        _Pragma("unroll") for (int r = 0; r < TB_Q; r++) if (keep & (1u << r)) {            \
            const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;                         \
            (void)j;                                                                        \
            ARR[slot[r]] = (VAL);                                                           \
        }                                                                                   \
        __syncthreads();                                                                    \
    } while (0)
#define TB_LEAVE(OUT, ARR)                                                                  \
    do {                                                                                    \
        for (uint32_t i = tid; i < tot; i += TB_THREADS) {                                  \
            if (base + i >= io.capacity) break; /* the host checked n_kept <= capacity */   \
            OUT[base + i] = ARR[i];                                                         \
        }                                                                                   \
        __syncthreads();                                                                    \
    } while (0)
    if (io.o_hash) {
        TB_STAGE(s64, io.hash[j]);
        TB_LEAVE(io.o_hash, s64);
    }
    if (io.o_start) {
        TB_STAGE(s32, io.start[j]);
        TB_LEAVE(io.o_start, s32);
    }
    if (io.o_end) {
        TB_STAGE(s32, io.end[j]);
        TB_LEAVE(io.o_end, s32);
    }
    if (io.o_rev) {
        TB_STAGE(s8, io.rev[j]);
        TB_LEAVE(io.o_rev, s8);
    }
    if (io.o_count) {
        TB_STAGE(s32, cnt[r]);
        TB_LEAVE(io.o_count, s32);
    }
    if (io.o_offset) {
        TB_STAGE(s32, (uint32_t)(j - io.km_off[read_of(io.km_off, rlo, rhi, j)]));
        TB_LEAVE(io.o_offset, s32);
    }
#undef TB_STAGE
#undef TB_LEAVE
}

// ---- graph edges (s2k_table_edges): the same compaction, 0, 1 or 2 keys per item ----------------------------------
constexpr uint32_t TB_NONE = 0xFFFFFFFFu; // an item that is not solid (oriented ids stay below 2^32 - 2: the table has < 2^31 keys)

struct EdgeWs {
    uint32_t *node; // per item: its oriented node 2 * rank + rev, TB_NONE when it is not solid
    CompactWs c;    // wmask: the items j for which (j, j + 1) is an adjacency; wpre, tile_kept: keys emitted, not items
};

// Items j and j + 1 form an adjacency when both are solid and j + 1 starts no read.  The tile's items and one halo item (the next
// tile's first, looked up by lane 0) go to LDS as oriented nodes; the read starts inside (t0, t0 + TB_TILE] are marked from the reads
// that a binary search of km_off finds there (an empty read marks the same item as the read after it).
__global__ __launch_bounds__(TB_THREADS) void edges_count_kernel(TableView tv, const uint64_t *__restrict__ km_off, uint64_t n_reads,
                                                                 const uint64_t *__restrict__ hash, const uint8_t *__restrict__ rev,
                                                                 uint64_t n_items, uint32_t minc, EdgeWs ws) {
    __shared__ uint32_t snode[TB_TILE + 1];
    __shared__ uint8_t sstart[TB_TILE + 1]; // sstart[x]: item t0 + x starts a read
    __shared__ uint32_t wc[TB_WORDS];
    __shared__ uint64_t sreads[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    uint64_t q[TB_Q];
    uint32_t c[TB_Q], pos[TB_Q];
#pragma unroll
    for (int r = 0; r < TB_Q; r++) q[r] = hash[std::min<uint64_t>(t0 + (uint64_t)r * TB_THREADS + tid, n_items - 1)];
    if (tid < 2) sreads[tid] = reads_upto(km_off, n_reads, t0 + (tid ? TB_TILE : 0));
    lookup_many<true>(tv, q, c, pos);
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        uint32_t u = TB_NONE;
        if (j < n_items) {
            if (c[r] >= minc) u = 2u * pos[r] + rev[j];
            ws.node[j] = u;
        }
        snode[r * TB_THREADS + tid] = u;
        sstart[r * TB_THREADS + tid] = 0;
    }
    if (tid == 0) {
        const uint64_t j = t0 + TB_TILE;
        uint32_t u = TB_NONE;
        if (j < n_items) {
            uint32_t hc, hp;
            lookup_one(tv, hash[j], &hc, &hp);
            if (hc >= minc) u = 2u * hp + rev[j];
        }
        snode[TB_TILE] = u;
        sstart[TB_TILE] = 0;
    }
    __syncthreads();
    for (uint64_t r = sreads[0] + tid; r < sreads[1]; r += TB_THREADS) {
        const uint64_t x = km_off[r] - t0; // in [1, TB_TILE] for a non-decreasing km_off; a table that is not one writes no LDS outside
        if (x <= TB_TILE) sstart[x] = 1;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int x = r * TB_THREADS + tid;
        const uint64_t j = t0 + x;
        const uint32_t u = snode[x], v = snode[x + 1];
        const bool adj = j + 1 < n_items && !sstart[x + 1] && u != TB_NONE && v != TB_NONE;
        const uint64_t m1 = __ballot(adj), m2 = __ballot(adj && v != (u ^ 1u)); // a hairpin (v == u ^ 1) is its own twin: one key
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64;
        if (lane == 0) {
            wc[r * 4 + wv] = (uint32_t)(__popcll(m1) + __popcll(m2));
            if (w0 < n_items) ws.c.wmask[w0 >> 6] = m1;
        }
    }
    __syncthreads();
    tile_prefixes(wc, t0, n_items, ws.c);
}

// each adjacency's key (u << 32 | v), then its twin's ((v ^ 1) << 32 | u ^ 1) unless it is its own, staged in LDS at tile-relative
// slots; the tile's keys leave as one contiguous run
__global__ __launch_bounds__(TB_THREADS) void edges_write_kernel(uint64_t n_items, EdgeWs ws, uint64_t *__restrict__ out, uint64_t capacity) {
    __shared__ uint64_t skey[2 * TB_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint64_t base = ws.c.tile_off[blockIdx.x], tot = ws.c.tile_off[blockIdx.x + 1] - base;
    if (tot == 0) return;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t j = t0 + (uint64_t)r * TB_THREADS + tid;
        const uint64_t w = (t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64) >> 6;
        const bool adj = j < n_items && ((ws.c.wmask[w] >> lane) & 1ull); // j + 1 < n_items whenever the bit is set
        uint32_t u = 0, v = 0;
        if (adj) {
            u = ws.node[j];
            v = ws.node[j + 1];
        }
        const bool two = adj && v != (u ^ 1u);
        const uint64_t below = (1ull << lane) - 1ull;
        const uint64_t m1 = __ballot(adj), m2 = __ballot(two);
        if (adj) {
            const uint32_t slot = ws.c.wpre[w] + (uint32_t)(__popcll(m1 & below) + __popcll(m2 & below));
            skey[slot] = ((uint64_t)u << 32) | v;
            if (two) skey[slot + 1] = ((uint64_t)(v ^ 1u) << 32) | (u ^ 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < tot; i += TB_THREADS) {
        if (base + i >= capacity) break; // the host checked n_edges <= capacity
        out[base + i] = skey[i];
    }
}

uint32_t table_bits(uint64_t n) {
    uint32_t b = 1;
    while (b < TB_MAX_BITS && (n >> (b + 1)) >= TB_KEYS_PER_BUCKET) b++; // largest b with n / 2^b >= 4
#ifdef S2K_DEBUG_KNOBS // `make KNOBS=1` only: S2K_DEBUG_TABLE_BITS fixes B (tools/table_rate.py --bits-sweep)
    if (const char *e = std::getenv("S2K_DEBUG_TABLE_BITS")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= (long)TB_MAX_BITS) b = (uint32_t)v;
    }
#endif
    return b;
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_table *s2k_table_create(s2k_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n, s2k_status *status) {
    auto fail = [&](s2k_status s) -> s2k_table * {
        if (status) *status = s;
        return nullptr;
    };
    if (!ctx || (n && !d_keys)) return fail(S2K_ERR_INVALID_ARG);
    Call c(ctx, "s2k_table_create");
    if (n >= (1ull << 32)) return fail(c.invalid("2^32 keys or more"));
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return fail(S2K_ERR_DEVICE);
    s2k_table *t = new (std::nothrow) s2k_table;
    if (!t) return fail(S2K_ERR_NOMEM);
    t->ctx = ctx;
    t->keys = d_keys;
    t->counts = d_counts;
    t->n = n;
    t->bits = table_bits(n);
    const size_t dir_n = (1ull << t->bits) + 1;
    if (hipMalloc((void **)&t->dir, (dir_n + 1) * 4) != hipSuccess) {
        delete t;
        return fail(c.nomem("directory allocation"));
    }
    uint32_t *bad = t->dir + dir_n;
    const uint32_t hbad = c.check(t->dir, (dir_n + 1) * 4, bad, [&] { // n == 0: every bucket empty
        if (n)
            hipLaunchKernelGGL(table_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.st, d_keys, (uint32_t)n, 64u - t->bits,
                               t->bits, t->dir, bad);
    });
    if (!c.ok() || hbad) {
        (void)hipFree(t->dir);
        delete t;
        return fail(!c.ok() ? c.device_error() : c.invalid("the keys are not strictly ascending"));
    }
    if (status) *status = S2K_OK;
    return t;
}

void s2k_table_destroy(s2k_table *t) {
    if (!t) return;
    (void)hipSetDevice(ctx_device(t->ctx));
    (void)hipFree(t->dir);
    delete t;
}

s2k_status s2k_table_lookup(s2k_table *t, const uint64_t *d_query, uint64_t n, uint32_t *d_out) {
    if (!t || (n && (!d_query || !d_out))) return S2K_ERR_INVALID_ARG;
    if (n == 0) return S2K_OK;
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Call c(t->ctx, "s2k_table_lookup");
    const uint64_t nb = (n + TB_TILE - 1) / TB_TILE;
    if (nb >= (1ull << 32)) return c.invalid("too many queries for one call");
    hipLaunchKernelGGL(table_lookup_kernel, dim3((unsigned)nb), dim3(TB_THREADS), 0, c.st, t->view(), d_query, n, d_out);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_table_filter(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, const s2k_solid_out *out,
                            uint64_t *n_kept) {
    if (n_kept) *n_kept = 0;
    if (!t || !in || !out || !n_kept || !in->km_off || !in->hash || !out->km_off || (out->start && !in->start) || (out->end && !in->end) ||
        (out->rev && !in->rev))
        return S2K_ERR_INVALID_ARG;
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Call c(t->ctx, "s2k_table_filter");
    const Ends ends = read_ends(c, in->km_off, nullptr, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ends.n_items < ends.km0) return c.invalid("in->km_off must start at 0 and end at or after its start");
    const uint64_t n_items = ends.n_items;
    if (n_items == 0) { // no items: every read is empty
        c.zero(out->km_off, (n_reads + 1) * 8);
        if (!c.sync()) return c.device_error();
        return S2K_OK;
    }
    const uint64_t nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32) || n_reads + 1 >= (1ull << 40)) return c.invalid("too many items for one call");
    Layout L;
    const auto cnt = L.take<uint32_t>(n_items);
    const auto cw = carve(L, n_items, nt);
    char *w = L.alloc(t->ctx);
    if (!w) return c.nomem();
    const FilterWs ws{cnt(w), cw(w)};
    const uint32_t minc = min_count ? min_count : 1u;
    hipLaunchKernelGGL(filter_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), in->hash, n_items, minc, ws);
    c.launched();
    c.scan(ws.c.tile_kept, nt, ws.c.tile_off, cw.scan_tmp(w));
    if (c.ok()) {
        hipLaunchKernelGGL(filter_offsets_kernel, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, c.st, in->km_off, n_reads, n_items, nt,
                           ws, out->km_off);
        c.launched();
    }
    uint64_t kept = 0;
    c.fetch(&kept, ws.c.tile_off + nt, 8);
    if (!c.sync()) return c.device_error();
    *n_kept = kept;
    const bool want = out->hash || out->start || out->end || out->rev || out->offset || out->count;
    if (!want || kept == 0) return S2K_OK;
    if (kept > out->capacity) return S2K_ERR_CAPACITY;
    FilterIo io{in->km_off, n_reads, in->hash, in->start, in->end, in->rev, out->hash, out->start, out->end, out->offset, out->count, out->rev,
                out->capacity};
    hipLaunchKernelGGL(filter_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, io, n_items, minc, ws);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

s2k_status s2k_table_edges(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, uint64_t *d_edge_keys,
                           uint64_t capacity, uint64_t *n_edges) {
    if (n_edges) *n_edges = 0;
    if (!t || !in || !n_edges || !in->km_off || !in->hash || !in->rev) return S2K_ERR_INVALID_ARG;
    Call c(t->ctx, "s2k_table_edges");
    if (t->n >= (1ull << 31)) return c.invalid("2^31 keys or more (oriented node ids are 32-bit)");
    if (hipSetDevice(ctx_device(t->ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const Ends ends = read_ends(c, in->km_off, nullptr, n_reads);
    if (!c.ok()) return c.device_error();
    if (ends.km0 != 0 || ends.n_items < ends.km0) return c.invalid("in->km_off must start at 0 and end at or after its start");
    const uint64_t n_items = ends.n_items;
    if (n_items == 0) return S2K_OK;
    const uint64_t nt = (n_items + TB_TILE - 1) / TB_TILE;
    if (nt >= (1ull << 32)) return c.invalid("too many items for one call");
    Layout L;
    const auto node = L.take<uint32_t>(n_items);
    const auto cw = carve(L, n_items, nt);
    char *w = L.alloc(t->ctx);
    if (!w) return c.nomem();
    const EdgeWs ws{node(w), cw(w)};
    const uint32_t minc = min_count ? min_count : 1u;
    hipLaunchKernelGGL(edges_count_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, t->view(), in->km_off, n_reads, in->hash, in->rev,
                       n_items, minc, ws);
    c.launched();
    c.scan(ws.c.tile_kept, nt, ws.c.tile_off, cw.scan_tmp(w));
    uint64_t total = 0;
    c.fetch(&total, ws.c.tile_off + nt, 8);
    if (!c.sync()) return c.device_error();
    *n_edges = total;
    if (!d_edge_keys || total == 0) return S2K_OK;
    if (total > capacity) return S2K_ERR_CAPACITY;
    hipLaunchKernelGGL(edges_write_kernel, dim3((unsigned)nt), dim3(TB_THREADS), 0, c.st, n_items, ws, d_edge_keys, capacity);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

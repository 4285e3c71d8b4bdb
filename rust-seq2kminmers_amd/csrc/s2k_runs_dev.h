// s2k_runs_dev.h -- a stream of items cut into runs, one output record per run: what s2k_table_thread, s2k_paths_walks,
// s2k_paths_bridge and s2k_paths_lift share.  Each of them brings the rule that says whether an item continues the
// one before it and the fields of a record; the rest is here.
//
// The stable stream compaction of s2k_compact_dev.h with two masks over tiles of TB_TILE items (lane tid holds items r * 256 + tid):
// heads (the item is kept and does not continue its predecessor) and tails (it is kept and its successor does not continue it).
//  1. A count kernel puts what its rule reads into LDS, index x + 1 <-> item t0 + x with the item before the tile at index 0 and
//     the one after it at TB_TILE + 1, and ends in run_count_end: two ballots per 64 items, tile_prefixes twice, and whether a run is
//     open at the tile's first item.
//  2. launch_scan_u32 over the heads per tile (count_runs).  Tails before a tile = heads before it - open: no second scan.
//  3. run_offsets_kernel: out_off[r] = heads before off[r].
//  4. A write kernel begins with run_tile.  Record s is the s-th head and the s-th tail: the heads' tile-relative indices go to LDS
//     at their slots; a tail at tile-relative slot k finds its head at slot k - open there, and the one tail per tile whose head lies
//     in an earlier tile finds it by head_item (one lane; nothing walks a run).  The tail's lane gathers what it needs of the head
//     (RunTile::head_of); each field is staged in LDS at the slots and leaves with leave_run (leave_field).
//
// Workspace per stream: per mask 8 B + 4 B per 64 items and 4 B + 8 B per tile, and 4 B per tile for open.
#pragma once
#include "s2k_compact_dev.h"

namespace s2k {
namespace {

struct RunWs {
    uint32_t *tile_open; // per tile: 1 when its first item continues the item before it
    CompactWs h, t;      // heads; tails (of the tails only wmask, wpre and tile_kept are used)
};

struct RunPieces {
    Layout::Piece<uint32_t> tile_open;
    CompactPieces h, t;
    RunWs operator()(char *w) const { return RunWs{tile_open(w), h(w), t(w)}; }
};
inline RunPieces carve_runs(Layout &L, uint64_t n, uint64_t n_tiles) {
    RunPieces p;
    p.tile_open = L.take<uint32_t>(n_tiles);
    p.h = carve(L, n, n_tiles);
    p.t = carve(L, n, n_tiles);
    return p;
}

// The end of a count kernel, after the barrier that makes the tile's LDS whole.  head(r, i) and tail(r, i): the lane's r-th item, at
// LDS index i, is a head / a tail (false for an item past n); open(): the tile's first item continues the one before it (one lane
// asks).
template <typename H, typename T, typename O>
__device__ __forceinline__ void run_count_end(const RunWs &ws, uint64_t t0, uint64_t n, H head, T tail, O open) {
    __shared__ uint32_t wch[TB_WORDS], wct[TB_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const int i = r * TB_THREADS + tid + 1;
        const uint64_t mh = __ballot(head(r, i)), mt = __ballot(tail(r, i));
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64;
        if (lane == 0) {
            wch[r * 4 + wv] = (uint32_t)__popcll(mh);
            wct[r * 4 + wv] = (uint32_t)__popcll(mt);
            if (w0 < n) {
                ws.h.wmask[w0 >> 6] = mh;
                ws.t.wmask[w0 >> 6] = mt;
            }
        }
    }
    if (tid == 0) ws.tile_open[blockIdx.x] = open();
    __syncthreads();
    tile_prefixes(wch, t0, n, ws.h);
    tile_prefixes(wct, t0, n, ws.t);
}

__global__ __launch_bounds__(256) void run_offsets_kernel(const uint64_t *__restrict__ off, uint64_t n_reads, uint64_t n, uint64_t n_tiles, CompactWs heads,
                                                          uint64_t *__restrict__ out_off) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    out_off[r] = kept_before(heads, n, n_tiles, off[r]);
}
inline void launch_run_offsets(Call &c, const uint64_t *off, uint64_t n_reads, uint64_t n, uint64_t n_tiles, const RunWs &ws, uint64_t *out_off) {
    c.launch(run_offsets_kernel, (unsigned)((n_reads + 1 + 255) / 256), 256, off, n_reads, n, n_tiles, ws.h, out_off);
}

// lane-private staging of one field: out[base + slot[r]] = val(r, j) for the lane's kept items j, through LDS (stage4: room for
// TB_TILE elements of T and a run's shift) and leave_run.  Nothing when out is NULL.  Ends with a barrier.
template <typename T, typename F>
__device__ __forceinline__ void leave_field(T *__restrict__ out, uint64_t base, uint32_t keep, const uint32_t (&slot)[TB_Q], uint32_t tot, uint4 *stage4, F val) {
    if (!out) return;
    T *stage = (T *)stage4;
    const uint64_t t0 = (uint64_t)blockIdx.x * TB_TILE;
    const uint32_t sh = shift_of(out + base);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if ((keep >> r) & 1u) stage[sh + slot[r]] = (T)val(r, t0 + (uint64_t)r * TB_THREADS + threadIdx.x);
    __syncthreads();
    leave_run(out + base, stage, sh, tot);
}

// what a write kernel knows of its tile once run_tile has filled it
struct RunTile {
    uint64_t t0, hbase, tbase; // the tile's first item; heads / tails before the tile
    uint32_t htot, ttot, open; // heads / tails in the tile; its first item continues the one before it
    uint32_t hslot[TB_Q], tslot[TB_Q], hkeep, tkeep;
    const uint32_t *shead; // LDS, by head slot: the head's item, relative to the tile
    const uint64_t *sopen; // LDS: the head of the open run
    // the head of the run whose tail is the lane's r-th item
    __device__ __forceinline__ uint64_t head_of(int r) const { return tslot[r] >= open ? t0 + shead[tslot[r] - open] : *sopen; }
    template <typename T, typename F>
    __device__ __forceinline__ void leave_heads(T *out, uint4 *stage4, F val) const { leave_field(out, hbase, hkeep, hslot, htot, stage4, val); }
    template <typename T, typename F>
    __device__ __forceinline__ void leave_tails(T *out, uint4 *stage4, F val) const { leave_field(out, tbase, tkeep, tslot, ttot, stage4, val); }
};

// The start of a write kernel.  false: the tile has no record to write and the kernel returns (the whole workgroup: no barrier has
// been passed).  heads_too: the kernel writes fields of the heads by themselves, so a tile that holds heads and no tail stays, and
// the open run's head is looked for only where a tail needs it.  before_barrier(): what else the kernel puts into LDS.
template <typename F>
__device__ __forceinline__ bool run_tile(const RunWs &ws, uint64_t n, bool heads_too, RunTile &rt, F before_barrier) {
    __shared__ uint32_t shead[TB_TILE];
    __shared__ uint64_t sopen;
    const int tid = threadIdx.x;
    rt.t0 = (uint64_t)blockIdx.x * TB_TILE;
    rt.hbase = ws.h.tile_off[blockIdx.x];
    rt.htot = (uint32_t)(ws.h.tile_off[blockIdx.x + 1] - rt.hbase);
    rt.ttot = ws.t.tile_kept[blockIdx.x];
    if (rt.ttot == 0 && !(heads_too && rt.htot)) return false;
    rt.open = ws.tile_open[blockIdx.x];
    rt.tbase = rt.hbase - rt.open; // tails before the tile: every head before it has its tail but the open one
    rt.hkeep = tile_slots(ws.h, rt.t0, n, rt.hslot), rt.tkeep = tile_slots(ws.t, rt.t0, n, rt.tslot);
    before_barrier();
    if (tid == 64 && rt.open && (!heads_too || rt.ttot)) sopen = head_item(ws.h, blockIdx.x, rt.tbase);
#pragma unroll
    for (int r = 0; r < TB_Q; r++)
        if ((rt.hkeep >> r) & 1u) shead[rt.hslot[r]] = (uint32_t)(r * TB_THREADS + tid);
    __syncthreads();
    rt.shead = shead, rt.sopen = &sopen;
    return true;
}
__device__ __forceinline__ bool run_tile(const RunWs &ws, uint64_t n, RunTile &rt) {
    return run_tile(ws, n, false, rt, [] {});
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// launch() the count kernel, scan the heads per tile, fetch their total and the count kernel's k counters (and its flag word, when
// the call reads one again), wait.  false: the call has failed.
template <typename F>
inline bool count_runs(Call &c, const RunWs &ws, uint64_t n_tiles, uint64_t *scan_tmp, F launch, uint64_t *total, const unsigned long long *totals,
                       unsigned long long *h, int k, const uint32_t *flag = nullptr, uint32_t *hflag = nullptr) {
    launch();
    c.launched();
    c.scan(ws.h.tile_kept, n_tiles, ws.h.tile_off, scan_tmp);
    c.fetch(total, ws.h.tile_off + n_tiles, 8);
    c.fetch(h, totals, (size_t)k * sizeof(*h));
    if (flag) c.fetch(hflag, flag, 4);
    return c.sync();
}

} // namespace
} // namespace s2k

// s2k_compact_dev.h -- the stable stream compaction over tiles of TB_TILE items that the filter and the edges (s2k_table.hip,
// DESIGN.md §3.8, §3.9) and the induced subgraph (s2k_simplify.hip, §3.12) share, and the one workgroup scan.
//
// Lane tid of a tile's workgroup holds items r * TB_THREADS + tid, r = 0 .. TB_Q - 1.  A count kernel ballots its items round by round
// (tile_ballot: word r * 4 + wave of the tile, the mask and its popcount) and ends in a barrier and tile_prefixes; launch_scan_u32 over tile_kept gives
// tile_off; a write kernel takes its slots from tile_slots, stages what it keeps in LDS at them and lets the run go with leave_run.
#pragma once
#include <algorithm>

#include "s2k_call.h"
#include "s2k_dev.h"

namespace s2k {
namespace {

constexpr int TB_THREADS = 256;
constexpr int TB_Q = 8;                          // items per lane
constexpr uint32_t TB_TILE = TB_THREADS * TB_Q; // 2 048 items per workgroup
constexpr int TB_WORDS = TB_TILE / 64;           // mask words per tile

// exclusive scan over a workgroup of NW waves; *total = the sum; wsum: NW words of LDS
template <int NW>
__device__ inline uint32_t block_excl_scan(uint32_t x, uint32_t *wsum, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const uint32_t v = wsum[j];
        pre += j < w ? v : 0u;
        tot += v;
    }
    __syncthreads();
    *total = tot;
    return pre + incl - x;
}

struct CompactWs {
    uint64_t *wmask;     // per 64 items: kept mask
    uint32_t *wpre;      // per 64 items: kept items before the word inside its tile
    uint32_t *tile_kept; // per tile
    uint64_t *tile_off;  // n_tiles + 1
};

// round r of a count kernel: the wave's ballot of `kept` (false for an item past n), its popcount to wc and the mask to its word.
// (filter_count_kernel, s2k_table.hip, and vote_count_kernel, s2k_vote.hip, write the same lines out: through this function their
// fused look-ups are scheduled into 91 and 90 VGPRs against 78, a wave per SIMD less.)
__device__ __forceinline__ void tile_ballot(uint32_t *wc, int r, uint64_t t0, uint64_t n, const CompactWs &ws, bool kept) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t m = __ballot(kept);
    const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64; // first item of this wave's word
    if (lane == 0) {
        wc[r * 4 + wv] = (uint32_t)__popcll(m);
        if (w0 < n) ws.wmask[w0 >> 6] = m;
    }
}

// after the TB_Q ballots of a tile (wc[r * 4 + wave] = the popcount of that word) and a barrier: the words' prefixes and the tile's
// total
__device__ __forceinline__ void tile_prefixes(const uint32_t *wc, uint64_t t0, uint64_t n_items, const CompactWs &ws) {
    const int tid = threadIdx.x;
    if (tid < TB_WORDS) { // word k of the tile = items t0 + 64 k ..: r = k / 4, wave k % 4
        uint32_t pre = 0;
        for (int x = 0; x < tid; x++) pre += wc[x];
        const uint64_t w0 = t0 + (uint64_t)tid * 64;
        if (w0 < n_items) ws.wpre[w0 >> 6] = pre;
        if (tid == TB_WORDS - 1) ws.tile_kept[blockIdx.x] = pre + wc[tid];
    }
}

// the tile-relative slot of each of the lane's TB_Q items -> the bits of those that are kept
__device__ __forceinline__ uint32_t tile_slots(const CompactWs &ws, uint64_t t0, uint64_t n_items, uint32_t slot[TB_Q]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t keep = 0;
#pragma unroll
    for (int r = 0; r < TB_Q; r++) {
        const uint64_t w0 = t0 + (uint64_t)r * TB_THREADS + (uint64_t)wv * 64;
        const uint64_t m = w0 < n_items ? ws.wmask[w0 >> 6] : 0ull;
        const uint32_t pre = w0 < n_items ? ws.wpre[w0 >> 6] : 0u;
        slot[r] = pre + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        keep |= (uint32_t)((m >> lane) & 1ull) << r;
    }
    return keep;
}

// kept items before input index j (j <= n_items), once launch_scan_u32 has written tile_off
__device__ inline uint64_t kept_before(const CompactWs &ws, uint64_t n_items, uint64_t n_tiles, uint64_t j) {
    if (j >= n_items) return ws.tile_off[n_tiles];
    const uint64_t w = j >> 6;
    const uint64_t below = (j & 63) ? ws.wmask[w] & ((1ull << (j & 63)) - 1ull) : 0ull;
    return ws.tile_off[j / TB_TILE] + ws.wpre[w] + (uint64_t)__popcll(below);
}

// the input index of kept item number s, which lies in a tile before tile b (one lane): the head of a run whose tail lies in tile b
// (s2k_runs_dev.h)
__device__ inline uint64_t head_item(const CompactWs &h, uint64_t b, uint64_t s) {
    uint64_t lo = 0, hi = b - 1; // the last tile whose first head is at or before s
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (h.tile_off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t rel = (uint32_t)(s - h.tile_off[lo]);
    const uint64_t w0 = lo * TB_WORDS; // a tile before another one holds all its words
    uint32_t a = 0, z = TB_WORDS - 1;  // the last word whose prefix is at or below rel
    while (a < z) {
        const uint32_t mid = (a + z + 1) >> 1;
        if (h.wpre[w0 + mid] <= rel) a = mid;
        else z = mid - 1;
    }
    uint64_t m = h.wmask[w0 + a];
    for (uint32_t k = rel - h.wpre[w0 + a]; k; k--) m &= m - 1; // drop the heads before it
    return (w0 + a) * 64 + (uint64_t)__ffsll((unsigned long long)m) - 1;
}

// elements between p and the 16-byte boundary below it
template <typename T>
__device__ __forceinline__ uint32_t shift_of(const T *p) {
    return (uint32_t)(((uintptr_t)p & 15u) / sizeof(T));
}

// lds[shift .. shift + tot) -> out[0 .. tot), out = the run's first output address and shift = shift_of(out): whole 16-byte pieces
// where a piece lies inside the run, element by element at the two ends.  Ends with a barrier: lds may be staged again.
template <typename T>
__device__ __forceinline__ void leave_run(T *__restrict__ out, const T *lds, uint32_t shift, uint32_t tot) {
    constexpr uint32_t V = 16 / sizeof(T);
    const uint32_t lo = shift, hi = shift + tot;
    const uint32_t vlo = std::min((lo + V - 1) & ~(V - 1), hi), vhi = std::max(hi & ~(V - 1), vlo);
    T *o = out - shift; // o[i] <-> lds[i]; o + vlo is 16-byte aligned
    for (uint32_t i = lo + threadIdx.x; i < vlo; i += TB_THREADS) o[i] = lds[i];
    for (uint32_t i = vlo / V + threadIdx.x; i < vhi / V; i += TB_THREADS) ((uint4 *)o)[i] = ((const uint4 *)lds)[i];
    for (uint32_t i = vhi + threadIdx.x; i < hi; i += TB_THREADS) o[i] = lds[i];
    __syncthreads();
}

constexpr uint32_t STAGE_PAD = 2; // a run starts at most 15 bytes into its first 16-byte piece: one more 8-byte element, rounded up

// the workspace of one stream of n items in n_tiles tiles, taken from a call's layout: the four arrays and the tile scan's block sums
struct CompactPieces {
    Layout::Piece<uint64_t> wmask;
    Layout::Piece<uint32_t> wpre, tile_kept;
    Layout::Piece<uint64_t> tile_off, scan_tmp;
    CompactWs operator()(char *w) const { return CompactWs{wmask(w), wpre(w), tile_kept(w), tile_off(w)}; }
};
inline CompactPieces carve(Layout &L, uint64_t n, uint64_t n_tiles) {
    const uint64_t words = (n + 63) / 64;
    CompactPieces p;
    p.wmask = L.take<uint64_t>(words);
    p.wpre = L.take<uint32_t>(words);
    p.tile_kept = L.take<uint32_t>(n_tiles);
    p.tile_off = L.take<uint64_t>(n_tiles + 1);
    p.scan_tmp = L.bytes<uint64_t>(scan_tmp_bytes(n_tiles));
    return p;
}

} // namespace
} // namespace s2k

// s2k_count_sorted.hip -- s2k_count_device_ex: the (key, count) pairs of the distinct values of d_hash[0..n) that occur at least
// min_count times, optionally in ascending key order (include/s2k.h).  What a rust-mdbg-like consumer needs from the count: the
// rare k-min-mers (sequencing errors) dropped on the device, the "solid" ones in an order it can binary-search or merge.
//
// Partition, then count in LDS ("Counting with a cutoff"):
//  1. MSD radix partition by the key's top byte, then by its next 8..10 bits inside each top-level bucket (10 at configs[1]'s size:
//     ~512 keys per bucket on average) -- 2^16..2^18 buckets in key order, ping-pong d_hash -> B -> A.  Each pass is a histogram, a per-segment scan, a scatter.  The scatter ranks a tile of 8 192 keys
//     by digit in LDS and stores it digit run by digit run, so that consecutive lanes write consecutive addresses.
//  2. One workgroup per bucket: an open-addressing table of 4 096 slots in LDS (LDS atomics for the counts), the entries under
//     min_count dropped, the rest compacted (block scan) and, with S2K_COUNT_SORTED, bitonic-sorted in LDS; the pairs go back IN PLACE
//     over the bucket's own keys (a bucket has at least as many keys as kept pairs), with the kept count per bucket.
//  3. An exclusive scan of the kept counts and a copy kernel lay the buckets' pairs out back to back.
// Skew rule:
//  * many copies of few keys: every wave collapses the lanes that hold its first active lane's key into ONE LDS atomic of the
//    popcount, so a wave of one heavy hitter costs one atomic, not 64;
//  * many distinct keys: a bucket whose table reaches OVF_LIMIT distinct keys gives up and is re-partitioned on the next byte
//    (8 bits per level down to bit 0); a bucket of the last level holds one distinct key, so the recursion ends.  The pairs of those
//    deeper buckets are assembled in key order by the host (the rare path: one synchronisation per extra level).
// 2^64-1 is the table's EMPTY sentinel; a bucket counts it in an LDS side counter and appends it last (it is the largest key).
#include <algorithm>
#include <vector>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_compact_dev.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

constexpr uint64_t EMPTY = ~0ull;
constexpr int TILE_THREADS = 512;
constexpr int TILE_KPT = 16;
constexpr uint32_t TILE = TILE_THREADS * TILE_KPT; // keys per partition tile: 64 KiB of LDS staging
constexpr uint32_t RMAX = 1024;                  // widest digit (10 bits): staging + 3 x 4 KiB -> 2 workgroups per CU
constexpr int CNT_THREADS = 512;
constexpr int CNT_KPT = 4;                  // independent key loads in flight per lane
constexpr uint32_t SLOTS = 4096;            // LDS table: 32 KiB keys + 16 KiB counts -> 3 workgroups per CU
constexpr uint32_t OVF_LIMIT = 3072;        // distinct keys at which a bucket is re-partitioned (load factor 0.75; at most
                                            // OVF_LIMIT - 1 + CNT_THREADS claims ever happen, < SLOTS: probing always ends)
constexpr uint32_t KEPT_OVF = 0xFFFFFFFFu;  // kept[] of a bucket that was re-partitioned

struct Meta {
    unsigned long long n_distinct, n_kept;
    uint32_t n_next; // buckets re-partitioned at the next level
    uint32_t pad;
};

__device__ inline uint32_t lds_slot(uint64_t k) { // the bucket's keys share their top bits: mix the rest into the top 12
    k ^= k >> 32;
    k *= 0x9E3779B97F4A7C15ull;
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    return (uint32_t)(k >> 52);
}

// out[0..m] = exclusive prefix of f(in[0..m)), f = ceil(x / TILE) (tiles of a segment) or x; one workgroup
__global__ __launch_bounds__(1024) void excl_scan_kernel(const uint32_t *__restrict__ in, uint32_t m, int tiles, uint32_t *__restrict__ out) {
    __shared__ uint32_t wsum[16];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < m; b += 1024) {
        const uint32_t i = b + threadIdx.x;
        uint32_t x = i < m ? in[i] : 0u;
        if (tiles) x = (x + TILE - 1) / TILE;
        uint32_t tot;
        const uint32_t e = block_excl_scan<16>(x, wsum, &tot);
        if (i < m) out[i] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) out[m] = carry;
}

__global__ void init_kernel(uint32_t *seg_start, uint32_t *seg_len, uint32_t n) {
    seg_start[0] = 0;
    seg_len[0] = n;
}

// tile t -> (segment, first key, end) via the prefix of tiles per segment; false past the last tile
__device__ inline bool tile_of(const uint32_t *tile_off, uint32_t nseg, const uint32_t *seg_start, const uint32_t *seg_len, uint32_t t,
                               uint32_t *s, uint32_t *b, uint32_t *e) {
    if (t >= tile_off[nseg]) return false;
    uint32_t lo = 0, hi = nseg; // largest s with tile_off[s] <= t
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tile_off[mid] <= t) lo = mid;
        else hi = mid;
    }
    *s = lo;
    const uint32_t st = seg_start[lo], len = seg_len[lo];
    *b = st + (t - tile_off[lo]) * TILE;
    *e = (uint32_t)min((uint64_t)*b + TILE, (uint64_t)st + len);
    return true;
}

__global__ __launch_bounds__(TILE_THREADS) void part_hist_tile_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_start,
                                                                      const uint32_t *__restrict__ seg_len, uint32_t nseg,
                                                                      const uint32_t *__restrict__ tile_off, int shift, int bits, uint32_t *hist) {
    __shared__ uint32_t lh[RMAX];
    const uint32_t radix = 1u << bits, mask = radix - 1;
    uint32_t s, b, e;
    if (!tile_of(tile_off, nseg, seg_start, seg_len, blockIdx.x, &s, &b, &e)) return;
    uint64_t k[TILE_KPT]; // all loads in flight before the first LDS atomic
#pragma unroll
    for (int j = 0; j < TILE_KPT; j++) {
        const uint64_t i = (uint64_t)b + j * TILE_THREADS + threadIdx.x;
        k[j] = i < e ? keys[i] : 0;
    }
    for (uint32_t d = threadIdx.x; d < radix; d += TILE_THREADS) lh[d] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TILE_KPT; j++)
        if ((uint64_t)b + j * TILE_THREADS + threadIdx.x < e) atomicAdd(&lh[(k[j] >> shift) & mask], 1u);
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < radix; d += TILE_THREADS)
        if (lh[d]) atomicAdd(&hist[s * radix + d], lh[d]);
}

// one workgroup per segment: child buckets (start, len) of its 2^bits digits; cursor = start
__global__ __launch_bounds__(256) void part_children_kernel(const uint32_t *__restrict__ seg_start, const uint32_t *c_len, int bits,
                                                            uint32_t *__restrict__ c_start, uint32_t *__restrict__ cursor) {
    __shared__ uint32_t wsum[4];
    const uint32_t radix = 1u << bits;
    uint32_t carry = seg_start[blockIdx.x];
    for (uint32_t d0 = 0; d0 < radix; d0 += 256) {
        const uint32_t d = d0 + threadIdx.x, c = blockIdx.x * radix + d;
        uint32_t tot;
        const uint32_t e = block_excl_scan<4>(d < radix ? c_len[c] : 0u, wsum, &tot);
        if (d < radix) {
            c_start[c] = carry + e;
            cursor[c] = carry + e;
        }
        carry += tot;
    }
}

__global__ __launch_bounds__(TILE_THREADS) void part_scatter_tile_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_start,
                                                                         const uint32_t *__restrict__ seg_len, uint32_t nseg,
                                                                         const uint32_t *__restrict__ tile_off, int shift, int bits,
                                                                         uint32_t *cursor, uint64_t *__restrict__ out) {
    __shared__ uint64_t stage[TILE];
    __shared__ uint32_t lh[RMAX], loff[RMAX], gb[RMAX], wsum[TILE_THREADS / 64];
    const uint32_t radix = 1u << bits, mask = radix - 1;
    uint32_t s, b, e;
    if (!tile_of(tile_off, nseg, seg_start, seg_len, blockIdx.x, &s, &b, &e)) return;
    uint64_t k[TILE_KPT];
    uint32_t r[TILE_KPT];
#pragma unroll
    for (int j = 0; j < TILE_KPT; j++) {
        const uint64_t i = (uint64_t)b + j * TILE_THREADS + threadIdx.x;
        k[j] = i < e ? keys[i] : 0;
    }
    for (uint32_t d = threadIdx.x; d < radix; d += TILE_THREADS) lh[d] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TILE_KPT; j++)
        if ((uint64_t)b + j * TILE_THREADS + threadIdx.x < e) r[j] = atomicAdd(&lh[(k[j] >> shift) & mask], 1u);
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t d0 = 0; d0 < radix; d0 += TILE_THREADS) { // radix <= RMAX: at most two rounds
        const uint32_t d = d0 + threadIdx.x;
        uint32_t tot;
        const uint32_t h = d < radix ? lh[d] : 0u;
        const uint32_t ex = block_excl_scan<TILE_THREADS / 64>(h, wsum, &tot);
        if (d < radix) {
            loff[d] = carry + ex;
            if (h) gb[d] = atomicAdd(&cursor[s * radix + d], h);
        }
        carry += tot;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TILE_KPT; j++)
        if ((uint64_t)b + j * TILE_THREADS + threadIdx.x < e) {
            const uint32_t d = (k[j] >> shift) & mask;
            stage[loff[d] + r[j]] = k[j];
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < e - b; i += TILE_THREADS) { // digit runs: consecutive lanes, consecutive addresses
        const uint64_t x = stage[i];
        const uint32_t d = (x >> shift) & mask;
        out[gb[d] + (i - loff[d])] = x;
    }
}

__device__ inline void lds_insert(uint64_t k, uint32_t c, uint64_t *tkey, uint32_t *tcnt, uint32_t *ndist, volatile uint32_t *ovf) {
    uint32_t h = lds_slot(k);
    for (uint32_t probe = 0; probe < SLOTS; probe++) {
        uint64_t cur = ((volatile uint64_t *)tkey)[h];
        if (cur == EMPTY) {
            cur = atomicCAS((unsigned long long *)&tkey[h], (unsigned long long)EMPTY, (unsigned long long)k);
            if (cur == EMPTY) {
                atomicAdd(&tcnt[h], c);
                if (atomicAdd(ndist, 1u) + 1 >= OVF_LIMIT) *ovf = 1;
                return;
            }
        }
        if (cur == k) {
            atomicAdd(&tcnt[h], c);
            return;
        }
        h = (h + 1) & (SLOTS - 1);
    }
    *ovf = 1; // unreachable by the claim bound above; kept so that a full table can never lose a key
}

// one workgroup per bucket (see the header comment); keys[start .. start+len) are overwritten with the bucket's kept keys
__global__ __launch_bounds__(CNT_THREADS) void count_bucket_kernel(uint64_t *keys, uint32_t *__restrict__ cnt_out, const uint32_t *__restrict__ c_start,
                                                                   const uint32_t *__restrict__ c_len, uint32_t min_count, int sorted,
                                                                   uint32_t *__restrict__ kept, uint32_t *__restrict__ next_start,
                                                                   uint32_t *__restrict__ next_len, Meta *meta) {
    __shared__ uint64_t tkey[SLOTS];
    __shared__ uint32_t tcnt[SLOTS];
    __shared__ uint32_t ndist, side, ovf, wsum[CNT_THREADS / 64];
    const uint32_t c = blockIdx.x, start = c_start[c], len = c_len[c];
    if (len == 0) {
        if (threadIdx.x == 0) kept[c] = 0;
        return;
    }
    for (uint32_t i = threadIdx.x; i < SLOTS; i += CNT_THREADS) {
        tkey[i] = EMPTY;
        tcnt[i] = 0;
    }
    if (threadIdx.x == 0) ndist = side = ovf = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t base = 0; base < len; base += CNT_THREADS * CNT_KPT) {
        if (*(volatile uint32_t *)&ovf) break; // one LDS read per wave: uniform
        uint64_t k[CNT_KPT];
#pragma unroll
        for (int j = 0; j < CNT_KPT; j++) {
            const uint64_t i = base + j * CNT_THREADS + threadIdx.x;
            k[j] = i < len ? keys[start + i] : 0;
        }
#pragma unroll
        for (int j = 0; j < CNT_KPT; j++) {
            const bool valid = base + j * CNT_THREADS + threadIdx.x < len;
            const uint64_t ms = __ballot(valid && k[j] == EMPTY);
            if (ms && lane == 0) atomicAdd(&side, (uint32_t)__popcll(ms));
            const bool v = valid && k[j] != EMPTY;
            const uint64_t m = __ballot(v);
            if (!m) continue;
            const int lead = __ffsll((unsigned long long)m) - 1;
            const uint64_t k0 = __shfl(k[j], lead);
            const uint64_t meq = __ballot(v && k[j] == k0); // run collapse: one atomic for every copy of the lead key
            if (lane == lead) lds_insert(k0, (uint32_t)__popcll(meq), tkey, tcnt, &ndist, &ovf);
            if (v && k[j] != k0) lds_insert(k[j], 1u, tkey, tcnt, &ndist, &ovf);
        }
    }
    __syncthreads();
    if (ovf) { // too many distinct keys for the table: the next level splits this bucket on the next byte
        if (threadIdx.x == 0) {
            kept[c] = KEPT_OVF;
            const uint32_t q = atomicAdd(&meta->n_next, 1u);
            next_start[q] = start;
            next_len[q] = len;
        }
        return;
    }
    // compact the kept entries to the front of the table (through registers: all reads before any write)
    constexpr int SPT = SLOTS / CNT_THREADS;
    uint64_t ek[SPT];
    uint32_t ec[SPT], mine = 0;
#pragma unroll
    for (int j = 0; j < SPT; j++) {
        ek[j] = tkey[threadIdx.x * SPT + j];
        ec[j] = tcnt[threadIdx.x * SPT + j];
        mine += (ek[j] != EMPTY && ec[j] >= min_count) ? 1u : 0u;
    }
    uint32_t nk;
    uint32_t pos = block_excl_scan<CNT_THREADS / 64>(mine, wsum, &nk);
#pragma unroll
    for (int j = 0; j < SPT; j++)
        if (ek[j] != EMPTY && ec[j] >= min_count) {
            tkey[pos] = ek[j];
            tcnt[pos] = ec[j];
            pos++;
        }
    uint32_t m2 = 1;
    while (m2 < nk) m2 <<= 1;
    if (sorted) {
        for (uint32_t i = nk + threadIdx.x; i < m2; i += CNT_THREADS) tkey[i] = EMPTY; // pads sort last
        __syncthreads();
        for (uint32_t kk = 2; kk <= m2; kk <<= 1)
            for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                for (uint32_t i = threadIdx.x; i < m2 / 2; i += CNT_THREADS) {
                    const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo + j;
                    const uint64_t a = tkey[lo], bb = tkey[hi];
                    if ((a > bb) == ((lo & kk) == 0)) {
                        tkey[lo] = bb;
                        tkey[hi] = a;
                        const uint32_t t = tcnt[lo];
                        tcnt[lo] = tcnt[hi];
                        tcnt[hi] = t;
                    }
                }
                __syncthreads();
            }
    } else {
        __syncthreads();
    }
    const uint32_t sc = side;
    const uint32_t side_kept = sc >= min_count && sc > 0 ? 1u : 0u;
    for (uint32_t i = threadIdx.x; i < nk; i += CNT_THREADS) {
        keys[start + i] = tkey[i];
        cnt_out[start + i] = tcnt[i];
    }
    if (threadIdx.x == 0) {
        if (side_kept) {
            keys[start + nk] = EMPTY;
            cnt_out[start + nk] = sc;
        }
        kept[c] = nk + side_kept;
        atomicAdd(&meta->n_distinct, (unsigned long long)(ndist + (sc > 0 ? 1u : 0u)));
        atomicAdd(&meta->n_kept, (unsigned long long)(nk + side_kept));
    }
}

// entry e: len[e] pairs at src[e] (array B if which[e], else A) -> outputs at dst[e]
__global__ __launch_bounds__(256) void copy_pairs_kernel(const uint64_t *__restrict__ A, const uint64_t *__restrict__ B, const uint32_t *__restrict__ C,
                                                         const uint32_t *__restrict__ src, const uint32_t *__restrict__ len,
                                                         const uint32_t *__restrict__ dst, const uint32_t *__restrict__ which,
                                                         uint64_t *__restrict__ o_keys, uint32_t *__restrict__ o_cnt) {
    const uint32_t e = blockIdx.x, s = src[e], l = len[e], d = dst[e];
    if (l == KEPT_OVF) return;
    const uint64_t *K = (which && which[e]) ? B : A;
    for (uint32_t i = threadIdx.x; i < l; i += 256) {
        if (o_keys) o_keys[d + i] = K[s + i];
        if (o_cnt) o_cnt[d + i] = C[s + i];
    }
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_count_device_ex(s2k_ctx *ctx, const uint64_t *d_hash, uint64_t n, uint32_t min_count, uint32_t flags, uint64_t *d_keys,
                               uint32_t *d_counts, uint64_t capacity, uint64_t *n_distinct, uint64_t *n_kept) {
    if (!ctx || (!d_hash && n) || !n_distinct || !n_kept || (flags & ~S2K_COUNT_SORTED) || n >= (1ull << 32)) return S2K_ERR_INVALID_ARG;
    *n_distinct = *n_kept = 0;
    if (n == 0) return S2K_OK;
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    Call c(ctx, "s2k_count_device_ex");
    const uint32_t minc = min_count ? min_count : 1u;
    const int sorted = (flags & S2K_COUNT_SORTED) ? 1 : 0;
    const bool want = d_keys || d_counts;

    // workspace: A, B (n keys), C (n counts), segment / child / scan arrays, meta
    const uint64_t nsegmax = std::max<uint64_t>(256, n / OVF_LIMIT + 1); // a re-partitioned bucket holds >= OVF_LIMIT keys
    // second digit: 8..10 bits, so that a bucket holds ~512 keys on average -- k-min-mer hash prefixes are not uniform (the densest
    // 16-bit prefixes of configs[1] hold ~4.5x the mean), and a bucket must stay under OVF_LIMIT distinct keys to be counted in one go
    int bits2 = 8;
    while (bits2 < 10 && (n >> (8 + bits2)) > 512) bits2++;
    const uint32_t nb2 = 256u << bits2; // level-2 buckets
    const uint64_t maxchild = std::max<uint64_t>(nb2, 256 * nsegmax);
    Layout L;
    const auto pA = L.take<uint64_t>(n), pB = L.take<uint64_t>(n);
    const auto pC = L.take<uint32_t>(n);
    const auto pSS = L.take<uint32_t>(nsegmax), pSL = L.take<uint32_t>(nsegmax), pTO = L.take<uint32_t>(nsegmax + 1);
    const auto pCS = L.take<uint32_t>(maxchild), pCL = L.take<uint32_t>(maxchild), pCU = L.take<uint32_t>(maxchild), pKE = L.take<uint32_t>(maxchild);
    const auto pDO = L.take<uint32_t>(maxchild + 1);
    const auto pL1S = L.take<uint32_t>(256), pL1L = L.take<uint32_t>(256);
    const auto pM = L.take<Meta>(1);
    char *ws = L.alloc(ctx);
    if (!ws) return c.nomem();
    uint64_t *A = pA(ws), *B = pB(ws);
    uint32_t *C = pC(ws), *seg_s = pSS(ws), *seg_l = pSL(ws), *tile_off = pTO(ws);
    uint32_t *c_s = pCS(ws), *c_l = pCL(ws), *cur = pCU(ws), *kept = pKE(ws);
    uint32_t *dst_off = pDO(ws), *l1_s = pL1S(ws), *l1_l = pL1L(ws);
    Meta *meta = pM(ws);
    hipStream_t st = c.st;

    // one partition level: segments (ss, sl)[0..nseg) of src -> 256 children each (cs, cl) in dst
    auto level = [&](const uint64_t *src, uint64_t *dst, const uint32_t *ss, const uint32_t *sl, uint32_t nseg, uint64_t nkeys, int shift,
                     int bits, uint32_t *cs, uint32_t *cl) {
        const uint64_t tiles = nkeys / TILE + nseg; // bound; blocks past the real count return at once
        hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(1024), 0, st, sl, nseg, 1, tile_off);
        c.zero(cl, ((size_t)nseg << bits) * 4);
        hipLaunchKernelGGL(part_hist_tile_kernel, dim3((unsigned)tiles), dim3(TILE_THREADS), 0, st, src, ss, sl, nseg, tile_off, shift, bits, cl);
        hipLaunchKernelGGL(part_children_kernel, dim3(nseg), dim3(256), 0, st, ss, cl, bits, cs, cur);
        hipLaunchKernelGGL(part_scatter_tile_kernel, dim3((unsigned)tiles), dim3(TILE_THREADS), 0, st, src, ss, sl, nseg, tile_off, shift, bits, cur, dst);
        c.launched();
    };
    auto count = [&](uint64_t *keys, uint32_t nchild) {
        c.zero(&meta->n_next, 4);
        hipLaunchKernelGGL(count_bucket_kernel, dim3(nchild), dim3(CNT_THREADS), 0, st, keys, C, c_s, c_l, minc, sorted, kept, seg_s, seg_l, meta);
        c.launched();
    };
    Meta hm{};
    auto read_meta = [&]() {
        c.fetch(&hm, meta, sizeof(Meta));
        c.sync();
    };

    c.zero(meta, sizeof(Meta));
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(1), 0, st, seg_s, seg_l, (uint32_t)n);
    level(d_hash, B, seg_s, seg_l, 1, n, 56, 8, l1_s, l1_l);              // top byte
    level(B, A, l1_s, l1_l, 256, n, 56 - bits2, bits2, c_s, c_l);        // next bits2 bits: nb2 buckets in A
    count(A, nb2);
    read_meta();

    bool over = false;
    if (c.ok() && hm.n_next == 0) { // the usual case: every bucket fitted its LDS table
        over = hm.n_kept > capacity && want;
        if (want && !over && hm.n_kept) {
            hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(1024), 0, st, kept, nb2, 0, dst_off);
            hipLaunchKernelGGL(copy_pairs_kernel, dim3(nb2), dim3(256), 0, st, A, B, C, c_s, kept, dst_off, nullptr, d_keys, d_counts);
            c.launched();
            c.sync();
        }
    } else if (c.ok()) { // re-partition the buckets that overflowed, one byte deeper per level; assemble in key order here
        struct Fin {
            uint32_t start, len, which;
        };
        std::vector<Fin> fin;
        std::vector<uint32_t> hs, hk;
        auto collect = [&](uint32_t nchild, uint32_t which) {
            hs.resize(nchild);
            hk.resize(nchild);
            c.fetch(hs.data(), c_s, (size_t)nchild * 4);
            c.fetch(hk.data(), kept, (size_t)nchild * 4);
            if (!c.sync()) return;
            for (uint32_t i = 0; i < nchild; i++)
                if (hk[i] != KEPT_OVF && hk[i] != 0) fin.push_back({hs[i], hk[i], which});
        };
        if (want) collect(nb2, 0);
        uint64_t *src = A, *dst = B; // level L >= 3 reads what level L-1 wrote and writes the other array
        for (int shift = 56 - bits2; shift > 0 && c.ok() && hm.n_next;) {
            const int bits = std::min(8, shift);
            shift -= bits;
            const uint32_t nseg = hm.n_next;
            level(src, dst, seg_s, seg_l, nseg, n, shift, bits, c_s, c_l);
            count(dst, nseg << bits);
            read_meta();
            if (want) collect(nseg << bits, dst == B ? 1u : 0u);
            std::swap(src, dst);
        }
        if (c.ok() && hm.n_next) c.e = hipErrorUnknown; // cannot happen: a last-level bucket has one distinct key
        over = hm.n_kept > capacity && want;
        if (c.ok() && want && !over && !fin.empty()) {
            std::sort(fin.begin(), fin.end(), [](const Fin &a, const Fin &b) { return a.start < b.start; });
            std::vector<uint32_t> fs(fin.size()), fl(fin.size()), fd(fin.size()), fw(fin.size());
            uint32_t acc = 0;
            for (size_t i = 0; i < fin.size(); i++) {
                fs[i] = fin[i].start;
                fl[i] = fin[i].len;
                fw[i] = fin[i].which;
                fd[i] = acc;
                acc += fin[i].len;
            }
            for (size_t b0 = 0; b0 < fin.size() && c.ok(); b0 += maxchild) { // the child arrays carry the list, in chunks
                const size_t m = std::min<size_t>(maxchild, fin.size() - b0);
                c.copy(c_s, fs.data() + b0, m * 4, hipMemcpyHostToDevice);
                c.copy(c_l, fl.data() + b0, m * 4, hipMemcpyHostToDevice);
                c.copy(kept, fd.data() + b0, m * 4, hipMemcpyHostToDevice);
                c.copy(cur, fw.data() + b0, m * 4, hipMemcpyHostToDevice);
                if (c.ok()) {
                    hipLaunchKernelGGL(copy_pairs_kernel, dim3((unsigned)m), dim3(256), 0, st, A, B, C, c_s, c_l, kept, cur, d_keys, d_counts);
                    c.launched();
                }
                c.sync(); // the host lists are read by the copies: keep them until done
            }
        }
    }
    if (!c.ok()) return c.device_error();
    *n_distinct = hm.n_distinct;
    *n_kept = hm.n_kept;
    return over ? S2K_ERR_CAPACITY : S2K_OK;
}

} // extern "C"

// s2k_graph.hip -- the adjacency (CSR) of the minimizer-space graph over its 2 * n_nodes oriented nodes, from a strictly ascending
// table of edge keys (u << 32 | v): what s2k_count_device_ex(S2K_COUNT_SORTED) or s2k_counter_finish writes from the keys of
// s2k_table_edges (include/s2k.h: s2k_graph_adjacency).
//
//  1. adj_check_kernel: every key against the one before it and both of its node ids against 2 * n_nodes; one flag word records a
//     failure.  The host reads the flag before anything is written.
//  2. adj_write_kernel: lane i writes dst[i] and the row offsets of the sources since key i-1 (row_off[x] = i for src(i-1) < x <=
//     src(i)), as table_index_kernel writes its directory; lanes past the last source write row_off[x] = n_edges up to x = 2 * n_nodes.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

__global__ __launch_bounds__(256) void adj_check_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n_ids, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    const bool ok = (k >> 32) < n_ids && (k & 0xFFFFFFFFull) < n_ids && (i == 0 || keys[i - 1] < k);
    if (!ok) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(256) void adj_write_kernel(const uint64_t *__restrict__ keys, uint64_t n, uint64_t n_ids, uint64_t *__restrict__ row_off,
                                                        uint32_t *__restrict__ dst) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t k = keys[i], s = k >> 32;
        if (dst) dst[i] = (uint32_t)k;
        const uint64_t from = i > 0 ? (keys[i - 1] >> 32) + 1 : 0;
        for (uint64_t x = from; x <= s; x++) row_off[x] = i;
    }
    const uint64_t last = n ? keys[n - 1] >> 32 : 0; // the tail: every source after the last one (all of them when there is no edge)
    if (i <= n_ids && (n == 0 || i > last)) row_off[i] = n;
}

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_graph_adjacency(s2k_ctx *ctx, const uint64_t *d_edge_keys, uint64_t n_edges, uint64_t n_nodes, uint64_t *d_row_off,
                               uint32_t *d_dst) {
    if (!ctx || !d_row_off || (n_edges && !d_edge_keys)) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_graph_adjacency");
    if (n_nodes >= (1ull << 31)) return c.invalid("2^31 nodes or more (oriented node ids are 32-bit)");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    const uint64_t n_ids = 2 * n_nodes;
    if (n_edges) {
        uint32_t *bad = (uint32_t *)ctx_count_table(ctx, 4);
        if (!bad) return c.nomem();
        const uint32_t hbad = c.check(bad, 4, bad, [&] {
            hipLaunchKernelGGL(adj_check_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, c.st, d_edge_keys, n_edges, n_ids, bad);
        });
        if (!c.ok()) return c.device_error();
        if (hbad) return c.invalid("the keys are not strictly ascending or name a node id >= 2 * n_nodes");
    }
    const uint64_t lanes = std::max<uint64_t>(n_edges, n_ids + 1);
    if ((lanes + 255) / 256 >= (1ull << 32)) return c.invalid("too many edges for one call");
    hipLaunchKernelGGL(adj_write_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, c.st, d_edge_keys, n_edges, n_ids, d_row_off, d_dst);
    c.launched();
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"

/* C consumer of the abundance-cutoff count (tests/test_count_solid.py compiles it with -Wall -Werror). */
#include "s2k.h"

s2k_status solid_pairs(s2k_ctx *ctx, const uint64_t *d_hash, uint64_t n, uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity,
                       uint64_t *n_kept) {
    uint64_t n_distinct = 0;
    return s2k_count_device_ex(ctx, d_hash, n, 2u, S2K_COUNT_SORTED, d_keys, d_counts, capacity, &n_distinct, n_kept);
}

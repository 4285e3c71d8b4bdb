/* C consumer of the count merge and the accumulating counter (tests/test_count_merge.py compiles it with -Wall -Werror). */
#include "s2k.h"

s2k_status solid_over_batches(s2k_ctx *ctx, const uint64_t *const *d_batches, const uint64_t *lens, int n_batches, uint64_t *d_keys,
                              uint32_t *d_counts, uint64_t capacity, uint64_t *n_kept) {
    s2k_status st = S2K_OK;
    uint64_t n_distinct = 0;
    int i;
    s2k_counter *c = s2k_counter_create(ctx, &st);
    if (!c) return st;
    for (i = 0; i < n_batches && st == S2K_OK; i++) st = s2k_counter_add(c, d_batches[i], lens[i]);
    if (st == S2K_OK) st = s2k_counter_finish(c, 2u, d_keys, d_counts, capacity, &n_distinct, n_kept);
    s2k_counter_destroy(c);
    return st;
}

s2k_status merge_two(s2k_ctx *ctx, const uint64_t *ak, const uint32_t *ac, uint64_t na, const uint64_t *bk, const uint32_t *bc, uint64_t nb,
                     uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity, uint64_t *n_kept) {
    uint64_t n_distinct = 0;
    return s2k_count_merge_device(ctx, ak, ac, na, bk, bc, nb, 1u, d_keys, d_counts, capacity, &n_distinct, n_kept);
}

s2k_status count_files(s2k_ctx *ctx, const char *const *paths, int n_files, s2k_counter *c, s2k_counts *totals) {
    const s2k_params p = {31u, 10u, 0.01, S2K_MODE_HPC, 0u};
    s2k_status st = S2K_OK;
    int i;
    for (i = 0; i < n_files && st == S2K_OK; i++) st = s2k_run_file_count(ctx, paths[i], &p, 0, c, totals + i, 0);
    return st;
}

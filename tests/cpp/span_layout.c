/* Prints what s2k_paths_spans and s2k_graph_resolve_mask share with their callers as "name value" lines (tests/test_span.py compares
 * them with the mirrors in rust-seq2kminmers_amd/__init__.py): the layout of the s2k_thread_out the paths are read from, S2K_STEP_LINKED
 * and S2K_NO_PARTNER.  The two prototypes are declared once more, as the bindings spell them: a header that differs does not compile.
 * Plain C11: the header must be usable from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
s2k_status s2k_paths_spans(s2k_ctx *, uint64_t, const s2k_thread_out *, uint64_t, const uint64_t *, const uint32_t *, uint64_t, const uint64_t *,
                           uint64_t, uint64_t *, uint64_t, uint64_t *, uint64_t *, uint64_t *, uint64_t *);
s2k_status s2k_graph_resolve_mask(s2k_ctx *, const uint64_t *, const uint32_t *, uint64_t, uint64_t, const uint64_t *, const uint32_t *, uint64_t,
                                  uint32_t, uint8_t *, uint32_t *, uint64_t *, uint64_t *);
int main(void) {
    SZ(s2k_thread_out); OFF(s2k_thread_out, path_off); OFF(s2k_thread_out, unitig); OFF(s2k_thread_out, pos); OFF(s2k_thread_out, count);
    OFF(s2k_thread_out, flags);
    printf("S2K_STEP_LINKED %u\n", S2K_STEP_LINKED);
    printf("S2K_NO_PARTNER %u\n", S2K_NO_PARTNER);
    return 0;
}

/* Prints what s2k_graph_untangle and s2k_unitig_expand share with their callers as "name value" lines (tests/test_untangle.py compares
 * them with the mirrors in rust-seq2kminmers_amd/__init__.py): S2K_NO_PARTNER, the status codes the two calls return, and the layout of
 * the s2k_unitig_out whose arrays the expansion reads and writes.  The two prototypes are declared once more, as the bindings spell
 * them: a header that differs does not compile.  Plain C11: the header must be usable from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
s2k_status s2k_graph_untangle(s2k_ctx *, const uint64_t *, const uint32_t *, uint64_t, uint64_t, const uint8_t *, const uint32_t *, const uint64_t *,
                              const uint32_t *, uint64_t *, uint32_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t, uint64_t *, uint64_t *);
s2k_status s2k_unitig_expand(s2k_ctx *, const uint64_t *, const uint32_t *, const uint8_t *, uint64_t, uint64_t, const uint32_t *, const uint64_t *,
                             const uint32_t *, const uint8_t *, uint64_t, uint64_t, uint64_t *, uint32_t *, uint32_t *, uint32_t *, uint8_t *,
                             uint32_t *, uint64_t, uint64_t *);
int main(void) {
    SZ(s2k_unitig_out); OFF(s2k_unitig_out, capacity); OFF(s2k_unitig_out, uni_off); OFF(s2k_unitig_out, members);
    OFF(s2k_unitig_out, node_unitig); OFF(s2k_unitig_out, node_pos); OFF(s2k_unitig_out, circular);
    printf("S2K_NO_PARTNER %u\n", S2K_NO_PARTNER);
    printf("S2K_ERR_INVALID_ARG %d\n", (int)S2K_ERR_INVALID_ARG);
    printf("S2K_ERR_CAPACITY %d\n", (int)S2K_ERR_CAPACITY);
    printf("S2K_ABI_VERSION %d\n", S2K_ABI_VERSION);
    return 0;
}

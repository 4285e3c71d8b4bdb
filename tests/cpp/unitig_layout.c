/* Prints sizeof / offsetof of s2k_unitig_out as "name value" lines (tests/test_unitigs.py compares them with the ctypes mirror
 * UnitigOut in rust-seq2kminmers_amd/__init__.py).  Plain C11: the header must be usable from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
int main(void) {
    SZ(s2k_unitig_out); OFF(s2k_unitig_out, capacity); OFF(s2k_unitig_out, uni_off); OFF(s2k_unitig_out, members);
    OFF(s2k_unitig_out, node_unitig); OFF(s2k_unitig_out, node_pos); OFF(s2k_unitig_out, circular);
    return 0;
}

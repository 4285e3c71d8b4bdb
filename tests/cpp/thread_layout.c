/* Prints sizeof / offsetof of s2k_thread_out and s2k_node_place as "name value" lines (tests/test_thread.py compares them with the
 * ctypes mirror ThreadOut and the numpy dtype NodePlace in rust-seq2kminmers_amd/__init__.py).  Plain C11: the header must be usable
 * from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
int main(void) {
    SZ(s2k_thread_out); OFF(s2k_thread_out, capacity); OFF(s2k_thread_out, path_off); OFF(s2k_thread_out, unitig); OFF(s2k_thread_out, pos);
    OFF(s2k_thread_out, count); OFF(s2k_thread_out, item); OFF(s2k_thread_out, flags); OFF(s2k_thread_out, start); OFF(s2k_thread_out, end);
    SZ(s2k_node_place); OFF(s2k_node_place, unitig); OFF(s2k_node_place, pos); OFF(s2k_node_place, len); OFF(s2k_node_place, circular);
    printf("S2K_STEP_LINKED %u\n", S2K_STEP_LINKED);
    return 0;
}

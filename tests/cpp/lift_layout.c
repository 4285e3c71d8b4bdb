/* The layouts and constants that the Python mirrors of s2k_unitig_copy_places and s2k_paths_lift rely on, printed by the C compiler:
 * tests/test_lift.py compares them with ctypes and numpy. */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define FIELD(S, F) printf(#S "." #F " %zu %zu\n", offsetof(S, F), sizeof(((S *)0)->F))

int main(void) {
    printf("sizeof.s2k_thread_out %zu\n", sizeof(s2k_thread_out));
    FIELD(s2k_thread_out, capacity);
    FIELD(s2k_thread_out, path_off);
    FIELD(s2k_thread_out, unitig);
    FIELD(s2k_thread_out, pos);
    FIELD(s2k_thread_out, count);
    FIELD(s2k_thread_out, item);
    FIELD(s2k_thread_out, flags);
    FIELD(s2k_thread_out, start);
    FIELD(s2k_thread_out, end);
    printf("sizeof.s2k_node_place %zu\n", sizeof(s2k_node_place));
    FIELD(s2k_node_place, unitig);
    FIELD(s2k_node_place, pos);
    FIELD(s2k_node_place, len);
    FIELD(s2k_node_place, circular);
    printf("S2K_NO_COPY %llu\n", (unsigned long long)S2K_NO_COPY);
    printf("S2K_STEP_LINKED %llu\n", (unsigned long long)S2K_STEP_LINKED);
    printf("S2K_ABI_VERSION %d\n", S2K_ABI_VERSION);
    printf("S2K_ERR_INVALID_ARG %d\n", (int)S2K_ERR_INVALID_ARG);
    printf("S2K_ERR_CAPACITY %d\n", (int)S2K_ERR_CAPACITY);
    return 0;
}

/* prints the layout of s2k_walk_out and the walk constants for tests/test_walk.py */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define F(f) printf("s2k_walk_out." #f " %zu %zu\n", offsetof(s2k_walk_out, f), sizeof(((s2k_walk_out *)0)->f))

int main(void) {
    printf("sizeof.s2k_walk_out %zu\n", sizeof(s2k_walk_out));
    F(capacity);
    F(walk_off);
    F(first_step);
    F(n_steps);
    F(items);
    F(qstart);
    F(qend);
    F(path_len);
    F(path_start);
    F(path_end);
    F(flags);
    F(edge);
    printf("S2K_WALK_CIRCULAR %u\n", S2K_WALK_CIRCULAR);
    printf("S2K_NO_EDGE %u\n", S2K_NO_EDGE);
    return 0;
}

/* prints the layout of s2k_thread_out, which s2k_paths_bridge reads and writes, and the step constant for tests/test_bridge.py */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define F(f) printf("s2k_thread_out." #f " %zu %zu\n", offsetof(s2k_thread_out, f), sizeof(((s2k_thread_out *)0)->f))

int main(void) {
    printf("sizeof.s2k_thread_out %zu\n", sizeof(s2k_thread_out));
    F(capacity);
    F(path_off);
    F(unitig);
    F(pos);
    F(count);
    F(item);
    F(flags);
    F(start);
    F(end);
    printf("S2K_STEP_LINKED %u\n", S2K_STEP_LINKED);
    printf("S2K_ABI_VERSION %d\n", S2K_ABI_VERSION);
    return 0;
}

/* prints the layout of s2k_segment_out and the constants of the segmented alignment for tests/test_align_segments.py */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define F(f) printf("s2k_segment_out." #f " %zu %zu\n", offsetof(s2k_segment_out, f), sizeof(((s2k_segment_out *)0)->f))

int main(void) {
    printf("sizeof.s2k_segment_out %zu\n", sizeof(s2k_segment_out));
    F(capacity);
    F(seg_off);
    F(q_begin);
    F(q_end);
    F(t_begin);
    F(t_end);
    printf("S2K_NO_STEP %llu\n", (unsigned long long)S2K_NO_STEP);
    printf("S2K_SEGMENT_LEN %u\n", S2K_SEGMENT_LEN);
    printf("S2K_SEGMENT_MIN_LEN %u\n", S2K_SEGMENT_MIN_LEN);
    printf("S2K_SEGMENT_STATS %d\n", S2K_SEGMENT_STATS);
    return 0;
}

/* prints the layout of s2k_align_out and the alignment constants for tests/test_align.py */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define F(f) printf("s2k_align_out." #f " %zu %zu\n", offsetof(s2k_align_out, f), sizeof(((s2k_align_out *)0)->f))

int main(void) {
    printf("sizeof.s2k_align_out %zu\n", sizeof(s2k_align_out));
    F(capacity);
    F(edits);
    F(flags);
    F(ops_off);
    F(n_ops);
    F(matches);
    F(ops);
    printf("S2K_ALIGN_OVER %u\n", S2K_ALIGN_OVER);
    printf("S2K_ALIGN_BAD_PATH %u\n", S2K_ALIGN_BAD_PATH);
    printf("S2K_ALIGN_MAX_EDITS %u\n", S2K_ALIGN_MAX_EDITS);
    printf("S2K_ALIGN_WAVES %u\n", S2K_ALIGN_WAVES);
    printf("S2K_CIGAR_I %u\n", S2K_CIGAR_I);
    printf("S2K_CIGAR_D %u\n", S2K_CIGAR_D);
    printf("S2K_CIGAR_EQ %u\n", S2K_CIGAR_EQ);
    printf("S2K_CIGAR_X %u\n", S2K_CIGAR_X);
    return 0;
}

/* prints the layout of s2k_pile and the pile-up constants for tests/test_pileup.py */
#include <stddef.h>
#include <stdio.h>

#include "s2k.h"

#define F(f) printf("s2k_pile." #f " %zu %zu\n", offsetof(s2k_pile, f), sizeof(((s2k_pile *)0)->f))

int main(void) {
    printf("sizeof.s2k_pile %zu\n", sizeof(s2k_pile));
    F(match);
    F(del);
    F(sub);
    F(ins);
    F(ins_long);
    printf("S2K_PILEUP_MAX_SHIFT %u\n", S2K_PILEUP_MAX_SHIFT);
    printf("S2K_PILEUP_STATS %d\n", S2K_PILEUP_STATS);
    printf("S2K_CONSENSUS_STATS %d\n", S2K_CONSENSUS_STATS);
    printf("S2K_ALIGN_OVER %u\n", S2K_ALIGN_OVER);
    printf("S2K_ALIGN_BAD_PATH %u\n", S2K_ALIGN_BAD_PATH);
    return 0;
}

/* Prints sizeof / offsetof of s2k_node_seqs as "name value" lines (tests/test_unitig_sequences.py compares them with the ctypes mirror
 * NodeSeqs in rust-seq2kminmers_amd/__init__.py).  Plain C11: the header must be usable from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
int main(void) {
    SZ(s2k_node_seqs); OFF(s2k_node_seqs, seq_off); OFF(s2k_node_seqs, seq_len); OFF(s2k_node_seqs, shift_fwd);
    OFF(s2k_node_seqs, shift_rev); OFF(s2k_node_seqs, rev); OFF(s2k_node_seqs, pool); OFF(s2k_node_seqs, pool_capacity);
    return 0;
}

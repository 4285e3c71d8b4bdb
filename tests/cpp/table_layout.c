/* Prints sizeof / offsetof of s2k_solid_out as "name value" lines (tests/test_count_table.py compares them with the ctypes mirror
 * SolidOut in rust-seq2kminmers_amd/__init__.py).  Plain C11: the header must be usable from C. */
#include "s2k.h"
#include <stddef.h>
#include <stdio.h>
#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
int main(void) {
    SZ(s2k_solid_out); OFF(s2k_solid_out, capacity); OFF(s2k_solid_out, km_off); OFF(s2k_solid_out, hash); OFF(s2k_solid_out, start);
    OFF(s2k_solid_out, end); OFF(s2k_solid_out, rev); OFF(s2k_solid_out, offset); OFF(s2k_solid_out, count);
    return 0;
}

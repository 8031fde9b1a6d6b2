/* ref_bcftools <mpileup|call> ...: dispatch to the reference's own entry points, nothing else (test infrastructure) */
#include <stdio.h>
#include <string.h>

int main_mpileup(int argc, char *argv[]);
int main_vcfcall(int argc, char *argv[]);

int main(int argc, char *argv[]) {
    if (argc >= 2 && !strcmp(argv[1], "mpileup")) return main_mpileup(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "call")) return main_vcfcall(argc - 1, argv + 1);
    fprintf(stderr, "usage: ref_bcftools mpileup|call ...\n");
    return 2;
}

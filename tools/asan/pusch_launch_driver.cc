// CPU driver for the PUSCH demodulator's launch rule (openlte_amd/csrc/pusch_launch.h), built with -fsanitize=address,undefined: answers
// queries, one per line of the file named on the command line (or of stdin),
//   M_max words_max maxlog noise n_rx lds_limit threads_override mmse
// with one line each,
//   fits family threads S_par lds_off lds_bytes label compiled
// fits: 1, or 0 for a combining launch that does not fit lds_limit at S_par = 1; family: plain / llr / llr_noise / llr_rx / llr_mmse;
// compiled: pusch_variant_compiled for the launch just planned -- whether k_pusch_demod exists for its family, width and antenna count.
//   pusch_launch_driver [query file]
#include <cstdio>

#include "../../openlte_amd/csrc/pusch_launch.h"

using namespace pusch_geom;

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!fp) { printf("pusch launch driver: cannot read %s\n", argv[1]); return 1; }
    static const char *const family[] = {"plain", "llr", "llr_noise", "llr_rx", "llr_mmse"};
    unsigned           M_max, words_max, maxlog, noise, n_rx, threads, mmse;
    unsigned long long limit;
    long               n = 0;
    while (fscanf(fp, "%u %u %u %u %u %llu %u %u", &M_max, &words_max, &maxlog, &noise, &n_rx, &limit, &threads, &mmse) == 8) {
        PuschLaunch L;
        const bool  fits = pusch_launch_plan(M_max, words_max, {maxlog != 0, noise != 0, mmse != 0, n_rx}, (size_t)limit, threads, &L);
        printf("%d %s %u %u %zu %zu %s %d\n", fits ? 1 : 0, family[(int)L.family], L.threads, L.S_par, L.lds_off, L.lds_bytes, L.label,
               pusch_variant_compiled(L.family, L.threads, L.n_rx) ? 1 : 0);
        n++;
    }
    if (fp != stdin) fclose(fp);
    fprintf(stderr, "pusch launch driver: %ld queries answered\n", n);
    return 0;
}

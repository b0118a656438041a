// CPU driver for the PDSCH demodulators' launch rule (openlte_amd/csrc/pdsch_launch.h), built with -fsanitize=address,undefined: answers
// queries, one per line of the file named on the command line (or of stdin),
//   n_alloc {N_prb cfi mod_type} x n_alloc  n_ant compact maxlog noise pack gold_table threads_override
// (n_alloc = 0: the four sizes max_pairs max_words max_words_lo max_symb_hi themselves in place of allocations) with one line each,
//   max_pairs max_words max_words_lo max_symb_hi family n_ant threads pairs_al words_al e_cap lds_bytes flags label noise_first compiled
// family: ref_one_port / ref_one_port_compact / ref_ports / llr / llr_noise; compiled: pdsch_variant_compiled for the launch just planned --
// whether the demodulator kernel exists for its family and port count.
//   pdsch_launch_driver [query file]
#include <cstdio>

#include "../../openlte_amd/csrc/pdsch_launch.h"

using namespace pdsch_geom;

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!fp) { printf("pdsch launch driver: cannot read %s\n", argv[1]); return 1; }
    static const char *const family[] = {"ref_one_port", "ref_one_port_compact", "ref_ports", "llr", "llr_noise"};
    unsigned n_alloc;
    long     n = 0;
    while (fscanf(fp, "%u", &n_alloc) == 1) {
        PdschDemodSizes s;
        unsigned        a, b, c, d, n_ant, compact, maxlog, noise, pack, gold;
        int             over;
        bool            ok = true;
        if (n_alloc == 0) {
            ok = fscanf(fp, "%u %u %u %u", &a, &b, &c, &d) == 4;
            if (ok) { s.max_pairs = a; s.max_words = b; s.max_words_lo = c; s.max_symb_hi = d; }
        }
        for (unsigned i = 0; ok && i < n_alloc; i++) {
            ok = fscanf(fp, "%u %u %u", &a, &b, &c) == 3;
            if (ok) s.add(a, b, c);
        }
        if (!ok || fscanf(fp, "%u %u %u %u %u %u %d", &n_ant, &compact, &maxlog, &noise, &pack, &gold, &over) != 7) break;
        PdschLaunch L;
        pdsch_launch_plan(s, n_ant, compact != 0, maxlog != 0, noise != 0, pack != 0, gold != 0, over, &L);
        printf("%u %u %u %u %s %u %u %u %u %u %zu %u %s %d %d\n", s.max_pairs, s.max_words, s.max_words_lo, s.max_symb_hi, family[(int)L.family], L.n_ant, L.threads,
               L.pairs_al, L.words_al, L.e_cap, L.lds_bytes, L.flags, L.label, L.noise_first ? 1 : 0, pdsch_variant_compiled(L.family, L.n_ant) ? 1 : 0);
        n++;
    }
    if (fp != stdin) fclose(fp);
    fprintf(stderr, "pdsch launch driver: %ld queries answered\n", n);
    return 0;
}

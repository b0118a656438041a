// CPU driver for the host half of the PUSCH plans and of the 3GPP transport-block mode (openlte_amd/csrc/pusch_plan.h, dlsch3_layout.h, pure
// host code), built with -fsanitize=address,undefined: answers queries, one per line of the file named on the command line (or of stdin), with
// one line each.  A query is a list of unsigned integers:
//   P brief N_rb spec caller_dmrs has_uci n_units {subframe cell} x n_units  n_rec {rec} x n_rec        pusch_plan_layout
//   D brief N_soft M_dl_harq  n_rec {rec} x n_rec                                                       mi_dlsch3_layout
//   A N_rb n_units spec has_uci rec                                                                     pusch_alloc_check alone
// rec = rep unit mod_type tbs rv_idx tx_mode rnti N_prb first_prb last0 last1 [O_ack O_ri Qp_ack Qp_ri Q_cqi]: `rep` copies of an allocation whose
// resource blocks are first_prb, first_prb + 1, .. in both slots, the LAST entry of slot 0 / 1 replaced by last0 / last1 where that is not
// 0xFFFFFFFF; the five control-information numbers only where has_uci is 1 (D: never).  The uplink configuration is fixed (UL below); caller
// reference signals are the pattern 1000 a + j for allocation a's j-th float.
// An answer is `rc=<code> key=value ... err=<message to the end of the line>`; lists are comma separated, records inside a list colon
// separated.  brief = 1 leaves the per-allocation and per-slot lists out (the plans of a few hundred thousand allocations).  dmrs_ok[a]: the
// pool at the allocation's offset holds what mi_lte_ul_dmrs_pusch gives for its (cell, subframe, N_prb), or the caller's pattern.
//   pusch_plan_driver [query file]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../openlte_amd/csrc/pusch_plan.h"

namespace {

const mi_lte_ul_cfg UL = {3, 0, 0, 2, 5};

struct Rec { mi_lte_pdsch_alloc al; mi_lte_ulsch_uci uci; unsigned rep; };

bool next_u(FILE *fp, unsigned long long *v) { return fscanf(fp, "%llu", v) == 1; }

bool read_rec(FILE *fp, bool has_uci, Rec *out)
{
    unsigned long long v[16];
    const int          n = has_uci ? 16 : 11;
    for (int i = 0; i < n; i++)
        if (!next_u(fp, &v[i])) return false;
    memset(out, 0, sizeof(*out));
    mi_lte_pdsch_alloc &al = out->al;
    out->rep = (unsigned)v[0];
    al.unit = (uint32_t)v[1]; al.mod_type = (uint32_t)v[2]; al.tbs = (uint32_t)v[3]; al.rv_idx = (uint32_t)v[4]; al.tx_mode = (uint32_t)v[5];
    al.rnti = (uint32_t)v[6]; al.N_prb = (uint32_t)v[7];
    const uint32_t n_fill = al.N_prb < 112 ? al.N_prb : 112;
    for (uint32_t s = 0; s < 2; s++)
        for (uint32_t i = 0; i < n_fill; i++) al.prb[s][i] = (uint8_t)(v[8] + i);
    if (n_fill && v[9] != 0xFFFFFFFFull) al.prb[0][n_fill - 1] = (uint8_t)v[9];
    if (n_fill && v[10] != 0xFFFFFFFFull) al.prb[1][n_fill - 1] = (uint8_t)v[10];
    if (has_uci) out->uci = {(uint8_t)v[11], (uint8_t)v[12], (uint16_t)v[13], (uint16_t)v[14], (uint32_t)v[15]};
    return true;
}

template <typename T, typename F> void list(const char *key, const std::vector<T> &v, F one)
{
    printf(" %s=", key);
    for (size_t i = 0; i < v.size(); i++) { if (i) putchar(','); one(v[i]); }
}
void list_u(const char *key, const std::vector<uint32_t> &v) { list(key, v, [](uint32_t x) { printf("%u", x); }); }
void list_z(const char *key, const std::vector<size_t> &v) { list(key, v, [](size_t x) { printf("%zu", x); }); }

void print_g3(const MiDlsch3Layout &g, bool brief)
{
    printf(" n_slot=%zu soft_bytes=%zu bits_bytes=%zu", g.slots.size(), g.soft_bytes, g.bits_bytes);
    list("g3_groups", g.groups, [](const MiKGroup &x) { printf("%u:%u:%u:%u", x.K, x.n_cb, x.cb_base, x.e_max); });
    list_z("g_soft", g.g_soft); list_z("g_bits", g.g_bits);
    if (brief) return;
    list_u("a_slot", g.a_slot); list_u("a_nc", g.a_nc); list_u("a_K", g.a_K); list_u("a_tbs", g.a_tbs); list_z("a_soft", g.a_soft);
    list("slots", g.slots, [](const Dl3Slot &s) { printf("%u:%u:%u:%u:%u:%u:%u:%u", s.alloc, s.r, s.C, s.K, s.xs, s.soft_off4, s.bits_off8, s.pad); });
}

bool expand(FILE *fp, bool has_uci, std::vector<mi_lte_pdsch_alloc> *allocs, std::vector<mi_lte_ulsch_uci> *uci)
{
    unsigned long long n_rec;
    if (!next_u(fp, &n_rec)) return false;
    for (unsigned long long i = 0; i < n_rec; i++) {
        Rec r;
        if (!read_rec(fp, has_uci, &r)) return false;
        allocs->insert(allocs->end(), r.rep, r.al);
        uci->insert(uci->end(), r.rep, r.uci);
    }
    return true;
}

bool query_P(FILE *fp)
{
    unsigned long long h[6];
    for (auto &x : h)
        if (!next_u(fp, &x)) return false;
    const bool brief = h[0] != 0, spec = h[2] != 0, caller = h[3] != 0, has_uci = h[4] != 0;
    const mi_lte_dl_cfg cfg = {2048, (uint32_t)h[1], 1, MI_LTE_IQ_F32_PLANAR};
    std::vector<uint32_t> sf(h[5]), cell(h[5]);
    for (size_t u = 0; u < sf.size(); u++) {
        unsigned long long a, b;
        if (!next_u(fp, &a) || !next_u(fp, &b)) return false;
        sf[u] = (uint32_t)a; cell[u] = (uint32_t)b;
    }
    std::vector<mi_lte_pdsch_alloc> allocs;
    std::vector<mi_lte_ulsch_uci>   uci;
    if (!expand(fp, has_uci, &allocs, &uci)) return false;
    const uint32_t     n = (uint32_t)allocs.size();
    std::vector<float> pat;
    if (caller)
        for (uint32_t a = 0; a < n; a++)
            for (uint32_t j = 0; j < 48 * (allocs[a].N_prb <= 110 ? allocs[a].N_prb : 0); j++) pat.push_back((float)(1000 * a + j));
    PuschPlanLayout L;
    const char     *err = nullptr;
    const int rc = pusch_plan_layout(&cfg, &UL, caller ? pat.data() : nullptr, sf.data(), cell.data(), (uint32_t)sf.size(), allocs.data(), n, spec,
                                     has_uci ? uci.data() : nullptr, &L, &err);
    printf("rc=%d", rc);
    if (rc == MI_LTE_OK) {
        printf(" n=%u e_bytes=%zu M_max=%u words_max=%u max_tbs=%u out_stride=%u dmrs_n=%zu x_end=%u", n, L.e_bytes, L.M_max, L.words_max, L.max_tbs,
               L.out_stride, L.dmrs.size(), L.x_off.empty() ? 0u : L.x_off.back());
        list("groups", L.groups, [](const MiKGroup &x) { printf("%u:%u:%u:%u", x.K, x.n_cb, x.cb_base, x.e_max); });
        if (!brief) {
            list("desc", L.desc, [](const PuschDesc &d) { printf("%u:%u:%u", d.subfr, d.cell, d.dmrs_off); });
            std::vector<uint32_t> ok(n);
            for (uint32_t a = 0, at = 0; a < n; a++) {
                const uint32_t     M = 12 * allocs[a].N_prb;
                std::vector<float> want(4 * (size_t)M);
                if (caller) { memcpy(want.data(), &pat[at], sizeof(float) * 4 * M); at += 4 * M; }
                else if (mi_lte_ul_dmrs_pusch(&UL, L.desc[a].cell, L.desc[a].subfr, allocs[a].N_prb, &want[0], &want[M], &want[2 * M], &want[3 * M]) != MI_LTE_OK) want.assign(4 * (size_t)M, -1.0f);
                ok[a] = (size_t)L.desc[a].dmrs_off + 4 * M <= L.dmrs.size() && memcmp(want.data(), &L.dmrs[L.desc[a].dmrs_off], sizeof(float) * 4 * M) == 0;
            }
            list_u("dmrs_ok", ok); list_u("c_init", L.c_init); list_u("e_len", L.e_len); list_u("e_off", L.e_off);
            list("row", L.row, [](uint8_t r) { printf("%u", r); });
            list_u("cb_alloc", L.cb_alloc); list_u("x_off", L.x_off); list_u("G", L.G);
        }
        if (spec) print_g3(L.g3, brief);
    }
    printf(" err=%s\n", err ? err : "");
    return true;
}

bool query_D(FILE *fp)
{
    unsigned long long h[3];
    for (auto &x : h)
        if (!next_u(fp, &x)) return false;
    const mi_lte_dlsch_cfg cfg = {(uint32_t)h[1], (uint32_t)h[2]};
    std::vector<mi_lte_pdsch_alloc> allocs;
    std::vector<mi_lte_ulsch_uci>   uci;
    if (!expand(fp, false, &allocs, &uci)) return false;
    MiDlsch3Layout g;
    const char    *err = nullptr;
    const int      rc  = mi_dlsch3_layout(&cfg, allocs.data(), (uint32_t)allocs.size(), &g, &err);
    printf("rc=%d", rc);
    if (rc == MI_LTE_OK) print_g3(g, h[0] != 0);
    printf(" err=%s\n", err ? err : "");
    return true;
}

bool query_A(FILE *fp)
{
    unsigned long long h[4];
    for (auto &x : h)
        if (!next_u(fp, &x)) return false;
    Rec r;
    if (!read_rec(fp, h[3] != 0, &r)) return false;
    int         row = -7;
    uint32_t    G   = 0;
    const char *err = nullptr;
    const int   rc  = pusch_alloc_check(r.al, (uint32_t)h[0], (uint32_t)h[1], h[2] != 0, h[3] ? &r.uci : nullptr, &row, &G, &err);
    printf("rc=%d row=%d G=%u planned=%d err=%s\n", rc, rc == MI_LTE_OK ? row : -1, G, pusch_nprb_planned(r.al.N_prb, (uint32_t)h[0], h[2] != 0) ? 1 : 0, err ? err : "");
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    FILE *fp = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!fp) { printf("pusch plan driver: cannot read %s\n", argv[1]); return 1; }
    char kind[4];
    long n = 0;
    while (fscanf(fp, "%1s", kind) == 1) {
        const bool ok = kind[0] == 'P' ? query_P(fp) : kind[0] == 'D' ? query_D(fp) : kind[0] == 'A' ? query_A(fp) : false;
        if (!ok) { printf("pusch plan driver: malformed query %ld\n", n); return 1; }
        n++;
    }
    if (fp != stdin) fclose(fp);
    fprintf(stderr, "pusch plan driver: %ld queries answered\n", n);
    return 0;
}

// tools/asan/turbo_swar_driver.cc: the byte-parallel helpers of openlte_amd/csrc/turbo_swar.h against a scalar restatement of the
// reference's steps (conv_encode_soft with g = 03, and the case ladders of turbo_decode's Steps 3, 10 and 11), on the CPU under
// g++ -fsanitize=address,undefined (tools/asan/run_turbo_swar.sh).  Exhaustive where the domain allows: every (a, b) of soft_xor and
// Step 3, every (A, B, G) of Step 10, every (B, G) of Step 11, values in [-127, 127]; whole blocks with halo through the feedback
// and through the two nine-bit sums the way k_turbo_perm / k_turbo_vote walk a unit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../openlte_amd/csrc/turbo_swar.h"

using namespace turbo_swar;

namespace {

long long n_checked = 0, n_bad = 0;
void fail(const char *what, int a, int b, int c, int got, int want)
{
    if (n_bad++ < 20) std::printf("MISMATCH %s (%d, %d, %d): got %d, want %d\n", what, a, b, c, got, want);
}

// ---- the reference's steps, one value at a time
int ref_step3(int a, int f) // liblte_phy.cc:10688-10707
{
    if (a >= 0 && f >= 0) return (a + f) >> 1;
    if (a < 0 && f < 0) return (-a - f) >> 1;
    if (a >= 0 && f < 0) return -((a - f) >> 1);
    return -((-a + f) >> 1);
}
int ref_step10(int A, int B, int G) // :10778-10797: the mixed-sign branches read in_act_1 (A)
{
    if (B >= 0 && G >= 0) return (B + G) >> 1;
    if (B < 0 && G < 0) return (-B - G) >> 1;
    if (B >= 0 && G < 0) return -((A - G) >> 1);
    return -((-A + G) >> 1);
}
int ref_step11(int B, int G) // :10800-10819
{
    if (B >= 0 && G >= 0) return (B + G) >> 1;
    if (B < 0 && G < 0) return (-B - G) >> 1;
    if (B >= 0 && G < 0) return -((B - G) >> 1);
    return -((-B - G) >> 1);
}
// fb[0] = 127, fb[1 ..] = conv_encode_soft(x, constraint length 3, g = 03, no tail biting): :10096-10148
std::vector<int> ref_feedback(const std::vector<int> &x)
{
    std::vector<int> fb(x.size() + 1);
    int              s_reg[3] = {127, 127, 127};
    const int        g_array[3] = {0, 1, 1};
    fb[0] = 127;
    for (size_t i = 0; i < x.size(); i++) {
        s_reg[2] = s_reg[1];
        s_reg[1] = s_reg[0];
        s_reg[0] = x[i];
        int tmp_sum = 0, tmp_mag = 0, tmp_sign = 0;
        for (int k = 0; k < 3; k++)
            if (g_array[k] == 1) {
                if (s_reg[k] >= 0) tmp_mag += s_reg[k];
                else { tmp_mag += -s_reg[k]; tmp_sign += 1; }
                tmp_sum++;
            }
        int d = tmp_mag >> (tmp_sum - 1);
        if (tmp_sign % 2 == 1) d = -d;
        fb[i + 1] = d;
    }
    fb.pop_back();
    return fb;
}

uint32_t pack(const int (&v)[4]) { return (uint32_t)(uint8_t)v[0] | (uint32_t)(uint8_t)v[1] << 8 | (uint32_t)(uint8_t)v[2] << 16 | (uint32_t)(uint8_t)v[3] << 24; }
int      sb(uint32_t w, int k) { return (int8_t)(w >> (8 * k)); }
int      ub(uint32_t w, int k) { return (int)((w >> (8 * k)) & 0xFFu); }
int      wrap(int v) { return v > 127 ? v - 255 : v; } // keeps a group of four consecutive values inside [-127, 127]

void check_split()
{
    for (int a = -127; a <= 127; a += 4) {
        const int      v[4] = {wrap(a), wrap(a + 1), wrap(a + 2), wrap(a + 3)};
        const uint32_t w = pack(v);
        const SM4      s = split(w);
        for (int k = 0; k < 4; k++, n_checked++) {
            if (ub(s.m, k) != std::abs(v[k]) || ub(s.s, k) != (v[k] < 0 ? 0x80 : 0)) fail("split", v[k], 0, 0, ub(s.m, k) | ub(s.s, k) << 8, std::abs(v[k]));
            if (sb(to_tc(s), k) != v[k]) fail("to_tc(split)", v[k], 0, 0, sb(to_tc(s), k), v[k]);
            if (join(s) != to_joined(w)) fail("to_joined", v[k], 0, 0, (int)to_joined(w), (int)join(s));
            for (int neg = 0; neg < 2; neg++) { // the trellis kernels' write: magnitude and a 0xFF mask per negative step, no "-0"
                const uint32_t j = joined_from(s.m, neg ? 0xFFFFFFFFu : 0u);
                if (ub(j, k) != (std::abs(v[k]) | ((neg && v[k] != 0) ? 0x80 : 0))) fail("joined_from", v[k], neg, 0, ub(j, k), std::abs(v[k]));
            }
            for (int neg = 0; neg < 2; neg++)
                if (v[k] >= 0 && ub(biased((uint32_t)v[k] << (8 * k) | (LO7 & ~(0xFFu << (8 * k))), neg ? HI : 0u), k) != 128 + (neg ? -v[k] : v[k]))
                    fail("biased", v[k], neg, 0, ub(biased((uint32_t)v[k] << (8 * k), neg ? HI : 0u), k), 128 + (neg ? -v[k] : v[k]));
        }
    }
}

void check_pairs() // soft_xor, Step 3 in both forms, Step 11: every (a, b)
{
    for (int a = -127; a <= 127; a++)
        for (int b0 = -127; b0 <= 127; b0 += 4) {
            const int av[4] = {a, wrap(a + 100), a, wrap(a + 200)}, bv[4] = {b0, wrap(b0 + 1), wrap(b0 + 2), wrap(b0 + 3)};
            const SM4 A = split(pack(av)), B = split(pack(bv)), X = soft_xor(A, B);
            const uint32_t tc = to_tc(X), nb = step3_neg_biased(A, B), s11 = step11_neg_biased(A, B);
            for (int k = 0; k < 4; k++, n_checked += 3) {
                const int want = ref_step3(av[k], bv[k]);
                if (sb(tc, k) != want || ub(X.m, k) != std::abs(want) || ub(X.s, k) != (want < 0 ? 0x80 : 0)) fail("soft_xor", av[k], bv[k], 0, sb(tc, k), want);
                if (ub(nb, k) != 128 - want) fail("step3_neg_biased", av[k], bv[k], 0, ub(nb, k), 128 - want);
                if (ub(s11, k) != 128 - ref_step11(av[k], bv[k])) fail("step11", av[k], bv[k], 0, ub(s11, k), 128 - ref_step11(av[k], bv[k]));
            }
        }
}

void check_step10() // every (A, B, G): 16.6 M triples
{
    for (int a = -127; a <= 127; a++)
        for (int b = -127; b <= 127; b++) {
            const int av[4] = {a, a, wrap(a + 77), a}, bv[4] = {b, b, b, wrap(b + 131)};
            const SM4 A = split(pack(av)), B = split(pack(bv));
            for (int g0 = -127; g0 <= 127; g0 += 4) {
                const int      gv[4] = {g0, wrap(g0 + 1), wrap(g0 + 2), wrap(g0 + 3)};
                const uint32_t u = step10_biased(A, B, split(pack(gv)));
                for (int k = 0; k < 4; k++, n_checked++)
                    if (ub(u, k) != 128 + ref_step10(av[k], bv[k], gv[k])) fail("step10", av[k], bv[k], gv[k], ub(u, k) - 128, ref_step10(av[k], bv[k], gv[k]));
            }
        }
}

// ---- whole blocks the way the kernels walk them: units of 16 values = four words, the word before the unit as halo (0x7F7F7F7F in front of
// the first unit), values past the block end are whatever the array holds
uint32_t rng_state = 12345u;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
int      draw(int kind)
{
    switch (kind) {
    case 0: return (int)(rnd() % 255u) - 127;                 // full range
    case 1: return (int)(rnd() % 3u) - 1;                     // 0 and +-1: magnitude-0 results under a negative sign
    case 2: return (rnd() & 1u) ? 127 : -127;                 // saturated
    case 3: return (rnd() % 4u) ? 0 : (int)(rnd() % 5u) - 2;  // mostly 0
    default: return 0;
    }
}
void fill(std::vector<int> &v, size_t K, int kind)
{
    for (size_t i = 0; i < v.size(); i++) v[i] = i < K ? draw(kind) : draw(0); // junk past the block end must not reach a valid position
}
uint32_t word_of(const std::vector<int> &v, int w) // word w of the padded array; w = -1: the preset
{
    if (w < 0) return LO7;
    const int q[4] = {v[4 * w], v[4 * w + 1], v[4 * w + 2], v[4 * w + 3]};
    return pack(q);
}

void check_block(size_t K, int kind_a, int kind_b, int kind_c)
{
    const size_t     Kp = (K + 15) & ~(size_t)15;
    std::vector<int> A(Kp), B1(Kp), B2(Kp), X0(Kp);
    fill(A, K, kind_a); fill(B1, K, kind_b); fill(B2, K, kind_c); fill(X0, K, 0);
    const std::vector<int> va(A.begin(), A.begin() + K), vb(B1.begin(), B1.begin() + K), vc(B2.begin(), B2.begin() + K);
    const std::vector<int> fa = ref_feedback(va), fb = ref_feedback(vb), fc = ref_feedback(vc);
    for (size_t u = 0; u < Kp / 16; u++) {
        uint32_t pa = to_joined(word_of(A, (int)(4 * u) - 1)), pb = to_joined(word_of(B1, (int)(4 * u) - 1)), pc = to_joined(word_of(B2, (int)(4 * u) - 1));
        for (int j = 0; j < 4; j++) {
            const int w = (int)(4 * u) + j;
            const uint32_t ja = to_joined(word_of(A, w)), jb = to_joined(word_of(B1, w)), jc = to_joined(word_of(B2, w));
            const SM4 a = unjoin(ja), b = unjoin(jb), c = unjoin(jc);
            const SM4 F = feedback(ja, pa), G = feedback(jb, pb), H = feedback(jc, pc);
            pa = ja; pb = jb; pc = jc;
            const uint32_t c1 = to_tc(step3(a, F)), nb = step3_neg_biased(a, F), u1 = step10_biased(a, b, G), n2 = step11_neg_biased(c, H);
            const uint32_t x0b = word_of(X0, w) ^ HI;
            const uint32_t s0e = sub_halves(even_halves(x0b), even_halves(nb)), s0o = sub_halves(odd_halves(x0b), odd_halves(nb));
            const uint32_t de = sub_halves(even_halves(u1), even_halves(n2)), dd = sub_halves(odd_halves(u1), odd_halves(n2));
            for (int k = 0; k < 4; k++) {
                const size_t i = 4 * (size_t)w + k;
                if (i >= K) continue;
                n_checked += 4;
                const int fgot = (ub(F.s, k) ? -1 : 1) * ub(F.m, k);
                if (fgot != fa[i] || (ub(F.m, k) == 0 && ub(F.s, k))) fail("feedback", (int)i, (int)K, kind_a, fgot, fa[i]);
                const int c1w = ref_step3(A[i], fa[i]);
                if (sb(c1, k) != c1w) fail("C1", (int)i, (int)K, kind_a, sb(c1, k), c1w);
                const int s0 = (int16_t)(((k & 1) ? s0o : s0e) >> (16 * (k >> 1)));
                if (s0 != X0[i] + c1w) fail("q(d0) + C1", (int)i, (int)K, kind_a, s0, X0[i] + c1w);
                const int d = (int16_t)(((k & 1) ? dd : de) >> (16 * (k >> 1))), dw = ref_step10(A[i], B1[i], fb[i]) + ref_step11(B2[i], fc[i]);
                if (d != dw) fail("D1 + D2", (int)i, (int)K, kind_b * 10 + kind_c, d, dw);
            }
        }
    }
}

} // namespace

int main()
{
    check_split();
    check_pairs();
    check_step10();
    const size_t sizes[] = {40, 104, 16, 8, 1088, 6144}; // 40, 104, 8: a last unit of eight valid values
    for (size_t K : sizes)
        for (int ka = 0; ka < 5; ka++)
            for (int kb = 0; kb < 5; kb++)
                for (int rep = 0; rep < (K < 200 ? 20 : 2); rep++) check_block(K, ka, kb, (ka + kb + rep) % 5);
    std::printf("turbo swar driver: %lld values checked, %lld mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}

// DCI formats 0 / 1A / 1C as bit fields (36.212 5.3.3.1): one field list per format that the packers (tx_ctrl.cc, pdcch_synth.cc) and the unpackers
// (dci.cc) both read, the resource indication value of 36.213 7.1.6.3 / 8.1.1, and the payload sizes.  Host arithmetic in plain C++: no HIP, no context.
#pragma once
#include <cmath>
#include <cstdint>

namespace dci {

// width of the RIV field of a contiguous allocation, the logarithms in float as the reference takes them (dci_1a_pack, liblte_phy.cc:13138)
inline uint32_t riv_bits(uint32_t N_rb) { return (uint32_t)ceilf(logf(N_rb * (N_rb + 1) / 2) / logf(2)); }
inline uint32_t riv_encode(uint32_t N_rb, uint32_t N_prb, uint32_t first)
{
    return (N_prb - 1) <= N_rb / 2 ? N_rb * (N_prb - 1) + first : N_rb * (N_rb - N_prb + 1) + (N_rb - 1 - first);
}
// the whole range of the field: false past N_rb (N_rb + 1) / 2 - 1 (inside that range the two branches are one-to-one); what no branch
// reaches is left as it was
inline bool riv_decode(uint32_t N_rb, uint32_t riv, uint32_t *N_prb, uint32_t *first)
{
    const uint32_t q = riv / N_rb, r = riv % N_rb;
    const bool     ok = riv < N_rb * (N_rb + 1) / 2;
    if (q + r < N_rb) { *N_prb = q + 1; *first = r; }
    else if (ok) { *N_prb = N_rb - q + 1; *first = N_rb - 1 - r; }
    return ok;
}
// SI-, P- and RA-RNTI: format 1A carries N_PRB^1A in the TPC field's place for them (36.212 5.3.3.1.3)
inline bool common_rnti(uint32_t rnti) { return rnti == 0xFFFFu || rnti == 0xFFFEu || (rnti >= 1 && rnti <= 0x3Cu); }
// 36.212 5.3.3.1.2: payload sizes that are ambiguous get one more bit
inline bool ambiguous_size(uint32_t n) { return n == 12 || n == 14 || n == 16 || n == 20 || n == 24 || n == 26 || n == 32 || n == 40 || n == 44 || n == 56; }
// the sizes of formats 1A and 1C the reference's receiver decodes with, by bandwidth (liblte_phy.cc:4835-4857)
inline void sizes(uint32_t N_rb_dl, uint32_t *s1a, uint32_t *s1c)
{
    switch (N_rb_dl) {
    case 6:  *s1a = 21; *s1c = 9;  break;
    case 15: *s1a = 22; *s1c = 11; break;
    case 25: *s1a = 25; *s1c = 13; break;
    case 50: *s1a = 27; *s1c = 13; break;
    case 75: *s1a = 27; *s1c = 14; break;
    default: *s1a = 28; *s1c = 15; break;
    }
}

// every field of the three formats; flag: localized / distributed (1A), hopping (0); gap: N_gap,1 / N_gap,2 (1C)
struct Fields { uint32_t format, flag, gap, riv, mcs, harq, ndi, rv, tpc, cyclic_shift, cqi_request; };
struct Field { uint32_t Fields::*at; uint32_t bits; };
constexpr uint32_t RIV = 0xFFu, GAP = 0xFEu; // widths that depend on the bandwidth: the caller gives them
constexpr Field FORMAT_1A[] = {{&Fields::format, 1}, {&Fields::flag, 1}, {&Fields::riv, RIV}, {&Fields::mcs, 5}, {&Fields::harq, 3}, {&Fields::ndi, 1}, {&Fields::rv, 2}, {&Fields::tpc, 2}};
constexpr Field FORMAT_0[]  = {{&Fields::format, 1}, {&Fields::flag, 1}, {&Fields::riv, RIV}, {&Fields::mcs, 5}, {&Fields::ndi, 1}, {&Fields::tpc, 2}, {&Fields::cyclic_shift, 3}, {&Fields::cqi_request, 1}};
constexpr Field FORMAT_1C[] = {{&Fields::gap, GAP}, {&Fields::riv, RIV}, {&Fields::mcs, 5}};

// (pack and unpack are inlined by force: with the list a constant the loop folds to the shifts one would write by hand, which
// mi_lte_pdcch_decode_run's per-DCI unpacking is timed by)
#define DCI_INLINE inline __attribute__((always_inline))
DCI_INLINE uint32_t width(const Field &f, uint32_t riv_len, uint32_t gap_len) { return f.bits == RIV ? riv_len : f.bits == GAP ? gap_len : f.bits; }
// the first field of formats 0 / 1A on its own: which of the two the payload is
inline uint32_t format_flag(uint64_t payload, uint32_t n_bits) { return (uint32_t)((payload >> (n_bits ? n_bits - 1 : 0)) & 1u); }
template <uint32_t N>
inline uint32_t total_bits(const Field (&list)[N], uint32_t riv_len, uint32_t gap_len = 0)
{
    uint32_t n = 0;
    for (const Field &f : list) n += width(f, riv_len, gap_len);
    return n;
}
// the fields in order, the first in the most significant of the total_bits() bits of *payload (each cut to its width); returns that count
template <uint32_t N>
DCI_INLINE uint32_t pack(const Field (&list)[N], const Fields &v, uint32_t riv_len, uint64_t *payload, uint32_t gap_len = 0)
{
    uint32_t n = 0;
    *payload = 0;
    for (const Field &f : list) {
        const uint32_t w = width(f, riv_len, gap_len);
        *payload = (*payload << w) | (v.*f.at & ((1ull << w) - 1ull));
        n += w;
    }
    return n;
}
// the reverse for a payload whose first bit is bit n_bits - 1 (n_bits <= 64); a field that reaches past the last bit reads from bit 0 up, as
// the reference's unpackers leave it
template <uint32_t N>
DCI_INLINE Fields unpack(const Field (&list)[N], uint64_t payload, uint32_t n_bits, uint32_t riv_len, uint32_t gap_len = 0)
{
    Fields   v{};
    uint32_t pos = n_bits;
    for (const Field &f : list) {
        const uint32_t w = width(f, riv_len, gap_len);
        if (w == 0) continue;
        pos = pos >= w ? pos - w : 0;
        v.*f.at = (uint32_t)((payload >> pos) & ((1ull << w) - 1ull));
    }
    return v;
}

} // namespace dci

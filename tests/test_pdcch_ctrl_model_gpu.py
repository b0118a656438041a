"""GPU: the first stage of the blind PDCCH search -- PCFICH decision, the table of every CCE's resource elements, the 1-, 2- and 4-port
combiner, the QPSK soft value and the descrambler (k_pdcch_search_demod; include/mi_lte.h, "PDCCH, 3GPP mode", step 1) -- against the float64
model and the independent 36.211 modulator of pdcch_ctrl_model.  Nothing here uses the library's own transmitter."""
import numpy as np
import pytest

import pdcch_ctrl_cases as pc
import pdcch_ctrl_model as pm
from test_pdcch_search_cpu import space

pytestmark = pytest.mark.gpu

CAP_SHARE = 0.01  # of a case's bits may be close calls: a condition on the inputs, like the half that must be unsaturated
CASE_IDX = list(range(len(pc.CASES)))
SIZES = (27, 41)


def run(ctx, n_rb, n_ant, n_g, cells, sfs, grid_sets, rntis=(), regs_36211=False):
    """One plan, one run per entry of grid_sets (same units, other data): per run (h_cfi, h_n_cce, n_found, found, soft [n, stride])"""
    import openlte_amd as m
    cfg = m.DlCfg(pc.FFT[n_rb], n_rb, n_ant, 0)
    plan = ctx.pdcch_search_plan(cfg, sorted(set(cells)), SIZES, rntis, phich_res=float(pm.N_G[n_g]), regs_36211=regs_36211)
    d_sf, d_cell = ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))
    out = []
    try:
        for g in grid_sets:
            d_g = ctx.to_device(np.ascontiguousarray(g, np.float32))
            try:
                out.append(plan.search_dev(d_g, d_sf, d_cell, len(sfs)) + (plan.soft(len(sfs)),))
            finally:
                d_g.free()
    finally:
        d_sf.free()
        d_cell.free()
        plan.close()
    return out


def run_case(ctx, i, kinds, numbering="library"):
    n_rb, n_ant, n_g, units = pc.ALL[i]
    return run(ctx, n_rb, n_ant, n_g, [u[0] for u in units], [u[1] for u in units], [pc.batch(i, k, numbering)[0] for k in kinds], regs_36211=numbering == "36.211")


def check_soft(got, want):
    """a unit's soft bits against decode()'s dict: equal but for close calls; returns the number of close calls"""
    assert (np.abs(got) <= 127).all()
    n_close, bad = pm.compare(got, want)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want["soft"][bad[:8]])
    return n_close


# ---- geometry of every CCE

@pytest.mark.parametrize("i", CASE_IDX, ids=pc.IDS)
def test_every_cce_lies_where_36211_puts_it(ctx, i):
    """Noiseless, random bits on every CCE, true estimates.  A first run on other data over the largest region fills the plan's soft buffer;
    the second run must leave everything past its own 72 N_cce as the first wrote it."""
    (_, f_n_cce, _, _, f_soft), (h_cfi, h_n_cce, n_found, _, soft) = run_case(ctx, i, ("filler", "clean"))
    _, bits = pc.batch(i, "clean")
    want = pc.reference(i, "clean")
    assert h_cfi.tolist() == [w["cfi"] for w in want] == [u[2] for u in pc.CASES[i][3]]
    assert h_n_cce.tolist() == [w["n_cce"] for w in want]
    assert n_found.tolist() == [0] * len(want)
    assert (f_n_cce > h_n_cce).any() and soft.shape == f_soft.shape
    for u, w in enumerate(want):
        n = 72 * w["n_cce"]
        got = soft[u, :n].astype(np.int64)
        assert (np.sign(got) == 1 - 2 * bits[u].reshape(-1).astype(np.int64)).all(), (u, np.flatnonzero(np.sign(got) != 1 - 2 * bits[u].reshape(-1).astype(np.int64))[:8])
        assert (np.abs(got) >= np.abs(w["soft"]) - 1).all()
        assert (soft[u, n:] == f_soft[u, n:]).all()
        assert f_n_cce[u] <= h_n_cce[u] or (f_soft[u, n:72 * int(f_n_cce[u])] != 0).all()  # (the tail held the first run's values, not zeros)


# ---- soft values

@pytest.mark.parametrize("i", CASE_IDX, ids=pc.IDS)
def test_soft_values_at_10_db_equal_the_float64_decoder(ctx, i):
    (h_cfi, h_n_cce, _, _, soft), = run_case(ctx, i, ("noisy",))
    want = pc.reference(i, "noisy")
    assert h_cfi.tolist() == [w["cfi"] for w in want]  # (also where the PCFICH fails or decides on another value)
    assert h_n_cce.tolist() == [w["n_cce"] for w in want]
    n_bits = n_close = n_sat = 0
    for u, w in enumerate(want):
        if not w["n_cce"]:
            continue
        got = soft[u, :72 * w["n_cce"]].astype(np.int64)
        n_close += check_soft(got, w)
        n_sat += int((np.abs(got) == 1).sum())
        n_bits += len(got)
    print("%s: %d bits, %d close calls, %d saturated" % (pc.IDS[i], n_bits, n_close, n_sat))
    assert n_bits > 0 and n_close <= CAP_SHARE * n_bits and n_bits - n_sat >= 0.5 * n_bits


def test_saturated_floor_at_minus_3_db(ctx):
    """-3 dB: much of the region lies a whole unit from its quadrant's point and reads magnitude 1 with the quadrant's and the descrambler's signs"""
    i = pc.IDS.index("25-2-1_6")
    (h_cfi, h_n_cce, _, _, soft), = run_case(ctx, i, ("low",))
    want = pc.reference(i, "low")
    assert h_cfi.tolist() == [w["cfi"] for w in want] and h_n_cce.tolist() == [w["n_cce"] for w in want]
    n_bits = n_sat = n_close = 0
    for u, w in enumerate(want):
        if not w["n_cce"]:
            continue
        got = soft[u, :72 * w["n_cce"]].astype(np.int64)
        n_close += check_soft(got, w)
        sat = w["sat"] & ~w["close_sym"]
        assert (np.abs(got[sat]) == 1).all() and (got[sat] == w["soft"][sat]).all()
        n_sat += int(sat.sum())
        n_bits += len(got)
    assert n_bits > 0 and n_sat >= 0.2 * n_bits and n_close <= CAP_SHARE * n_bits


# ---- MI_LTE_PDCCH_SEARCH_36211_REGS

@pytest.mark.parametrize("i", pc.IDX_36211, ids=pc.IDS_36211)
def test_positions_of_36211_with_the_flag(ctx, i):
    """cells whose default tables are not 36.211's (a PHICH group numbered past a wrapped PCFICH group; four ports and one symbol), sent
    by the model at 36.211's positions: with the flag every CCE is where it was sent, and the soft values are the float64 decoder's"""
    (h_cfi, h_n_cce, _, _, soft), (n_cfi, n_n_cce, _, _, n_soft) = run_case(ctx, i, ("clean", "noisy"), "36.211")
    _, bits = pc.batch(i, "clean", "36.211")
    want, n_want = pc.reference(i, "clean", numbering="36.211"), pc.reference(i, "noisy", numbering="36.211")
    assert h_cfi.tolist() == [w["cfi"] for w in want] == [u[2] for u in pc.ALL[i][3]] and h_n_cce.tolist() == [w["n_cce"] for w in want]
    assert n_cfi.tolist() == [w["cfi"] for w in n_want] and n_n_cce.tolist() == [w["n_cce"] for w in n_want]
    n_bits = n_close = 0
    for u, (w, nw) in enumerate(zip(want, n_want)):
        got = soft[u, :72 * w["n_cce"]].astype(np.int64)
        assert (np.sign(got) == 1 - 2 * bits[u].reshape(-1).astype(np.int64)).all()
        assert (np.abs(got) >= np.abs(w["soft"]) - 1).all()
        if nw["n_cce"]:
            n_close += check_soft(n_soft[u, :72 * nw["n_cce"]].astype(np.int64), nw)
            n_bits += 72 * nw["n_cce"]
    assert n_bits > 0 and n_close <= CAP_SHARE * n_bits


# ---- edges

@pytest.mark.parametrize("n_ant", [1, 2, 4])
def test_zero_estimates_and_a_huge_sample(ctx, n_ant):
    """what the header says of a non-finite combiner output and of a sample far outside the constellation"""
    n_rb, n_g, cfi = 25, "1", 3
    cells, sfs = [44, 13, 302], [0, 9, 5]
    rng = np.random.default_rng(50 + n_ant)
    n_cce = [pc.n_cce_of(n_rb, n_ant, n_g, c, cfi) for c in cells]
    # unit 1: port 1 in total fade, its estimate plane zero (2 and 4 ports)
    g = np.stack([pm.modulate(n_rb, n_ant, c, s, cfi, pm.N_G[n_g], rng.integers(0, 2, (n, 72)).astype(np.uint8), rng, snr_db=10.0,
                              dead_port=1 if (u == 1 and n_ant > 1) else None) for u, (c, s, n) in enumerate(zip(cells, sfs, n_cce))])
    flat = g.reshape(3, 2 + 2 * n_ant, -1)
    # unit 0: the estimates of one resource-element group (CCE 1, quadruplet 3) are zero on every port
    re0 = pm.geometry(n_rb, n_ant, cells[0], pm.N_G[n_g], cfi)[1][1, 12:16]
    flat[0, 2:, re0] = 0.0
    hit0 = 72 + 2 * 12 + np.arange(8)
    # unit 2: one received sample is 1e30 (CCE 2, element 5)
    assert n_ant == 1 or not (flat[1, 3].any() or flat[1, 2 + n_ant + 1].any())
    re2 = pm.geometry(n_rb, n_ant, cells[2], pm.N_G[n_g], cfi)[1][2, 5]
    flat[2, 0, re2] = 1e30
    hit2 = 2 * 72 + 2 * (np.array([5]) if n_ant == 1 else np.array([4, 5]))
    hit2 = np.concatenate([hit2, hit2 + 1])
    (h_cfi, h_n_cce, n_found, found, soft), = run(ctx, n_rb, n_ant, n_g, cells, sfs, [g])
    assert h_cfi.tolist() == [cfi] * 3 and h_n_cce.tolist() == n_cce
    assert n_found.tolist() == [0, 0, 0] and found == [[], [], []]  # no error, and an empty RNTI set: no hit
    want = [pm.decode(n_rb, n_ant, c, s, pm.N_G[n_g], g[u]) for u, (c, s) in enumerate(zip(cells, sfs))]
    for u, w in enumerate(want):
        got = soft[u, :72 * n_cce[u]].astype(np.int64)
        check_soft(got, w)  # every element, the affected ones included: the model restates the header
        if u == 0:
            assert (got[hit0] == 0).all() and (np.delete(got, hit0) != 0).all()
        if u == 2:
            assert (np.abs(got[hit2]) == 1).all()
        if u == 1 and n_ant == 4:  # ports (1, 3) on elements 2, 3 of every group: port 3 alone still decodes them
            assert (got != 0).all()


# ---- end to end, the model's transmitter

LAYOUT = {20: [(8, 8), (4, 16), (2, 0), (1, 3), (1, 6)], 17: [(8, 8), (1, 16), (4, 0), (2, 4), (1, 7)],
          73: [(8, 64), (8, 16), (4, 32), (2, 60), (1, 72), (1, 40), (2, 0)]}


def rnti_for(rng, sf, n_cce, L, cce, taken):
    for _ in range(20000):
        r = int(rng.integers(0x3D, 0xFFF4))
        if r not in taken and (cce in space(r, sf, n_cce, L) or (L >= 4 and cce < 16)):
            return r
    raise AssertionError("no RNTI with a candidate at CCE %d, L = %d" % (cce, L))


@pytest.mark.parametrize("n_rb,n_ant", [(25, 1), (25, 2), (25, 4), (100, 4)])
def test_every_record_of_the_model_transmitter_is_found(ctx, n_rb, n_ant):
    n_g, cfi = "1", 3
    cells, sfs = [49, 302, 13], [0, 9, 4]
    rng = np.random.default_rng(10 * n_rb + n_ant)
    recs, unlisted, grids, taken = [], [], [], set()
    for cell, sf in zip(cells, sfs):
        n_cce = pc.n_cce_of(n_rb, n_ant, n_g, cell, cfi)
        lst = []
        for L, cce in LAYOUT[n_cce]:
            size = SIZES[len(lst) % 2]
            r = rnti_for(rng, sf, n_cce, L, cce, taken)
            taken.add(r)
            lst.append((r, L, cce, size, int(rng.integers(0, 1 << 62)) & ((1 << size) - 1)))
        recs.append(lst[:-1])
        unlisted.append(lst[-1])  # sent like the others, its RNTI not in the set
        grids.append(pm.modulate(n_rb, n_ant, cell, sf, cfi, pm.N_G[n_g], pm.place_dcis(n_cce, lst), rng, snr_db=30.0))
    assert {r[1] for lst in recs for r in lst} == {1, 2, 4, 8} and max(r[2] for lst in recs for r in lst) >= 16
    listed = sorted(r[0] for lst in recs for r in lst)
    (h_cfi, h_n_cce, n_found, found, _), = run(ctx, n_rb, n_ant, n_g, cells, sfs, [np.stack(grids)], listed)
    assert h_cfi.tolist() == [cfi] * 3
    for u in range(3):
        got = {t[:5] for t in found[u]}
        assert int(n_found[u]) <= 16 and len(found[u]) == int(n_found[u])
        for r in recs[u]:
            assert r in got, (u, r, sorted(got))
        assert {t[0] for t in found[u]} <= {r[0] for r in recs[u]}  # nothing for another unit's RNTI, nothing for the unlisted one
        assert unlisted[u][0] not in {t[0] for t in found[u]}

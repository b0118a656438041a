"""CPU: what tests/test_demap_geometry_gpu.py stands on.  The model's resource-element extraction (demap_llr_model.pdsch_res) counts what
fuzz_cases.re_count counts (which tests/test_fuzz_cpu.py pins to the reference's loop) around every window edge and band edge of all six
bandwidths; on two and four ports every (symbol, PRB) group is even, so a transmit-diversity pair never leaves its pair-table entry; and the
draw of tests/demap_geometry_cases.py delivers the kinds, modulations, CRS shifts and store paths it promises, on planes that keep the model's
guard band under the 1 % that test_demap_llr_gpu.check_against_model allows.  No GPU."""
import numpy as np
import pytest

import demap_geometry_cases as gc
import demap_llr_model as dm
from fuzz_cases import re_count


def single(p0, p1, cfi):
    import openlte_amd as m
    return m.make_alloc(0, 1, 16, [p0], 0x11, prbs_slot1=[p1], n_pdcch_symbs=cfi)


def test_pdsch_res_counts_what_re_count_counts():
    """Six bandwidths x 1 / 2 / 4 ports x cells 0 .. 5 x subframes 0 / 5 / 3 x control regions 1 .. 4 x every PRB within one of the window and
    both band edges x slot 1 on the same PRB and on another: 25 488 single-PRB allocations, len(pdsch_res) == re_count, and on two and four
    ports a multiple of the port count (M_symb's truncation drops nothing)."""
    n = 0
    for n_rb in gc.N_RBS:
        fp, lp = gc.window_prbs(n_rb)
        prbs = sorted({0, n_rb - 1} | set(range(max(0, fp - 1), min(n_rb, lp + 2))))
        for cfi in (1, 2, 3, 4):
            for k, p0 in enumerate(prbs):
                for p1 in (p0, prbs[(k + len(prbs) // 2) % len(prbs)]):
                    al = single(p0, p1, cfi)
                    for n_ant in (1, 2, 4):
                        for cell in range(6):
                            for sf in (0, 5, 3):
                                got = len(dm.pdsch_res(al, sf, cell, n_rb, 1, n_ant))
                                assert got == re_count(n_rb, n_ant, cell, sf, cfi, [p0], [p1]), (n_rb, n_ant, cell, sf, cfi, p0, p1)
                                assert got % n_ant == 0, (n_rb, n_ant, cell, sf, cfi, p0, p1)
                                n += 1
    assert n == 25488


def test_every_txdiv_table_entry_is_even():
    """Two and four ports, every PRB of every bandwidth, cells 0 .. 2, subframes 0 / 5 / 3, the widest data region: every (symbol, PRB) group of
    pdsch_res -- one entry of the kernel's pair table -- holds an even number of resource elements (4, 6, 8 or 12), and every allocation's total is
    a multiple of the port count.  What follows: every entry starts at an even RE index, the other element of a transmit-diversity pair (index
    i ^ 1) lies in the same entry, and no pair ever leaves its table entry -- across PRBs, symbols or the window.  The table search
    (`locate`) in k_pdsch_demod_llr is therefore a fallback that no valid geometry reaches."""
    sizes, n_groups = set(), 0
    for n_rb in gc.N_RBS:
        for p in range(n_rb):
            al = single(p, p, 1)
            for n_ant in (2, 4):
                for cell in range(3):
                    for sf in (0, 5, 3):
                        pos = dm.pdsch_res(al, sf, cell, n_rb, 1, n_ant)
                        assert len(pos) % n_ant == 0, (n_rb, p, n_ant, cell, sf)
                        _, counts = np.unique(pos // dm.N_SC, return_counts=True)  # (one PRB: a group per symbol)
                        assert not (counts % 2).any(), (n_rb, p, n_ant, cell, sf, counts)
                        sizes |= set(int(c) for c in counts)
                        n_groups += len(counts)
    print("%d non-empty (symbol, PRB) groups, sizes %s" % (n_groups, sorted(sizes)))
    assert sizes == {4, 6, 8, 12} and n_groups == 61830


@pytest.fixture(scope="module")
def draws():
    return {p: gc.draw(*p) for p in gc.PARAMS}


def test_parameter_sets():
    small = [p for p in gc.PARAMS if p[2] == "small"]
    assert sorted(p[:2] for p in small) == sorted((n_rb, n_ant) for n_rb in (6, 15, 25, 50, 75, 100) for n_ant in (1, 2, 4))
    assert sorted(p[:3] for p in gc.PARAMS if p[2] != "small") == sorted((n_rb, n_ant, v) for n_rb in (75, 100) for n_ant in (1, 2, 4)
                                                                          for v in ("lds_max", "direct_min"))
    assert len(gc.PARAMS) == 30 and len({p[3] for p in gc.PARAMS}) == 30


def test_the_draw_keeps_its_promises(draws):
    """Every parameter set: subframes 0, 5 and another; the CRS shifts; four allocations per unit; every kind (the one-slot-in-window set where
    the band is wider than the window) and every modulation; a run over each edge of the window and a one-slot-in-window set in subframes
    0 / 5; control regions within 1 .. 3 (4 at 6 RB, and used there); no empty allocation; the largest allocation on its side of 32 KiB."""
    one_port_residues = set()
    for (n_rb, n_ant, variant, seed), (cfi, sfs, cells, allocs, planes) in draws.items():
        tag = (n_rb, n_ant, variant)
        assert sfs[:2] == [0, 5] and sfs[2] not in (0, 5) and 0 <= sfs[2] <= 9 and 1 <= cfi <= 3
        assert all(0 <= c < 504 for c in cells)
        if n_ant == 1:
            assert len({c % 6 for c in cells}) == 3, tag
            if variant == "small":
                one_port_residues |= {c % 6 for c in cells}
        else:
            assert {c % 3 for c in cells} == {0, 1, 2}, tag
        assert planes.shape == (3, 2 + 2 * n_ant, 16, dm.N_SC) and planes.dtype == np.float32 and np.isfinite(planes).all()
        h = planes[:, 2:2 + n_ant] + 1j * planes[:, 2 + n_ant:]
        assert all(np.abs(h[u, a] - h[u, b]).min() > 0 for u in range(3) for a in range(n_ant) for b in range(a))  # (h_pa != h_pb everywhere)
        small = [al for al in allocs if al.N_prb <= 8]
        assert len(small) == 12 and [sum(al.unit == u for al in small) for u in range(3)] == [4, 4, 4], tag
        assert {al.mod_type for al in small} == {1, 2, 3} and all(al.tx_mode == (1 if n_ant == 1 else 2) for al in allocs), tag
        assert all(0 <= al.n_pdcch_symbs <= (4 if n_rb == 6 else 3) for al in allocs) and (n_rb != 6 or any(al.n_pdcch_symbs == 4 for al in allocs)), tag
        kinds = set().union(*(gc.kinds_of(al, n_rb) for al in small))
        assert kinds >= set(gc.KINDS) - ({"one_slot_in_window"} if n_rb == 6 else set()), (tag, kinds)
        fp, lp = gc.window_prbs(n_rb)
        win = [al for al in small if sfs[al.unit] in (0, 5)]
        if n_rb > 6:
            runs = [gc.prb_lists(al)[0] for al in win if "run" in gc.kinds_of(al, n_rb)]
            assert any(fp - 1 in r and fp in r for r in runs) and any(lp in r and lp + 1 in r for r in runs), (tag, runs)
            assert any("one_slot_in_window" in gc.kinds_of(al, n_rb) for al in win), tag
        for al in allocs:
            p0, p1 = gc.prb_lists(al)
            assert all(0 <= p < n_rb for p in p0 + p1) and len(set(p0)) == len(p0) and len(set(p1)) == len(p1)
            n_re = re_count(n_rb, n_ant, cells[al.unit], sfs[al.unit], al.n_pdcch_symbs or cfi, p0, p1)
            assert n_re >= n_ant and n_re == len(dm.pdsch_res(al, sfs[al.unit], cells[al.unit], n_rb, cfi, n_ant)), (tag, p0, p1)
        e_bytes = gc.plan_e_bytes(allocs, cfi)
        if variant == "small":
            assert len(allocs) == 12 and e_bytes <= 13 * 8 * 72 + 63
        else:
            big = [al for al in allocs if al.N_prb > 8]
            assert len(allocs) == 13 and len(big) == 1 and big[0].N_prb == gc.BIG_PRB[variant] and big[0].mod_type == 2 and big[0].n_pdcch_symbs == 2
            p0, p1 = gc.prb_lists(big[0])
            assert p0 == p1 == list(range(p0[0], p0[0] + big[0].N_prb))
            assert e_bytes == {"lds_max": 32256, "direct_min": 32832}[variant] and (e_bytes <= 32768) == (variant == "lds_max")
    assert one_port_residues == set(range(6))


def test_the_draw_is_reproducible():
    p = gc.PARAMS[4]
    a, b = gc.draw(*p), gc.draw(*p)
    assert a[:3] == b[:3] and (a[4] == b[4]).all()
    assert [bytes(x) for x in a[3]] == [bytes(x) for x in b[3]]


def test_guard_band_of_the_drawn_planes(draws):
    """The model alone over every parameter set, automatic gain and the GPU test's fixed one: under 1 % of the soft bits within the guard band
    (a condition on the inputs: the cap is check_against_model's), and clamped and graded bytes both occur."""
    import openlte_amd as m
    for (n_rb, n_ant, variant, seed), drawn in draws.items():
        auto = gc.model_of(drawn, n_rb, n_ant, 0.0, m.DEMAP_AUTO_T)
        fixed = float(np.float32(1.5 * np.median([r.gain for r in auto])))
        for res in (auto, gc.model_of(drawn, n_rb, n_ant, fixed, m.DEMAP_AUTO_T)):
            x, e = np.concatenate([r.x for r in res]), np.concatenate([r.bytes for r in res])
            frac = dm.in_guard(x).mean()
            print("%d RB, %d ports, %s: %d soft bits, %.3f %% in the guard band" % (n_rb, n_ant, variant, len(x), 100 * frac))
            assert all(len(r.bytes) > 0 and r.gain > 0 for r in res)
            assert frac < 0.01, (n_rb, n_ant, variant, frac)
            assert (np.abs(e) == 127).any() and (np.abs(e) < 127).any()

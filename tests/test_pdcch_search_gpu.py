"""GPU: the blind PDCCH search (include/mi_lte.h: "PDCCH, 3GPP mode") against a numpy model of the header's text.

From the de-mapper on everything is integer work, so given the tapped int8 soft bits the model reproduces the whole result -- rate
un-matching, the tail-biting decoder with its tie rules, CRC16, the search-space rule, the order and the cap -- and h_n_found and every
field of every record must be equal, metric and energy included, also where what is decoded is noise."""
import numpy as np
import pytest

from test_pdcch_search_cpu import DCI_1A_BITS, space
from test_ulsch_cqi_cpu import conv_tb, rm_index, viterbi3

pytestmark = pytest.mark.gpu

MAX_FOUND = 16
FFT = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 2048, 100: 2048}


# ---- the model

def candidates(n_cce):
    """(L, first CCE) in reporting order"""
    return [(L, c) for L in (8, 4, 2, 1) for c in range(0, n_cce - L + 1, L)]


def crc16_syndrome(c, n_bits):
    """c [n, n_bits + 16] decided bits -> the CRC16 remainder of the information bits XOR the received parity, per row"""
    rem = np.zeros(len(c), np.int64)
    for t in range(n_bits + 16):
        rem = (rem << 1) | (c[:, t] if t < n_bits else 0)
        rem = np.where(rem & 0x10000, rem ^ 0x11021, rem)
    par = np.zeros(len(c), np.int64)
    for t in range(16):
        par = (par << 1) | c[:, n_bits + t]
    return (rem ^ par) & 0xFFFF


_RM = {}


def rm(N, E):
    if (N, E) not in _RM:
        _RM[(N, E)] = rm_index(N, E)
    return _RM[(N, E)]


def model(soft, n_cce, sfs, sizes, listed, any_cce):
    """soft int8 [n, stride]; listed: bool [65536] -> (n_found [n], per unit the first MAX_FOUND records as the binding's tuples)"""
    n = len(soft)
    hits = [dict() for _ in range(n)]  # (candidate index, size index) -> record
    for si, n_bits in enumerate(sizes):
        N = n_bits + 16
        rows, d = [], []
        for u in range(n):
            for ci, (L, cce) in enumerate(candidates(int(n_cce[u]))):
                if N >= 72 * L:
                    continue  # no redundancy left
                e = soft[u, 72 * cce:72 * (cce + L)].astype(np.int64)
                du = np.zeros(3 * N, np.int64)
                np.add.at(du, rm(N, 72 * L), e)
                if np.abs(du).sum() == 0:
                    continue  # an empty region
                rows.append((u, ci, L, cce))
                d.append(du)
        if not rows:
            continue
        d = np.stack(d)
        c = viterbi3(d)
        metric = ((1 - 2 * conv_tb(c)) * d).sum(axis=1)
        energy = np.abs(d).sum(axis=1)
        x = crc16_syndrome(c, n_bits)
        for k, (u, ci, L, cce) in enumerate(rows):
            xk = int(x[k])
            if xk == 0 or not listed[xk]:
                continue
            if not (any_cce or (L >= 4 and cce in (0, 4, 8, 12) and cce % L == 0) or cce in space(xk, int(sfs[u]), int(n_cce[u]), L)):
                continue
            payload = 0
            for b in c[k, :n_bits]:
                payload = (payload << 1) | int(b)
            hits[u][(ci, si)] = (xk, L, cce, n_bits, payload, int(metric[k]), int(energy[k]))
    return np.array([len(h) for h in hits]), [[h[k] for k in sorted(h)][:MAX_FOUND] for h in hits]


def bitmap(rntis):
    b = np.zeros(65536, bool)
    b[np.asarray(rntis, np.int64)] = True
    return b


class Dev:
    """grids and unit arrays on the device"""

    def __init__(self, ctx, grids, sfs, cells):
        self.n = len(sfs)
        self.bufs = [ctx.to_device(np.ascontiguousarray(grids, np.float32)), ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))]

    def run(self, plan):
        return plan.search_dev(self.bufs[0], self.bufs[1], self.bufs[2], self.n)

    def free(self):
        for b in self.bufs:
            b.free()


def random_records(rng, n_cce, sf, sizes, n_rec, rntis=None):
    """n_rec non-overlapping DCIs of random C-RNTIs, each on one of its RNTI's own candidates (any L whose code rate leaves redundancy)"""
    used, recs = set(), []
    for _ in range(200):
        if len(recs) == n_rec:
            break
        rnti = int(rng.integers(0x3D, 0xFFF4)) if rntis is None else int(rng.choice(rntis))
        n_bits = int(rng.choice(sizes))
        L = int(rng.choice([L for L in (1, 2, 4, 8) if n_bits + 16 <= 0.82 * 72 * L]))
        sp = space(rnti, sf, n_cce, L)
        if not sp:
            continue
        cce = int(rng.choice(sp))
        if used & set(range(cce, cce + L)) or rnti in [r[0] for r in recs]:
            continue
        used |= set(range(cce, cce + L))
        recs.append((rnti, L, cce, n_bits, int(rng.integers(0, 1 << 62)) & ((1 << n_bits) - 1)))
    return recs


def n_cce_of(n_rb, n_ant, cfi):
    import openlte_amd as m
    return m.load_library().mi_lte_get_n_cce(n_rb, int(np.ceil(n_rb / 8.0)), cfi + (1 if n_rb <= 10 else 0), n_ant)


def make_units(rng, n_rb, n_ant, cfi, sizes, n, cells, snr_db, seed, n_rec=(2, 5)):
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(FFT[n_rb], n_rb, n_ant, 0)
    sfs, cell = rng.integers(0, 10, n), rng.choice(cells, n)
    n_cce = n_cce_of(n_rb, n_ant, cfi)
    recs = [random_records(rng, n_cce, int(sfs[u]), sizes, int(rng.integers(*n_rec))) for u in range(n)]
    g = synth.ctrl_grids_dci(cfg, sfs, cell, np.full(n, cfi), recs, snr_db=snr_db, seed=seed)
    return cfg, sfs, cell, recs, g, n_cce


# ---- exact against the model

SHAPES = [(25, 1, 3, (27, 41)), (25, 2, 3, (27, 41)), (25, 4, 3, (27, 41)), (15, 2, 2, (22, 31)), (6, 1, 3, (21,)), (6, 2, 3, (21,)), (100, 4, 3, (28,))]


@pytest.mark.parametrize("n_rb,n_ant,cfi,sizes", SHAPES)
def test_search_equals_the_model_at_3_db(ctx, n_rb, n_ant, cfi, sizes):
    rng = np.random.default_rng(100 * n_rb + n_ant)
    n, cells = (4 if n_rb == 100 else 24), [5, 301]
    cfg, sfs, cell, recs, g, n_cce = make_units(rng, n_rb, n_ant, cfi, sizes, n, cells, 3.0, n_rb + n_ant)
    if n_rb == 100:  # one unit with four symbols: the extent of the plan's tables
        from openlte_amd import synth
        g[0] = synth.ctrl_grids_dci(cfg, sfs[:1], cell[:1], [4], [recs[0]], snr_db=3.0, seed=3)[0]
    rntis = sorted({r[0] for lst in recs for r in lst} | {int(x) for x in rng.integers(1, 0x10000, 40)})
    plan = ctx.pdcch_search_plan(cfg, cells, sizes, rntis)
    dev = Dev(ctx, g, sfs, cell)
    try:
        h_cfi, h_n_cce, n_found, found = dev.run(plan)
        soft = plan.soft(n)
    finally:
        dev.free()
        plan.close()
    # at 3 dB the PCFICH itself fails on the weaker channels (cfi 0: no candidate) or, rarely, decodes as another value: whatever it gave, the
    # region's size follows from it, and the model below runs on that size
    want_cfi = [4 if (n_rb == 100 and u == 0) else cfi for u in range(n)]
    assert h_n_cce.tolist() == [n_cce_of(n_rb, n_ant, int(c)) if c > 0 and c + (n_rb <= 10) <= 4 else 0 for c in h_cfi]
    assert sum(int(a) == b for a, b in zip(h_cfi, want_cfi)) >= n // 4
    assert soft.shape[1] >= 72 * int(h_n_cce.max())
    assert all((np.abs(soft[u, :72 * int(h_n_cce[u])].astype(np.int64)) <= 127).all() for u in range(n))  # (the de-mapper's range; past 72 N_cce nothing is written)
    if n_rb == 6:
        assert h_n_cce.max() < 8  # no L = 8 candidate: floor(N_cce / 8) = 0
    w_n, w_found = model(soft, h_n_cce, sfs, sizes, bitmap(rntis), False)
    assert n_found.tolist() == w_n.tolist()
    assert found == w_found
    assert int(n_found.sum()) > 0


def test_search_order_and_cap_with_every_rnti_listed(ctx):
    """All 65 535 RNTIs and ANY_CCE: every candidate of non-zero energy is a hit, h_n_found exceeds the cap and the order rule decides."""
    rng = np.random.default_rng(77)
    sizes, n = (27, 41), 6
    cfg, sfs, cell, recs, g, n_cce = make_units(rng, 25, 2, 3, sizes, n, [9], 3.0, 77)
    plan = ctx.pdcch_search_plan(cfg, [9], sizes, np.arange(1, 0x10000), any_cce=True)
    dev = Dev(ctx, g, sfs, cell)
    try:
        _, h_n_cce, n_found, found = dev.run(plan)
        soft = plan.soft(n)
    finally:
        dev.free()
        plan.close()
    w_n, w_found = model(soft, h_n_cce, sfs, sizes, bitmap(np.arange(1, 0x10000)), True)
    assert n_found.tolist() == w_n.tolist() and found == w_found
    n_pairs = sum(1 for L, _ in candidates(20) for s in sizes if s + 16 < 72 * L)
    full = [u for u in range(n) if h_n_cce[u] == 20]  # (the units whose PCFICH survived 3 dB)
    assert full and n_found[full].min() > MAX_FOUND and n_found.max() <= n_pairs
    for u in full:
        lst = found[u]
        assert len(lst) == MAX_FOUND
        keys = [(-L, cce, sizes.index(nb)) for _, L, cce, nb, _, _, _ in lst]
        assert keys == sorted(keys) and len(set(keys)) == MAX_FOUND


# ---- every DCI sent is found where it was sent

@pytest.mark.parametrize("n_rb,n_ant,cfi,sizes", [(25, 1, 3, (27, 41)), (25, 2, 3, (27, 41)), (25, 4, 3, (27, 41)), (15, 2, 2, (22, 31)), (6, 1, 3, (21,)), (6, 4, 3, (21,))])
def test_every_dci_sent_is_found_where_it_was_sent(ctx, n_rb, n_ant, cfi, sizes):
    rng = np.random.default_rng(7 * n_rb + n_ant)
    n, cells = 48, [0, 77, 503]
    cfg, sfs, cell, recs, g, n_cce = make_units(rng, n_rb, n_ant, cfi, sizes, n, cells, 30.0, 5 * n_rb + n_ant)
    rntis = sorted({r[0] for lst in recs for r in lst})
    assert {r[1] for lst in recs for r in lst} == {L for L in (1, 2, 4, 8) if L <= n_cce}  # every aggregation level the shape has, L = 1 included
    plan = ctx.pdcch_search_plan(cfg, cells, sizes, rntis)
    dev = Dev(ctx, g, sfs, cell)
    try:
        h_cfi, h_n_cce, n_found, found = dev.run(plan)
    finally:
        dev.free()
        plan.close()
    assert h_cfi.tolist() == [cfi] * n and h_n_cce.tolist() == [n_cce] * n
    for u in range(n):
        assert 2 <= len(recs[u]) <= 4 or n_rb == 6
        got = {t[:5] for t in found[u]}
        assert int(n_found[u]) <= MAX_FOUND  # (nothing was cut off: the lists are complete)
        for r in recs[u]:
            assert r in got, (u, r, sorted(got))
        assert {t[0] for t in found[u]} <= set(rntis)


# ---- the filter

def test_search_space_filter(ctx):
    import openlte_amd as m
    from openlte_amd import synth
    cfg = m.DlCfg(512, 25, 2, 0)
    sf, cell, n_cce, rnti = 4, 21, 20, 0x2B1D
    own = {L: set(space(rnti, sf, n_cce, L)) for L in (1, 2, 4, 8)}
    outside = next(c for c in range(n_cce) if c not in own[1])  # one CCE that is not the RNTI's (and L = 1 is never the common space's)
    common = next(c for c in (0, 4, 8, 12) if c not in own[4])
    recs = [[(rnti, 1, outside, 27, 0x5A5A5A5)], [(rnti, 4, common, 41, 0x123456789A)]]
    g = synth.ctrl_grids_dci(cfg, [sf, sf], [cell, cell], [3, 3], recs, snr_db=30.0, seed=2)
    dev = Dev(ctx, g, [sf, sf], [cell, cell])
    res = {}
    try:
        for any_cce in (False, True):
            plan = ctx.pdcch_search_plan(cfg, [cell], (27, 41), [rnti], any_cce=any_cce)
            res[any_cce] = dev.run(plan)[3]
            plan.close()
    finally:
        dev.free()
    assert recs[0][0] not in {t[:5] for t in res[False][0]}
    assert recs[0][0] in {t[:5] for t in res[True][0]}
    assert recs[1][0] in {t[:5] for t in res[False][1]} and recs[1][0] in {t[:5] for t in res[True][1]}
    for u in range(2):  # what the default reports lies in the RNTI's own or the common space, and ANY_CCE reports all of it and more
        for t in res[False][u]:
            assert t[2] in own[t[1]] or (t[1] >= 4 and t[2] in (0, 4, 8, 12))
        assert set(res[False][u]) <= set(res[True][u])


# ---- agreement with the existing receiver where both can see

@pytest.mark.parametrize("n_rb,n_ant", [(25, 1), (25, 2), (50, 4), (6, 2)])
def test_search_agrees_with_the_common_space_receiver(ctx, n_rb, n_ant):
    import openlte_amd as m
    from openlte_amd import synth
    rng = np.random.default_rng(n_rb + n_ant)
    n, cells = 32, [12, 400]
    cfg = m.DlCfg(FFT[n_rb], n_rb, n_ant, 0)
    sfs, cell, cfis = rng.integers(0, 10, n), rng.choice(cells, n), rng.integers(2 if n_rb > 10 else 1, 4, n)
    rntis = [0xFFFF, 0xFFFE] + list(range(1, 0x3D))
    dcis = []
    for u in range(n):
        lst = []
        for r in rng.choice(rntis, int(rng.integers(1, 4 if n_rb > 6 else 2)), replace=False):
            npb = int(rng.integers(1, min(n_rb // 2, 8) + 1))
            lst.append((int(r), int(rng.integers(0, 27)), npb, int(rng.integers(0, n_rb - npb + 1)), int(rng.integers(0, 4))))
        dcis.append(lst)
    g = synth.ctrl_grids(cfg, sfs, cell, cfis, dcis, snr_db=12.0, seed=n_rb + n_ant)
    size = DCI_1A_BITS[n_rb]
    old = ctx.pdcch_plan(cfg, cells, 1.0, per_port_estimates=True)
    new = ctx.pdcch_search_plan(cfg, cells, (size,), rntis)
    dev = Dev(ctx, g, sfs, cell)
    try:
        _, o_cfi, _, o_dci = old.decode_dev(dev.bufs[0], dev.bufs[1], dev.bufs[2], n)
        h_cfi, _, n_found, found = dev.run(new)
    finally:
        dev.free()
        old.close()
        new.close()
    assert h_cfi.tolist() == o_cfi.tolist() == cfis.tolist()
    n_seen = 0
    for u in range(n):
        got = {t[:5] for t in found[u]}
        assert int(n_found[u]) <= MAX_FOUND
        for d in o_dci[u]:
            if d.format == 0 and d.candidate < 4:
                assert (d.rnti, 4, 4 * d.candidate, size, d.payload) in got, (u, d.rnti, d.candidate)
                n_seen += 1
    assert n_seen >= (n // 2 if n_rb > 6 else 1)  # (the comparison is not an empty one)


# ---- edges

def test_search_edges(ctx):
    import openlte_amd as m
    from openlte_amd import synth
    rng = np.random.default_rng(1)
    cfg = m.DlCfg(512, 25, 2, 0)
    sizes, rnti, sf, cell = (27, 41), 0x1234, 6, 33
    cce = space(rnti, sf, 20, 2)[0]
    rec = (rnti, 2, cce, 27, 0x2AAAAAA)
    g = synth.ctrl_grids_dci(cfg, [sf] * 4, [cell, 34, cell, cell], [3] * 4, [[rec], [rec], [rec], []], snr_db=200.0, seed=4)
    g[2, :2] = rng.standard_normal(g[2, :2].shape).astype(np.float32)  # unit 2: the received grid is noise, PCFICH included
    plan = ctx.pdcch_search_plan(cfg, [cell], sizes)  # (cell 34 is not the plan's)
    dev = Dev(ctx, g, [sf] * 4, [cell, 34, cell, cell])
    try:
        h_cfi, h_n_cce, n_found, found = dev.run(plan)
        assert h_cfi.tolist() == [3, 0, 0, 3] and h_n_cce.tolist() == [20, 0, 0, 20]
        assert n_found.tolist() == [0, 0, 0, 0] and found == [[], [], [], []]  # an empty RNTI set: no hit
        assert ctx.last_kernels().split(",")[:2] == ["k_pdcch_search_demod:1", "k_pdcch_search_decode:1"]
        soft = plan.soft(4)
        plan.set_rntis([rnti, 0x4321])
        h_cfi, h_n_cce, n_found, found = dev.run(plan)  # ... changes the second run only
        assert h_cfi.tolist() == [3, 0, 0, 3] and h_n_cce.tolist() == [20, 0, 0, 20]
        assert rec in {t[:5] for t in found[0]} and found[1] == [] and found[2] == [] and n_found[1:3].tolist() == [0, 0]
        # unit 3: a noiseless empty control region gives no hit, here and in the model (its soft bits are the de-mapper's smallest, +-1)
        assert n_found[3] == 0 and found[3] == []
        assert (np.abs(soft[3, :72 * 20]) == 1).all()
        w_n, w_found = model(soft, h_n_cce, [sf] * 4, sizes, bitmap([rnti, 0x4321]), False)
        assert n_found.tolist() == w_n.tolist() and found == w_found
        with pytest.raises(m.MiLteError, match="error -1"):
            plan.set_rntis([rnti, 0])
        with pytest.raises(m.MiLteError):
            plan.set_rntis([0x10000])
        assert dev.run(plan)[2].tolist() == n_found.tolist()  # a refused set leaves the plan's as it was
        plan.set_rntis([])
        assert dev.run(plan)[2].tolist() == [0, 0, 0, 0]
    finally:
        dev.free()
        plan.close()


def test_search_plan_refusals(ctx):
    import openlte_amd as m
    cfg = m.DlCfg(512, 25, 2, 0)
    for bad_cfg, kw in [(m.DlCfg(512, 26, 2, 0), {}), (m.DlCfg(512, 25, 3, 0), {}), (cfg, {"phich_res": 0.0}), (cfg, {"phich_res": 2.5}), (cfg, {"phich_res": float("nan")})]:
        with pytest.raises(m.MiLteError, match="error -4"):
            ctx.pdcch_search_plan(bad_cfg, [1], (27,), **kw)
    with pytest.raises(m.MiLteError, match="error -4"):
        m.PdcchSearchPlan(ctx, cfg, [1], (27,), phich_dur_extended=1)
    for sizes in [(), (27, 28, 29, 30, 31), (7,), (65,), (27, 41, 27)]:
        with pytest.raises(m.MiLteError, match="error -1"):
            ctx.pdcch_search_plan(cfg, [1], sizes)
    for rntis in [[0], [5, 0x10000]]:
        with pytest.raises(m.MiLteError, match="error -1"):
            ctx.pdcch_search_plan(cfg, [1], (27,), rntis)
    with pytest.raises(m.MiLteError, match="error -1"):
        ctx.pdcch_search_plan(cfg, [504], (27,))
    # every refusal came before any launch and the context is still usable
    plan = ctx.pdcch_search_plan(cfg, [1], (8, 64), [5])
    with pytest.raises(m.MiLteError):
        plan.soft(1)  # no run yet
    plan.close()

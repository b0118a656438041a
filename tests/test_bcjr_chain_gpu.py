"""GPU: the max-log-MAP decoders behind a reference-mode PDSCH plan (mi_lte_pdsch_plan_set_decoder: BCJR, BCJR_BLOCK, BCJR_EARLY) -- the glue
in front of and behind the decoders, which nothing else runs: k_cb_desc + k_rm_bcjr_prep (rate un-matching straight into the batch decoder's granule
arrays and tail records), k_rm_to_i8 (rate un-matching into the interleaved int8 block k_bcjr_block takes), k_crc_finish (filler removal, CRC24A,
byte / packed output) and pdsch_run's loop over the block-size groups through one scratch.  The decoders themselves are pinned at all 188 sizes
(test_bcjr_sizes_gpu.py); here every shape class of the glue runs: N_d = 4 / 12 / 20 / 28, K % 16 = 8, K % 64 != 0, the six workgroup widths, every
redundancy version with K_MIMO 1 and 2, a limited soft buffer, punctured blocks, many laps with and without saturation of their sums, the staged and
the unstaged gathers of both kernels, filler bits, groups of 1 / 64 / 65 / 130 code blocks, a later group smaller than an earlier one, both
interleavers, early termination and a re-assigned dynamic plan's scratch growth -- then a seeded sweep over every bandwidth, 1 / 2 / 4 ports and
every modulation.

The checker is test_pdsch_chain_in_bcjr_mode's composition, for every allocation of a plan after a run: the allocation's soft bits (the demodulator
is pinned by the REF-mode tests and does not depend on the decoder) -> lo_rate_unmatch_turbo (pinned to the compiled reference in test_oracle.py) ->
10000.0 (NULL) to 0, clip to +-127 -> the plain-C model of the decoder -> filler removal + CRC24A.  Status and EVERY output bit must be equal, the
bits of blocks whose CRC fails included (the library writes them).  No tolerance anywhere in this file."""
import functools
import time

import numpy as np
import pytest

import fuzz_cases as fz
import lte_testdata as td

pytestmark = pytest.mark.gpu

N_ITER = 6
THREADS = min(16, fz.n_threads())
# 36.212 table 5.1.4-1: the sub-block interleaver's column permutation
COL_PERM = np.array([0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31])


# ---------------------------------------------------------------------------------------------------
# the geometry the kernels branch on, restated (36.212 5.1.4.1.2 with N_soft = 250368, M_DL_HARQ = 8, C = 1; turbo_plan.hpp, turbo.hip)

def block_size(tbs):
    """(K, F): the smallest turbo block size that holds the transport block and its CRC, and the filler bits in front of it."""
    K = next(k for k in td.ALL_K if k >= tbs + 24)
    return K, K - tbs - 24


@functools.lru_cache(maxsize=None)
def rm_geom(K, k_mimo):
    """(N_d, K_w, N_cb, N_nn): head padding of a stream, circular buffer, its limited length, soft bits one lap of it consumes."""
    D = K + 4
    R = (D + 31) // 32
    K_pi = 32 * R
    N_d, K_w = K_pi - D, 3 * K_pi
    N_cb = min(K_w, 250368 // (k_mimo * 8))
    p = np.arange(N_cb)
    q = np.maximum(p - K_pi, 0) >> 1
    n0 = 32 * (p % R) + COL_PERM[np.minimum(p // R, 31)]
    n12 = 32 * (q % R) + COL_PERM[np.minimum(q // R, 31)]
    n = np.where(p < K_pi, n0, np.where((p - K_pi) % 2 == 0, n12, (n12 + 1) % K_pi))
    return N_d, K_w, N_cb, int((n >= N_d).sum())  # (head padding is the only NULL the receiver honours)


def k_mimo(tx_mode):
    return 2 if tx_mode in (3, 4, 8, 9) else 1


def kpad64(K):
    return (K + 63) & ~63


def cb_width(K):
    return ((kpad64(K) >> 4) + 63) & ~63


def stage_cap(e_max):
    return (e_max + 16 + 63) & ~63


def e_max_of(al, cfi):
    """What the plan sizes an allocation's soft bits by (chain.hip plan_layout): every resource element behind the control region."""
    return (14 - cfi) * al.N_prb * 12 * (1, 2, 4, 6)[al.mod_type]


def staging(allocs, soft, cfi):
    """Per allocation (k_rm_bcjr_prep staged?, k_rm_to_i8 staged?), as mi_turbo_bcjr_group and the kernels decide it: per block-size GROUP the
    LDS room is that of the group's largest allocation -- next to the block's own Kp bytes in k_rm_bcjr_prep -- and none beyond 60 KiB; an
    allocation is then staged when it fits the room and its ranks fit 16 bits."""
    e_max = {}
    for al in allocs:
        K = block_size(al.tbs)[0]
        e_max[K] = max(e_max.get(K, 0), e_max_of(al, cfi))
    out = []
    for al, e in zip(allocs, soft):
        K = block_size(al.tbs)[0]
        cap = stage_cap(e_max[K])
        cap_prep = cap if kpad64(K) + cap <= 60 * 1024 else 0
        cap_i8 = cap if cap <= 60 * 1024 else 0
        E = len(e)
        out.append((E + 16 <= cap_prep and E < 0xFFFF, E + 16 <= cap_i8 and E < 0xFFFF))
    return out


# ---------------------------------------------------------------------------------------------------
# the checker

_EXPECTED = {}  # one model run per (soft bits, parameters): the plans of a test that share allocations share it


@pytest.fixture(autouse=True)
def _forget_expected():
    yield
    _EXPECTED.clear()


def expected(port, e, tbs, tx_mode, rv, block, n_iter, spec):
    """(status, bits [tbs], the rate un-matched sums before the clip) of the composition."""
    key = (e.tobytes(), tbs, tx_mode, rv, block, n_iter, spec)
    if key not in _EXPECTED:
        K, F = block_size(tbs)
        d = np.zeros(3 * (K + 4), np.float32)
        n = port.lo_rate_unmatch_turbo(np.ascontiguousarray(e, np.float32), len(e), K + 4, 1, tx_mode, 250368, 8, 0, rv, d)
        assert n == 3 * (K + 4)
        soft = np.where(d == 10000.0, 0.0, np.clip(d, -127, 127)).astype(np.int16)
        c = np.zeros(K, np.uint8)
        (port.lo_turbo_decode_bcjr_block if block else port.lo_turbo_decode_bcjr)(soft, K, n_iter, spec, c)
        p = np.zeros(24, np.uint8)
        port.lo_crc24a(np.ascontiguousarray(c[F:F + tbs]), tbs, p)
        _EXPECTED[key] = (0 if (p == c[F + tbs:]).all() else 2, c[F:F + tbs].copy(), d)
    return _EXPECTED[key]


def check(port, allocs, soft, st, bits, mode, spec=0, iters=None, what=""):
    """Status and every bit of every allocation against the composition.  iters: iterations per allocation (BCJR_EARLY), else N_ITER."""
    import openlte_amd as m
    block = mode == m.TURBO_BCJR_BLOCK

    def one(a):
        al = allocs[a]
        return expected(port, soft[a], al.tbs, al.tx_mode, al.rv_idx & 3, block, int(iters[a]) if iters is not None else N_ITER, spec)
    want = td.parallel_map(one, range(len(allocs)), threads=THREADS)
    bad = []
    for a, (w_st, w_bits, _) in enumerate(want):
        al = allocs[a]
        row = (a, al.tbs, al.mod_type, al.N_prb, al.rv_idx, al.tx_mode, len(soft[a]))
        if int(st[a]) != w_st:
            bad.append(("status", row, int(st[a]), w_st, int((bits[a] != w_bits).sum())))
        elif not (bits[a] == w_bits).all():
            bad.append(("bits", row, int((bits[a] != w_bits).sum())))
    assert not bad, (what, mode, spec, len(bad), bad[:8])
    return want


class Scene:
    """Subframe units from the library's own transmitter (synth.dl_units: it honours rv and tx_mode for F = 0) on a 20 MHz one-port cell,
    through the library's front end, resident on the device.  units = [(subframe, cell, snr_db, [(mod, tbs, prbs, rv, tx_mode), ...]), ...];
    .allocs[k] / .tx[k] in unit-major order."""

    def __init__(self, ctx, units, cfi=2, seed=1):
        import openlte_amd as m
        from openlte_amd import synth
        self.cfi = cfi
        self.cfg = m.DlCfg(2048, 100, 1, 0)
        self.sfs, self.cells = [u[0] for u in units], [u[1] for u in units]
        self.allocs, self.tx, iqs = [], [], []
        for u, (sf, cell, snr, specs) in enumerate(units):
            assert sf not in (0, 5)  # 138 resource elements per PRB with two control symbols
            one = [m.make_alloc(0, mod, tbs, list(prbs), 0x100 + i, rv, txm) for i, (mod, tbs, prbs, rv, txm) in enumerate(specs)]
            iq, t = synth.dl_units(self.cfg, [sf], [cell], one, len(one), n_pdcch_symbs=cfi, snr_db=snr, max_delay=4, seed=1000 * seed + u)
            iqs.append(iq[0])
            for i, (mod, tbs, prbs, rv, txm) in enumerate(specs):
                self.allocs.append(m.make_alloc(u, mod, tbs, list(prbs), 0x100 + i, rv, txm))
                self.tx.append(t[0, i, :tbs].copy())
        iq = np.stack(iqs)
        grid = ctx.dl_frontend(self.cfg, iq.reshape(-1, 2), np.arange(len(units)) * iq.shape[1], self.sfs, self.cells)
        self.d_sub = ctx.to_device(np.ascontiguousarray(grid, np.float32))

    def close(self):
        self.d_sub.free()


def both_modes():
    import openlte_amd as m
    return (m.TURBO_BCJR, m.TURBO_BCJR_BLOCK)


def run_plan(ctx, port, sc, allocs, tx=None, modes=None, spec=0, packed=False, limited=False, what=""):
    """One plan over `allocs` of the scene, run under every mode (and, packed, in both output forms), each run through the checker.
    Returns ({mode: (status, bits, expected)}, soft bits).  A block that passes its CRC is also the transmitted one (tx given)."""
    plan = ctx.pdsch_plan(sc.cfg, sc.cfi, allocs)
    res, soft = {}, None
    try:
        for mode in (modes or both_modes()):
            plan.set_decoder(mode, N_ITER, spec)
            for pk in ((False, True) if packed else (False,)):
                plan.set_packed(pk)
                st, bits = plan.run(sc.d_sub, sc.sfs, sc.cells)
                if soft is None:
                    soft = [plan.soft_bits(a) for a in range(len(allocs))]
                want = check(port, allocs, soft, st, bits, mode, spec, what=(what, "packed" if pk else "bytes"))
                if tx is not None:
                    for a in range(len(allocs)):
                        assert st[a] != 0 or (bits[a] == tx[a]).all(), (what, mode, a)
            res[mode] = (st.copy(), [b.copy() for b in bits], want)
    finally:
        plan.close()
    assert_limited(allocs, limited, what)
    return res, soft


def assert_limited(allocs, limited, what):
    """The limited soft buffer (N_cb < K_w) is where a row says so and nowhere else."""
    for al in allocs:
        _, K_w, N_cb, _ = rm_geom(block_size(al.tbs)[0], k_mimo(al.tx_mode))
        assert (N_cb < K_w) == limited, (what, al.tbs, al.tx_mode, N_cb, K_w)


def assert_both_verdicts(res, what):
    for mode, (st, _, _) in res.items():
        assert (st == 0).any() and (st == 2).any(), (what, mode, st.tolist())
        assert ((st == 0) | (st == 2)).all(), (what, mode, st.tolist())


# ---------------------------------------------------------------------------------------------------
# A. designed cases

def test_nd_classes_and_short_last_units(ctx, port):
    """K = 104, 112, 120, 128: N_d = 20, 12, 4, 28; K % 16 = 8 (nv = 8 in the last unit) at 104 and 120; Kp > K for all but 128.  QPSK on one PRB
    (E = 276: punctured) and on three (E = 828: two laps or more), every redundancy version."""
    tbss = (80, 88, 96, 104)
    assert [block_size(t) for t in tbss] == [(104, 0), (112, 0), (120, 0), (128, 0)]
    assert [rm_geom(t + 24, 1)[0] for t in tbss] == [20, 12, 4, 28]
    units = []
    for rv in range(4):
        for snr in (25.0, -8.0):
            specs = []
            for i, tbs in enumerate(tbss):
                specs += [(1, tbs, [4 * i], rv, 1), (1, tbs, [4 * i + 1, 4 * i + 2, 4 * i + 3], rv, 1)]
            units.append((1 + len(units) % 4, 11 + 40 * len(units), snr, specs))
    sc = Scene(ctx, units, seed=1)
    try:
        res, soft = run_plan(ctx, port, sc, sc.allocs, sc.tx, what="N_d")
        for al, e in zip(sc.allocs, soft):
            nnn = rm_geom(al.tbs + 24, 1)[3]
            assert nnn == 3 * (al.tbs + 28) and len(e) == 276 * al.N_prb
            assert (len(e) < nnn) if al.N_prb == 1 else (len(e) >= 2 * nnn)
        assert_both_verdicts(res, "N_d")
    finally:
        sc.close()


WIDTH_ROWS = ((512, 2), (1056, 4), (2560, 10), (3136, 12), (4096, 15), (5056, 19), (6144, 23))  # (K, PRBs at 64QAM: E a little above 3 (K + 4))


def test_every_workgroup_width(ctx, port):
    """k_rm_bcjr_prep runs one thread per 16 steps in workgroups of 64 .. 384 threads: a block size per width (1056: Kp = 1088), E a little above
    a lap at 64QAM, the redundancy versions cycling over them."""
    assert {cb_width(K) for K, _ in WIDTH_ROWS} == {64, 128, 192, 256, 320, 384}
    assert sum(n for _, n in WIDTH_ROWS) <= 100 and kpad64(1056) == 1088
    units = []
    for u, snr in enumerate((30.0, 30.0, 16.0, 11.0)):
        specs, first = [], 0
        for i, (K, n_prb) in enumerate(WIDTH_ROWS):
            assert block_size(K - 24) == (K, 0) and 3 * (K + 4) <= 828 * n_prb < 3 * (K + 4) + 828
            specs.append((3, K - 24, range(first, first + n_prb), (i + u) % 4, 1))
            first += n_prb
        units.append(((2, 3, 4, 6)[u], 100 * u + 3, snr, specs))
    sc = Scene(ctx, units, seed=2)
    try:
        res, _ = run_plan(ctx, port, sc, sc.allocs, sc.tx, what="widths")
        assert_both_verdicts(res, "widths")
    finally:
        sc.close()


def test_limited_soft_buffer(ctx, port):
    """tx_mode 3 and 4 (K_MIMO = 2): N_IR = 250368 / 16 = 15 648 soft positions, below K_w at K = 5312 (16 032) and 6144 (18 528) -- the rank
    tables' odd combos with positions the buffer never holds.  Every redundancy version, 16QAM and 64QAM."""
    units = []
    for txm in (3, 4):
        for mod, prbs in ((2, (29, 34)), (3, (20, 23))):
            for rv in range(4):
                lo = 9.0 if mod == 2 else 15.0
                specs = [(mod, 5312 - 24, range(0, prbs[0]), rv, txm), (mod, 6144 - 24, range(40, 40 + prbs[1]), rv, txm)]
                units.append((1 + len(units) % 4, 7 + 29 * len(units), 30.0 if (rv + mod + txm) % 2 else lo, specs))
    sc = Scene(ctx, units, seed=3)
    try:
        for K in (5312, 6144):
            assert rm_geom(K, 2)[2] == 15648 < rm_geom(K, 2)[1] and rm_geom(K, 1)[2] == rm_geom(K, 1)[1]
        res, _ = run_plan(ctx, port, sc, sc.allocs, sc.tx, limited=True, what="limited buffer")
        assert_both_verdicts(res, "limited buffer")
    finally:
        sc.close()


def test_punctured_large_block(ctx, port):
    """K = 6144 on 20 PRB at 64QAM: E = 16 560 < 18 444, ranks the allocation does not reach; rv 0 and 2."""
    units = [(3 + u, 50 + 200 * u, snr, [(3, 6120, range(0, 20), 0, 1), (3, 6120, range(30, 50), 2, 1)]) for u, snr in enumerate((30.0, 14.0))]
    sc = Scene(ctx, units, seed=4)
    try:
        res, soft = run_plan(ctx, port, sc, sc.allocs, sc.tx, what="punctured")
        assert all(len(e) == 16560 < rm_geom(6144, 1)[3] == 18444 for e in soft)
        assert_both_verdicts(res, "punctured")
    finally:
        sc.close()


def test_many_laps_and_saturation(ctx, port):
    """K = 40 with QPSK on 8 PRB: E = 2 208, 16 laps of the 132-position buffer, their sums saturated to +-127 -- at noise levels where the
    sums before the clip lie on both sides of 127 in one block; and test_staged_soft_combining's tbs 1000 on 50 PRB (four laps and a half)."""
    units = [(1 + u, 60 * u + 9, snr, [(1, 16, range(0, 8), u % 4, 1), (1, 1000, range(20, 70), (u + 1) % 4, 1)]) for u, snr in enumerate((20.0, 4.0, -4.0, -10.0))]
    sc = Scene(ctx, units, seed=5)
    try:
        res, soft = run_plan(ctx, port, sc, sc.allocs, sc.tx, what="laps")
        over_and_under = 0
        for al, e, (_, _, d) in zip(sc.allocs, soft, res[both_modes()[0]][2]):  # (the sums do not depend on the decoder)
            if al.tbs != 16:
                assert len(e) == 13800 and len(e) // rm_geom(1024, 1)[3] == 4
                continue
            assert len(e) == 2208 and len(e) // rm_geom(40, 1)[3] == 16
            mag = np.abs(d[d != 10000.0])
            print("K = 40, 16 laps: sums beyond +-127: %d of %d, largest %d" % (int((mag > 127).sum()), len(mag), int(mag.max())))
            over_and_under += int((mag > 127).any() and (mag < 127).any())
        assert over_and_under >= 1  # a block whose sums lie on both sides of the clip
        assert_both_verdicts(res, "laps")
    finally:
        sc.close()


def test_unstaged_gathers(ctx, port):
    """The gathers from global memory.  k_rm_bcjr_prep stages a group's soft bits in LDS while Kp + stage_cap(e_max) <= 60 KiB, k_rm_to_i8
    while stage_cap(e_max) <= 60 KiB and E < 0xFFFF; e_max is the group's largest allocation, so one large allocation takes the staging away
    from every block of its size.  70 PRB at 64QAM: k_rm_bcjr_prep unstaged, k_rm_to_i8 staged; 100 PRB (E = 82 800 >= 0xFFFF): both unstaged;
    100 PRB and 45 PRB of the same size in one group: both unstaged for both; 45 PRB alone: both staged."""
    sc1 = Scene(ctx, [(2 + u, 31 + 300 * u, snr, [(3, 6120, range(10, 80), 2 * u, 1)]) for u, snr in enumerate((30.0, 13.0))], seed=6)
    sc2 = Scene(ctx, [(1, 17, 30.0, [(3, 5992, range(0, 100), 0, 1)]), (8, 404, -6.0, [(3, 5992, range(0, 100), 1, 1)]),
                      (3, 250, 30.0, [(3, 5992, range(50, 95), 0, 1)]), (7, 99, 13.0, [(3, 5992, range(5, 50), 3, 1)])], seed=7)
    try:
        sides = {}
        for name, sc, sel, want_sides in (("70 PRB", sc1, [0, 1], {(False, True)}), ("100 PRB", sc2, [0, 1], {(False, False)}),
                                          ("100 + 45 PRB", sc2, [0, 1, 2, 3], {(False, False)}), ("45 PRB", sc2, [2, 3], {(True, True)})):
            allocs = [sc.allocs[k] for k in sel]
            res, soft = run_plan(ctx, port, sc, allocs, [sc.tx[k] for k in sel], what=name)
            sides[name] = set(staging(allocs, soft, sc.cfi))
            assert sides[name] == want_sides, (name, sides[name], [len(e) for e in soft])
            print("staging (k_rm_bcjr_prep, k_rm_to_i8) of", name, sorted(sides[name]), "E", [len(e) for e in soft])
            if name != "45 PRB":
                assert_both_verdicts(res, name)
        assert [len(e) for e in soft] == [37260, 37260]
        every = set().union(*sides.values())
        assert {s[0] for s in every} == {False, True} and {s[1] for s in every} == {False, True}  # both sides of both thresholds
    finally:
        sc1.close()
        sc2.close()


FILLER_ROWS = ((672, 1, 8), (1376, 2, 8), (2000, 3, 8), (680, 1, 8), (3200, 3, 12))  # test_filler_bit_transport_blocks_same_verdict_as_reference's


class RefScene:
    """Captures of the reference's own transmitter (td.multi_port_capture: it places filler bits), one unit each, through the library's front end."""

    def __init__(self, ctx, ref, rows):
        """rows = [(tbs, mod, n_prb, noise, seed)]"""
        import openlte_amd as m
        self.cfg, self.cfi = m.DlCfg(2048, 100, 1, 0), 2
        self.allocs, self.tx, self.sfs, self.cells, iqs = [], [], [], [], []
        for u, (tbs, mod, n_prb, noise, seed) in enumerate(rows):
            cap = td.multi_port_capture(ref, 1, seed=seed, mod=mod, tbs=tbs, prbs=list(range(30, 30 + n_prb)), noise=noise)
            ref.ref_phy_free(cap["phy"])
            iqs.append(cap["iq"])
            self.sfs.append(cap["sf"])
            self.cells.append(cap["cell"])
            self.allocs.append(m.make_alloc(u, mod, tbs, cap["prbs"], 0x2345, 0, 1))
            self.tx.append(cap["msg"])
        self.iq = np.stack(iqs)
        grid = ctx.dl_frontend(self.cfg, self.iq.reshape(-1, 2), np.arange(len(rows)) * self.iq.shape[1], self.sfs, self.cells)
        self.d_sub = ctx.to_device(np.ascontiguousarray(grid, np.float32))

    def close(self):
        self.d_sub.free()


def test_filler_bits(ctx, port, ref):
    """F > 0 (tbs + 24 between two block sizes): k_crc_finish starts behind the filler bits, in byte and in packed output; tbs = 680 is the
    F = 0 control.  Clean captures and noisy ones."""
    assert [block_size(t)[1] for t, _, _ in FILLER_ROWS] == [8, 8, 24, 0, 40]
    rows = [(tbs, mod, n_prb, noise, tbs + int(noise)) for noise in (0.0, 25.0) for tbs, mod, n_prb in FILLER_ROWS]
    sc = RefScene(ctx, ref, rows)
    try:
        res, _ = run_plan(ctx, port, sc, sc.allocs, sc.tx, packed=True, what="filler")
        assert_both_verdicts(res, "filler")
    finally:
        sc.close()


def test_transport_block_that_is_no_multiple_of_8(ctx, port, ref):
    """tbs = 1001 (K = 1056, F = 31; none of TS 36.213's sizes): k_crc_finish's bit-by-bit path, bytes and packed.  The same row through the
    REF decoder against lo_pdsch_channel_decode on the oracle's own grid.  Were plan creation to refuse the size, the refusal is the contract."""
    import openlte_amd as m
    import test_chain_gpu as tc
    assert block_size(1001) == (1056, 31)
    cfg = m.DlCfg(2048, 100, 1, 0)
    try:
        ctx.pdsch_plan(cfg, 2, [m.make_alloc(0, 1, 1001, list(range(30, 42)), 0x2345, 0, 1)]).close()
    except m.MiLteError as ex:
        assert "error -4" in str(ex), ex  # MI_LTE_ERR_UNSUPPORTED
        return
    sc = RefScene(ctx, ref, [(1001, 1, 12, 0.0, 1001), (1001, 1, 12, 30.0, 1002), (1001, 1, 12, 60.0, 1003)])
    try:
        res, _ = run_plan(ctx, port, sc, sc.allocs, None, packed=True, what="tbs 1001")
        # the REF decoder, fed the oracle's grid: soft bits, verdict and transport block identical
        for u, al in enumerate(sc.allocs):
            lc, s = td.oracle_frontend(port, 2048, 100, 1, sc.iq[u], sc.sfs[u], sc.cells[u])
            one = m.make_alloc(0, 1, 1001, list(range(30, 42)), 0x2345, 0, 1)
            err, out, desc = tc.oracle_pdsch(port, lc, s, one, 2, sc.cells[u], 1)
            d_sub = ctx.to_device(tc.upload_oracle_subframe(ctx, s, 1))
            plan = ctx.pdsch_plan(cfg, 2, [one])
            for pk in (False, True):
                plan.set_packed(pk)
                st, bits = plan.run(d_sub, [sc.sfs[u]], [sc.cells[u]])
                e = plan.soft_bits(0)
                assert e.shape == desc.shape and (e == desc).all()
                assert st[0] == err and (err != 0 or (len(out) == 1001 and (bits[0] == out).all())), (u, pk, st[0], err)
            plan.close()
            d_sub.free()
    finally:
        sc.close()


def test_group_shapes(ctx, port):
    """Groups of 1, 64, 65 and 130 code blocks (one tile, one tile and a block, a tile pair and two) of K = 40 on one PRB each, spread over
    three subframes at different noise; and one plan of 130 x K = 40, 3 x K = 1056, 1 x K = 6144 -- the groups run in ascending K through one
    scratch, each later one smaller than the one before -- whose verdicts and bits equal those of the three sizes planned alone."""
    units = []
    for u, snr in enumerate((15.0, -9.0, -14.0)):
        specs = [(1, 16, [p], p % 4, 1) for p in range(44)] + [(3, 1032, range(44, 48), u, 1)]
        if u == 0:
            specs.append((3, 6120, range(50, 73), 0, 1))
        units.append(((2, 4, 8)[u], 5 + 111 * u, snr, specs))
    sc = Scene(ctx, units, seed=8)
    try:
        by_unit = [[k for k, al in enumerate(sc.allocs) if al.unit == u and al.tbs == 16] for u in range(3)]
        small = [by_unit[i % 3][i // 3] for i in range(130)]  # allocation i of the K = 40 plans sits in unit i % 3
        mid = [k for k, al in enumerate(sc.allocs) if al.tbs == 1032]
        big = [k for k, al in enumerate(sc.allocs) if al.tbs == 6120]
        assert len(mid) == 3 and len(big) == 1
        alone = {}
        for n in (1, 64, 65, 130):
            sel = small[:n]
            res, _ = run_plan(ctx, port, sc, [sc.allocs[k] for k in sel], [sc.tx[k] for k in sel], what="K = 40 x %d" % n)
            if n > 1:
                assert_both_verdicts(res, n)
            alone[40] = res
        alone[1056] = run_plan(ctx, port, sc, [sc.allocs[k] for k in mid], [sc.tx[k] for k in mid], what="K = 1056 x 3")[0]
        alone[6144] = run_plan(ctx, port, sc, [sc.allocs[k] for k in big], [sc.tx[k] for k in big], what="K = 6144 x 1")[0]
        sel = big + small[:70] + mid + small[70:]  # (allocation order is not group order)
        mixed, _ = run_plan(ctx, port, sc, [sc.allocs[k] for k in sel], [sc.tx[k] for k in sel], what="three sizes")
        for mode in both_modes():
            st, bits, _ = mixed[mode]
            where = {k: j for j, k in enumerate(sel)}
            for K, ks in ((40, small), (1056, mid), (6144, big)):
                st1, bits1, _ = alone[K][mode]
                for j, k in enumerate(ks):
                    assert st[where[k]] == st1[j] and (bits[where[k]] == bits1[j]).all(), (mode, K, j)
    finally:
        sc.close()


def test_both_interleavers(ctx, port):
    """qpp_spec 0 (the reference's wrapped uint32 arithmetic) and 1 (36.212's) at K = 6144 and 3584, where the two differ and the wrapped one is
    no permutation (the de-interleaver's holes).  The transmitter interleaves the reference's way: under qpp_spec 1 these blocks fail."""
    assert 6144 in td.OVERFLOW_K and 3584 in td.OVERFLOW_K
    units = [((4, 6)[u], 77 + u, snr, [(3, 6120, range(0, 23), u, 1), (3, 3560, range(30, 44), 2 + u, 1)]) for u, snr in enumerate((30.0, 14.0))]
    sc = Scene(ctx, units, seed=9)
    try:
        res0, _ = run_plan(ctx, port, sc, sc.allocs, sc.tx, spec=0, what="qpp_spec 0")
        res1, _ = run_plan(ctx, port, sc, sc.allocs, None, spec=1, what="qpp_spec 1")
        for mode in both_modes():
            print("verdicts under qpp_spec 0 / 1:", res0[mode][0].tolist(), res1[mode][0].tolist())
            # (K = 6144: the two interleavers differ from index 2992 on, K = 3584 in the last few positions only)
            assert (res0[mode][0] == 0).any() and (res1[mode][0][[0, 2]] == 2).all(), (mode, res0[mode][0], res1[mode][0])
            assert any((b0 != b1).any() for b0, b1 in zip(res0[mode][1], res1[mode][1]))
    finally:
        sc.close()


@pytest.mark.parametrize("K", [40, 1088])
def test_early_termination_on_a_plan(ctx, port, K):
    """BCJR_EARLY on a reference-mode plan: a tile pair (128 code blocks) stops once an iteration changes none of its decisions.  A block's bits
    and verdict are the BCJR model's at the iterations its pair ran.  Pair p holds slots 128 p .. 128 p + 127 of the group, and in a plan of one
    block size slot order is allocation order: mi_plan_group (plan_core.cc) hands the slots of a size out in ascending allocation index, and the
    only group starts at slot 0 -- so allocation a belongs to pair a // 128, and ctx.turbo_early_exit_iterations() describes the plan's only group.
    K = 40: 128 clean blocks and 2 hopeless ones; K = 1088: 120 clean and 8 marginal blocks in the first pair, 12 hopeless ones in the second."""
    import openlte_amd as m
    if K == 40:
        units = [(1 + u, 33 * u, 25.0, [(1, 16, [p], (p + u) % 4, 1) for p in range(64)]) for u in range(2)]
        units.append((7, 300, -12.0, [(1, 16, [p], p, 1) for p in range(2)]))
    else:
        units = [(1 + u % 4, 20 * u + 1, 30.0, [(3, 1064, range(4 * p, 4 * p + 4), (p + u) % 4, 1) for p in range(20)]) for u in range(6)]
        units.append((6, 401, 19.0, [(3, 1064, range(4 * p, 4 * p + 4), p % 4, 1) for p in range(8)]))
        units.append((8, 402, 3.0, [(3, 1064, range(4 * p, 4 * p + 4), p % 4, 1) for p in range(12)]))
    sc = Scene(ctx, units, seed=10 + K)
    plan = ctx.pdsch_plan(sc.cfg, sc.cfi, sc.allocs)
    try:
        n = len(sc.allocs)
        assert n == (130 if K == 40 else 140) and all(block_size(al.tbs) == (K, 0) for al in sc.allocs)
        assert_limited(sc.allocs, False, "early")
        plan.set_decoder(m.TURBO_BCJR_EARLY, N_ITER, 0)
        st, bits = plan.run(sc.d_sub, sc.sfs, sc.cells)
        iters = ctx.turbo_early_exit_iterations()
        print("BCJR_EARLY, K = %d, %d blocks: iterations per tile pair" % (K, n), iters.tolist())
        assert len(iters) == 2 and iters.min() >= 2 and iters.max() <= N_ITER
        assert iters[0] != iters[1], iters
        soft = [plan.soft_bits(a) for a in range(n)]
        check(port, sc.allocs, soft, st, bits, m.TURBO_BCJR_EARLY, 0, iters=[iters[a // 128] for a in range(n)], what="early")
        assert (st == 0).any() and (st == 2).any()
        for a in range(n):
            assert st[a] != 0 or (bits[a] == sc.tx[a]).all(), a
    finally:
        plan.close()
        sc.close()


def test_dynamic_plan_grows_its_scratch(ctx, port):
    """A dynamic plan under BCJR_BLOCK: two small allocations, then nine W4 allocations (the int8 block and the decisions no longer fit: the
    plan re-allocates both), then the two small ones again in the larger scratch.  Every run equals a fresh static plan's, and the composition."""
    import openlte_amd as m
    w4 = [(3, 3240, range(12 * a, 12 * a + 12), 0, 1) for a in range(8)] + [(3, 1064, range(96, 100), 0, 1)]
    sc = Scene(ctx, [(1, 17, 19.0, w4), (6, 404, 2.0, [(1, 16, [3], 1, 1), (1, 80, [7, 8, 9], 2, 1)])], seed=11)
    dyn = ctx.pdsch_plan_dynamic(sc.cfg, 16, 1 << 18)
    try:
        dyn.set_decoder(m.TURBO_BCJR_BLOCK, N_ITER, 0)
        small, big = sc.allocs[9:], sc.allocs[:9]
        assert_limited(sc.allocs, False, "dynamic")
        seen = []
        for step, allocs in enumerate((small, big, small)):
            dyn.assign(sc.cfi, allocs)
            st, bits = dyn.run(sc.d_sub, sc.sfs, sc.cells)
            soft = [dyn.soft_bits(a) for a in range(len(allocs))]
            check(port, allocs, soft, st, bits, m.TURBO_BCJR_BLOCK, what=("dynamic", step))
            fresh = ctx.pdsch_plan(sc.cfg, sc.cfi, allocs)
            fresh.set_decoder(m.TURBO_BCJR_BLOCK, N_ITER, 0)
            st1, bits1 = fresh.run(sc.d_sub, sc.sfs, sc.cells)
            fresh.close()
            assert (st == st1).all() and all((bits[a][:al.tbs] == bits1[a]).all() for a, al in enumerate(allocs)), step
            seen.append(st.tolist())
        assert seen[0] == seen[2]
    finally:
        dyn.close()
        sc.close()


def test_last_kernels_names_what_ran(ctx, port):
    """mi_lte_last_kernels after a reference-mode plan's run, per decoder: the batch kernels (BCJR, BCJR_EARLY) take k_cb_desc + k_rm_bcjr_prep,
    the one-block-per-wavefront decoder k_rm_to_i8 + k_bcjr_block."""
    import openlte_amd as m
    sc = Scene(ctx, [(3, 9, 25.0, [(1, 80, [0, 1, 2], 0, 1)])], seed=12)
    plan = ctx.pdsch_plan(sc.cfg, sc.cfi, sc.allocs)
    try:
        batch = "k_pdsch_demod:1,k_cb_desc,k_rm_bcjr_prep,k_bcjr_half,k_bcjr_final,k_crc_finish per block size"
        for mode, want in ((m.TURBO_BCJR, batch), (m.TURBO_BCJR_EARLY, batch),
                           (m.TURBO_BCJR_BLOCK, "k_pdsch_demod:1,k_rm_to_i8,k_bcjr_block,k_crc_finish per block size")):
            plan.set_decoder(mode, N_ITER, 0)
            st, bits = plan.run(sc.d_sub, sc.sfs, sc.cells)
            assert ctx.last_kernels() == want, (mode, ctx.last_kernels())
            assert st[0] == 0 and (bits[0] == sc.tx[0]).all()
    finally:
        plan.close()
        sc.close()


# ---------------------------------------------------------------------------------------------------
# B. a seeded sweep

@pytest.fixture(scope="module")
def ref_big():
    from oracle import pyoracle
    L = pyoracle.ref_big()
    if L is None:
        pytest.skip("oracle/_ref/libref_oracle_big.so not built (needs the reference tree at build time)")
    return L


def draw_counts(cases):
    """What the draw holds of each class the glue kernels branch on."""
    Ks, n_d, widths = set(), set(), set()
    punctured = laps = filler = rv_nz = k8 = 0
    for c in cases:
        K, F = block_size(c["tbs"])
        N_d, _, _, nnn = rm_geom(K, k_mimo(c["tx_mode"]))
        Ks.add(K)
        n_d.add(N_d)
        widths.add(cb_width(K))
        punctured += c["e"] < nnn
        laps += c["e"] >= 2 * nnn
        filler += F > 0
        rv_nz += c["rv"] != 0
        k8 += K % 16 == 8
    return dict(distinct_K=len(Ks), N_d=len(n_d), widths=len(widths), punctured=punctured, two_laps_or_more=laps, filler=filler, rv_not_0=rv_nz, K_mod_16_is_8=k8)


SWEEP_N, SWEEP_SEED = 400, 411
SWEEP_FLOORS = dict(distinct_K=120, N_d=4, widths=6, punctured=30, two_laps_or_more=40, filler=8, rv_not_0=150, K_mod_16_is_8=60)  # counted: 148 4 6 51 75 12 233 104


def test_seeded_sweep(ctx, port, ref_big):
    """fuzz_cases.draw_dl_cases(400, 411): every bandwidth, 1 / 2 / 4 ports, every modulation (BPSK included), rv, tx_mode, punctured, repeated
    and filler cases, captures from the reference's transmitter, the library's own front end, one plan per (bandwidth, ports, control region)
    group under BCJR x 6 and again under BCJR_BLOCK x 6, the checker on every case.  A case leaves only where plan creation refuses it with
    MI_LTE_ERR_UNSUPPORTED or the reference's transmitter rejects it: 2 % of the draw at most, printed."""
    import openlte_amd as m
    t_start = time.time()
    cases = fz.draw_dl_cases(SWEEP_N, SWEEP_SEED)
    counts = draw_counts(cases)
    print("sweep draw:", counts)
    for k, floor in SWEEP_FLOORS.items():
        assert counts[k] >= floor, (k, counts[k], floor)
    t0 = time.time()
    r = fz.run_ref_dl(ref_big, cases, want_planes=False)
    t_ref = time.time() - t0
    skipped = [("rc_tx", i, int(r["rc_tx"][i])) for i in range(len(cases)) if r["rc_tx"][i] != 0]
    groups = {}
    for i, c in enumerate(cases):
        if r["rc_tx"][i] == 0:
            groups.setdefault((c["fft"], c["n_rb"], c["n_ant"], c["n_sym"]), []).append(i)
    n_pass, n_fail, n_run = {mode: 0 for mode in both_modes()}, {mode: 0 for mode in both_modes()}, 0
    for key, idx in groups.items():
        c0 = cases[idx[0]]
        n_ant, n = c0["n_ant"], len(idx)
        cfg = m.DlCfg(c0["fft"], c0["n_rb"], n_ant, m.IQ_I8)
        sfs = np.array([cases[i]["sf"] for i in idx], np.uint32)
        cells = np.array([cases[i]["cell"] for i in idx], np.uint32)
        allocs = [m.make_alloc(j, cases[i]["mod"], cases[i]["tbs"], cases[i]["prb0"], cases[i]["rnti"], cases[i]["rv"], cases[i]["tx_mode"], cases[i]["prb1"])
                  for j, i in enumerate(idx)]
        d_iq = ctx.to_device(np.ascontiguousarray(r["iq"][idx]).reshape(-1, 2))
        d_start = ctx.to_device((np.arange(n) * fz.UNIT_CAP).astype(np.uint64))
        d_sf, d_cell = ctx.to_device(sfs), ctx.to_device(cells)
        d_own = ctx.alloc(n * ctx.subframe_floats(n_ant) * 4)
        d_own.zero()
        plan = None
        try:
            ctx.dl_frontend_dev(cfg, d_iq, None, d_start, d_sf, d_cell, n, d_own)
            try:
                plan = ctx.pdsch_plan(cfg, c0["n_sym"], allocs)
            except m.MiLteError as ex:  # the plan names no allocation: find the refused ones
                assert "error -4" in str(ex), ex
                keep = []
                for j in range(n):
                    try:
                        ctx.pdsch_plan(cfg, c0["n_sym"], [allocs[j]]).close()
                        keep.append(j)
                    except m.MiLteError as ex1:
                        assert "error -4" in str(ex1), ex1
                        skipped.append(("unsupported", idx[j], cases[idx[j]]["tbs"]))
                allocs = [allocs[j] for j in keep]
                if not allocs:
                    continue
                plan = ctx.pdsch_plan(cfg, c0["n_sym"], allocs)
            soft = None
            for mode in both_modes():
                plan.set_decoder(mode, N_ITER, 0)
                st, bits = plan.run(d_own, sfs, cells)
                if soft is None:
                    soft = [plan.soft_bits(a) for a in range(len(allocs))]
                check(port, allocs, soft, st, bits, mode, what=("sweep", key))
                n_pass[mode] += int((st == 0).sum())
                n_fail[mode] += int((st == 2).sum())
            n_run += len(allocs)
        finally:
            if plan is not None:
                plan.close()
            for b in (d_iq, d_start, d_sf, d_cell, d_own):
                b.free()
    print("sweep: %d cases run, skipped %s, passes %s, failures %s, reference transmitter %.1f s, all %.1f s"
          % (n_run, skipped, list(n_pass.values()), list(n_fail.values()), t_ref, time.time() - t_start))
    assert len(skipped) <= SWEEP_N // 50 and n_run == SWEEP_N - len(skipped), skipped
    for mode in both_modes():
        assert n_pass[mode] >= 20 and n_fail[mode] >= 20 and n_pass[mode] + n_fail[mode] == n_run, (mode, n_pass[mode], n_fail[mode])

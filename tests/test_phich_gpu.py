"""k_phich_decode (openlte_amd/csrc/phich.hip) against the float64 model of tests/phich_model.py, which restates the "PHICH, 3GPP mode"
section of include/mi_lte.h: metric, the three repetitions and P_tot within 1e-4 (the bound of the project's other float32-against-float64
pins), every decision on a present indicator equal; memory guards and repeatability; a cell the plan does not know; every refusal; and the
library's own transmitter through the real front end, PDCCH and PHICH decoded from the same device subframes.

Largest differences measured over all fifteen parameter sets (MI355X): see DESIGN.md, "PHICH"."""
import ctypes as C

import numpy as np
import pytest

import phich_cases as pc
import phich_model as pm

pytestmark = pytest.mark.gpu

TOL = 1e-4


class _At:
    """a device address inside a DeviceBuffer"""

    def __init__(self, buf, offset):
        self.ptr = buf.ptr + offset


def _units(ctx, cells, sfs):
    return ctx.to_device(np.asarray(sfs, np.uint32)), ctx.to_device(np.asarray(cells, np.uint32))


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_kernel_against_model(ctx, case):
    import openlte_amd as m
    present, hi, sub, model = pc.make(case)
    n_units, n_grp = present.shape[0], present.shape[1]
    cfg = m.DlCfg(pc.FFT[case["n_rb"]], case["n_rb"], case["n_ant"], 0)
    plan = ctx.phich_plan(cfg, sorted(set(case["cells"])), phich_res=float(case["n_g"]))
    assert plan.n_group == n_grp == m.phich_n_group(case["n_rb"], float(case["n_g"]))
    d_sub = ctx.to_device(sub)
    d_sf, d_cell = _units(ctx, case["cells"], case["sfs"])
    out = plan.decode_dev(d_sub, d_sf, d_cell, n_units)
    for b in (d_sub, d_sf, d_cell):
        b.free()
    plan.close()
    assert out.shape == (n_units, n_grp, 8)
    worst = dict(metric=0.0, rep=0.0, power=0.0)
    for u in range(n_units):
        metric, power, rep, dec = model[u]
        worst["metric"] = max(worst["metric"], np.abs(out["metric"][u] - metric).max())
        worst["rep"] = max(worst["rep"], np.abs(out["rep"][u] - rep).max())
        worst["power"] = max(worst["power"], np.abs(out["power"][u] / power[:, None] - 1.0).max())
    print("phich %s: max |metric - model| %.3g, max |rep - model| %.3g, max |power / model - 1| %.3g" % (pc.case_id(case), worst["metric"], worst["rep"], worst["power"]))
    assert worst["metric"] <= TOL and worst["rep"] <= TOL and worst["power"] <= TOL
    for u in range(n_units):
        metric, power, rep, dec = model[u]
        on = present[u] == 1
        assert np.array_equal(out["hi"][u][on], dec[on]) and np.array_equal(out["hi"][u][on], hi[u][on])  # every present indicator, nothing left out
        far = ~on & (np.abs(metric) >= TOL)
        assert np.array_equal(out["hi"][u][far], dec[far])
        assert np.array_equal(out["hi"][u], (out["metric"][u] < 0).astype(np.uint32))
        assert not out["flags"][u].any() and not out["reserved"][u].any()


@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[-1]], ids=pc.case_id)
def test_guard_records_stay_untouched_and_two_runs_give_the_same_bytes(ctx, case):
    """One group on one port and 25 groups on four: the records land exactly in [n_units][N_group][8]; 16 guard records before and after
    keep their pattern; a second run into a second buffer gives identical bytes."""
    import openlte_amd as m
    present, hi, sub, model = pc.make(case)
    n_units, n_grp = present.shape[0], present.shape[1]
    cfg = m.DlCfg(pc.FFT[case["n_rb"]], case["n_rb"], case["n_ant"], 0)
    plan = ctx.phich_plan(cfg, sorted(set(case["cells"])), phich_res=float(case["n_g"]))
    d_sub = ctx.to_device(sub)
    d_sf, d_cell = _units(ctx, case["cells"], case["sfs"])
    guard, body = 16 * 32, plan.out_bytes(n_units)
    assert body == 32 * n_units * n_grp * 8
    runs = []
    for fill in (0xA5, 0x5A):
        buf = ctx.to_device(np.full(guard + body + guard, fill, np.uint8))
        assert plan.decode_dev(d_sub, d_sf, d_cell, n_units, d_out=_At(buf, guard)) is None
        ctx.sync()
        got = buf.download(np.uint8)
        buf.free()
        assert (got[:guard] == fill).all() and (got[guard + body:] == fill).all()
        runs.append(got[guard:guard + body].copy())
    for b in (d_sub, d_sf, d_cell):
        b.free()
    plan.close()
    assert np.array_equal(runs[0], runs[1])
    rec = runs[0].view(np.dtype(m.PhichResult)).reshape(n_units, n_grp, 8)
    assert np.abs(rec["metric"][0] - model[0][0]).max() <= TOL


def test_unknown_cell_gives_flagged_zero_records_and_leaves_the_other_units_alone(ctx):
    import openlte_amd as m
    case = next(c for c in pc.CASES if c["n_rb"] == 25 and c["n_ant"] == 2)
    present, hi, sub, model = pc.make(case)
    n_units, n_grp = present.shape[0], present.shape[1]
    cfg = m.DlCfg(512, 25, 2, 0)
    d_sub = ctx.to_device(sub)
    d_sf, d_cell = _units(ctx, case["cells"], case["sfs"])
    sf10 = list(case["sfs"])
    sf10[1] = 10  # a subframe number the scrambler has no meaning for: refused like an unknown cell
    d_sf10 = ctx.to_device(np.asarray(sf10, np.uint32))
    full = ctx.phich_plan(cfg, sorted(set(case["cells"])), phich_res=1.0)
    want = full.decode_dev(d_sub, d_sf, d_cell, n_units)
    got10 = full.decode_dev(d_sub, d_sf10, d_cell, n_units)
    full.close()
    part = ctx.phich_plan(cfg, [c for c in sorted(set(case["cells"])) if c != case["cells"][1]], phich_res=1.0)
    got = part.decode_dev(d_sub, d_sf, d_cell, n_units)
    part.close()
    for b in (d_sub, d_sf, d_cell, d_sf10):
        b.free()
    assert not want["flags"].any() and np.abs(want["metric"][1] - model[1][0]).max() <= TOL
    for g in (got, got10):
        assert (g["flags"][1] == m.PHICH_UNKNOWN_CELL).all()
        for f in ("metric", "power", "hi", "reserved"):
            assert not g[f][1].any()
        assert not g["rep"][1].any()
        for u in (0, 2, 3):
            assert g[u].tobytes() == want[u].tobytes()


def test_every_refusal_returns_its_code_without_a_launch(ctx):
    import openlte_amd as m
    L, E = ctx.L, -1  # MI_LTE_ERR_INVALID_ARG
    cells = np.array([3, 100], np.uint32)
    h = C.c_void_p()

    def create(cfg=None, res=1.0, dur=0, flags=0, cl=cells, n=2, ctx_h=ctx.h, out=C.byref(h), null_cfg=False):
        cfg = m.DlCfg(512, 25, 1, 0) if cfg is None else cfg
        return L.mi_lte_phich_plan_create(ctx_h, None if null_cfg else C.byref(cfg), res, dur, flags, cl, n, out)
    ctx.profile(True)
    assert create(ctx_h=None) == E and create(null_cfg=True) == E and create(n=0) == E and create(out=None) == E
    raw = C.CDLL(m.library_path()).mi_lte_phich_plan_create  # (no argument types: a null cell list can be passed)
    assert raw(ctx.h, C.byref(m.DlCfg(512, 25, 1, 0)), C.c_float(1.0), 0, 0, None, 2, C.byref(h)) == E
    for kw in (dict(cfg=m.DlCfg(512, 26, 1, 0)), dict(cfg=m.DlCfg(512, 25, 3, 0)), dict(res=0.0), dict(res=2.5), dict(res=float("nan")), dict(dur=1),
               dict(cfg=m.DlCfg(512, 25, 1, m.CE_COMPACT)), dict(flags=1)):
        assert create(**kw) == E, kw
        assert "PHICH plan" in L.mi_lte_last_error(ctx.h).decode()
    assert create(cl=np.array([3, 504], np.uint32)) == E
    assert not h.value
    plan = ctx.phich_plan(m.DlCfg(512, 25, 1, 0), [3, 100])
    d_sub = ctx.to_device(np.zeros((2, 4, 16, 1200), np.float32))
    d_sf, d_cell = _units(ctx, [3, 100], [0, 9])
    d_out = ctx.alloc(plan.out_bytes(2))
    run = L.mi_lte_phich_decode_run
    ok = (ctx.h, plan.h, d_sub.ptr, d_sf.ptr, d_cell.ptr, 2, d_out.ptr)
    for i in (0, 1, 2, 3, 4, 6):
        assert run(*[None if j == i else a for j, a in enumerate(ok)]) == E, i
    assert run(*ok[:5], 0, ok[6]) == E
    assert "k_phich_decode" not in ctx.profile_report()
    # all-zero subframes: P_tot = 0, flagged, everything zero
    assert run(*ok) == 0
    assert ctx.profile_report()["k_phich_decode"][0] == 1 and ctx.last_kernels() == "k_phich_decode:1"
    ctx.profile(False)
    rec = d_out.download(np.uint8).view(np.dtype(m.PhichResult))
    assert (rec["flags"] == m.PHICH_NO_POWER).all() and not rec["metric"].any() and not rec["rep"].any() and not rec["power"].any() and not rec["hi"].any()
    for b in (d_sub, d_sf, d_cell, d_out):
        b.free()
    plan.close()


def test_own_transmitter_through_the_front_end_with_the_pdcch(ctx):
    """One 25-RB, one-port subframe from the library's transmit functions -- CRS, PCFICH (CFI 2), PHICH with three of four groups filled (one
    with all eight sequences), one DCI 1A for the SI-RNTI -- as float samples through the downlink front end on the device.  On the same
    device subframe mi_lte_pdcch_decode_run finds the CFI and the DCI and the PHICH plan returns every indicator sent; what was not sent
    stays below 0.25."""
    import openlte_amd as m
    fft, nrb, cell, sf, cfi = 512, 25, 44, 3, 2
    n_grp = m.phich_n_group(nrb, 1.0)
    regs = [n for g in range(n_grp) for n in pm.group_regs(nrb, cell, g)]
    assert n_grp == 4 and len(set(regs)) == 12 and not set(regs) & {int(x + 0.5) for x in pm.pcfich_reg_numbers(nrb, cell)}  # (a cell whose REGs do not collide)
    rng = np.random.default_rng(2025)
    present, hi = pm.random_pattern(rng, 1, n_grp)
    present[0, 2, :] = 0
    present[0, 3, :] = [1, 0, 0, 0, 1, 0, 0, 0]  # sequences n and n + 4 of one group
    hi[0, 3, 0], hi[0, 3, 4] = 1, 0
    dci = m.TxAlloc()
    dci.chan_type, dci.rnti, dci.N_prb, dci.mcs, dci.rv_idx = 0, 0xFFFF, 4, 5, 0
    for s in range(2):
        for i in range(4):
            dci.prb[s][i] = 2 + i
    t = m.Transmitter(fft, nrb, cell)
    t.signals(sf)
    _, ph, n_symbs = t.control(sf, cfi, n_grp, present[0], hi[0], dcis=[dci])
    assert n_symbs == cfi and ph.N_reg == 12
    i0, q0 = t.samples()
    t.clear()
    t.signals(sf + 1)  # (the estimator's last symbols look at the next subframe's first reference symbol)
    i1, q1 = t.samples()
    t.close()
    per = len(i0)
    i_all = np.concatenate([i0, i1, np.zeros(per, np.float32)]) * np.float32(0.02)
    q_all = np.concatenate([q0, q1, np.zeros(per, np.float32)]) * np.float32(0.02)
    cfg = m.DlCfg(fft, nrb, 1, 0)
    sub = ctx.dl_frontend(cfg, (i_all, q_all), [0], [sf], [cell])
    d_sub = ctx.to_device(sub.astype(np.float32))
    d_sf, d_cell = _units(ctx, [cell], [sf])
    pd = ctx.pdcch_plan(cfg, [cell], phich_res=1.0)
    rc, got_cfi, nsym, dcis = pd.decode_dev(d_sub, d_sf, d_cell, 1)
    pd.close()
    plan = ctx.phich_plan(cfg, [cell], phich_res=1.0)
    out = plan.decode_dev(d_sub, d_sf, d_cell, 1)
    plan.close()
    for b in (d_sub, d_sf, d_cell):
        b.free()
    # (the aggregation-8 candidate that holds the DCI's four CCEs decodes it as well, in the reference as here: the first is candidate 0)
    assert got_cfi[0] == cfi and nsym[0] == cfi and len(dcis[0]) >= 1 and all(d.rnti == 0xFFFF and d.format == 0 for d in dcis[0]) and dcis[0][0].candidate == 0
    assert dcis[0][0].alloc.N_prb == 4 and dcis[0][0].alloc.prb[0][0] == 2 and dcis[0][0].mcs == 5
    on = present[0] == 1
    print("phich through the front end: present |metric| %.4f .. %.4f, absent |metric| <= %.4f" % (np.abs(out["metric"][0][on]).min(), np.abs(out["metric"][0][on]).max(),
                                                                                                   np.abs(out["metric"][0][~on]).max()))
    assert np.array_equal(out["hi"][0][on], hi[0][on])
    assert np.abs(out["metric"][0][on]).min() > 0.5 and np.abs(out["metric"][0][~on]).max() < 0.25
    assert not out["flags"].any()

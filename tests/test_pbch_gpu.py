"""GPU parity: PBCH decoding (HIP) vs the compiled reference's liblte_phy_bch_channel_decode (rest of SURVEY 8f N3).
Exact: same grids and estimates in, integer soft values from the de-mapper on; the port count, the position in the 40 ms period
and the 24 MIB bits must be equal -- also where the decode fails or, at low SNR, succeeds on a wrong hypothesis."""
import os

import numpy as np
import pytest

import lte_testdata as td

pytestmark = pytest.mark.gpu


def run_case(ctx, case):
    import openlte_amd as m
    cfg = m.DlCfg(case["fft"], case["nrb"], 4, 0)
    n = len(case["units"])
    d_g = ctx.to_device(np.ascontiguousarray(case["grids"], np.float32))
    d_cell = ctx.to_device(np.array([c for c, _ in case["units"]], np.uint32))
    try:
        na, off, mib = ctx.pbch_decode_dev(cfg, d_g, d_cell, n)
    finally:
        d_g.free()
        d_cell.free()
    return np.stack([np.where(na == 0, 2, 0).astype(np.uint32), na, off, mib], axis=1)


@pytest.mark.parametrize("name", list(td.PBCH_CASES))
def test_pbch_matches_reference(ctx, ref, name):
    case = td.pbch_case(ref, name)
    want = td.ref_pbch_decode(ref, case)
    got = run_case(ctx, case)
    assert got.tolist() == want.tolist(), name
    if name != "15MHz_noisy":  # at a workable SNR: the transmitted port count, SFN mod 4 and MIB come back
        for u, (cell, sfn) in enumerate(case["units"]):
            assert got[u, 0] == 0 and got[u, 1] == case["n_ant"] and got[u, 2] == sfn % 4
            assert got[u, 3] == int("".join(str(int(b)) for b in case["mibs"][u]), 2)
    else:
        assert 0 < int((got[:, 0] == 0).sum())


def test_pbch_golden_fixture(ctx):
    """Against outputs of the reference recorded by tools/gen_golden.py (no oracle at run time)."""
    g = td.load_golden("pbch_ref")
    for name in [str(x) for x in g["names"]]:
        fft, nrb = [int(x) for x in g[name + "_cfg"]]
        grids = np.zeros((len(g[name + "_cells"]), 10, 16, 1200), np.float32)
        grids[:, :, 7:11, :] = g[name + "_grids"]
        case = dict(fft=fft, nrb=nrb, units=[(int(c), 0) for c in g[name + "_cells"]], grids=grids)
        assert run_case(ctx, case).tolist() == g[name + "_want"].tolist(), name


def test_pbch_requires_four_estimate_planes(ctx):
    import openlte_amd as m
    d = ctx.alloc(1024)
    with pytest.raises(m.MiLteError):
        ctx.pbch_decode_dev(m.DlCfg(2048, 100, 1, 0), d, d, 1)
    d.free()

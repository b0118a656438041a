"""GPU: the max-log PDSCH demapper (k_pdsch_demod_llr<1 | 2 | 4>) over the drawn geometry of tests/demap_geometry_cases.py -- the counterpart of
tests/test_fuzz_gpu.py for the one demodulator the compiled reference cannot check.  Seeded synthetic estimate planes go straight to the
device (no generator, no front end); on all six bandwidths and 1 / 2 / 4 ports, with PRB lists that differ between the slots or do not ascend,
every CRS shift, control regions up to 4 symbols and plans on both sides of the 32 KiB that switches every allocation from LDS assembly to
direct stores: e_len is the reference loop's count (fuzz_cases.re_count), the bytes and gains are the float64 model's by
test_demap_llr_gpu.check_against_model's rules, and nothing outside an allocation's bytes moves."""
import numpy as np
import pytest

import demap_geometry_cases as gc
import demap_llr_model as dm
from fuzz_cases import re_count
from test_demap_llr_gpu import check_against_model, slots
from test_harq_gpu import decode

pytestmark = pytest.mark.gpu

N_SOFT = 1237248


class Units:
    """A draw on the device, with what test_harq_gpu.decode and check_against_model read of a transmission"""

    def __init__(self, ctx, n_ant, drawn):
        self.ctx = ctx
        self.cfi, self.sfs, self.cells, self.allocs, planes = drawn
        assert ctx.subframe_floats(n_ant) == planes[0].size
        self.d_sub = ctx.to_device(planes)
        self.d_sf, self.d_cell = ctx.to_device(np.asarray(self.sfs, np.uint32)), ctx.to_device(np.asarray(self.cells, np.uint32))

    def free(self):
        for b in (self.d_sf, self.d_cell, self.d_sub):
            b.free()


@pytest.mark.parametrize("param", gc.PARAMS, ids=gc.param_id)
def test_drawn_geometry_against_the_model(ctx, param):
    """The default demapper first (its e_len against re_count, its slots recorded), then MAXLOG under the automatic gain and under a fixed one
    of 1.5 x the median automatic gain on the same plan: the model's bytes and gains, a clamped and a graded byte, e_len unchanged, and every
    slot beyond its allocation's bytes as the default run left it -- from the next multiple of 16 where the allocation is assembled in LDS and
    leaves in 16-byte stores, from e_len itself in the "direct_min" plans, whose allocations are all stored directly."""
    import openlte_amd as m
    n_rb, n_ant, variant, seed = param
    drawn = gc.draw(*param)
    t = Units(ctx, n_ant, drawn)
    cfg = m.DlCfg(gc.FFT[n_rb], n_rb, n_ant, 0)
    plan = ctx.pdsch_plan_3gpp(cfg, t.cfi, t.allocs, N_SOFT) if n_ant == 1 else ctx.pdsch_plan_3gpp_txdiv(cfg, t.cfi, t.allocs, N_SOFT)
    direct = gc.plan_e_bytes(t.allocs, t.cfi) > 32 * 1024
    assert direct == (variant == "direct_min")
    decode(t, plan)
    assert ctx.last_kernels().startswith("k_pdsch_demod:1,")
    ref_len, ref_slots = [len(plan.soft_bits(a)) for a in range(plan.n_alloc)], slots(plan, t.allocs, t.cfi)
    for a, al in enumerate(t.allocs):
        p0, p1 = gc.prb_lists(al)
        n_re = re_count(n_rb, n_ant, t.cells[al.unit], t.sfs[al.unit], al.n_pdcch_symbs or t.cfi, p0, p1)
        assert ref_len[a] == dm.QM[al.mod_type] * n_ant * (n_re // n_ant) > 0, (a, ref_len[a], n_re, p0, p1)
    auto = gc.model_of(drawn, n_rb, n_ant, 0.0, m.DEMAP_AUTO_T)
    fixed = float(np.float32(1.5 * np.median([r.gain for r in auto])))
    label = "k_pdsch_demod_llr:1," if n_ant == 1 else "k_pdsch_demod_llr_txd:1,"
    for gain in (0.0, fixed):
        plan.set_demapper(m.DEMAP_MAXLOG, gain)
        decode(t, plan)
        assert ctx.last_kernels().startswith(label + "k_dl3_desc:1,")
        e = check_against_model(plan, t, auto if gain == 0 else gc.model_of(drawn, n_rb, n_ant, gain, m.DEMAP_AUTO_T), gain)
        assert (np.abs(e) == 127).any() and (np.abs(e) < 127).any()
        got = slots(plan, t.allocs, t.cfi)
        for a in range(plan.n_alloc):
            n = len(plan.soft_bits(a))
            assert n == ref_len[a], a
            keep = n if direct else (n + 15) & ~15
            assert (got[a][keep:] == ref_slots[a][keep:]).all(), a
    plan.close()
    t.free()

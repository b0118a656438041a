"""CPU: what test_pusch_predecode_gpu.py rests on, with no kernel in the loop.  The builder's cases keep the float64 model of the DMRS
estimate (pusch_demod_model.h_polar) well conditioned; the 74 planned transform sizes reach every radix in every position the kernel has code
for, every prime of the generic pass, and all four symbol-group shapes; the model's transform has the sign, the scale and the conjugate of
36.211 5.3.3 on a hand-made case; and a float32 restatement of the kernel's Stockham plan, against numpy's float64 FFT on the tests' own
inputs, gives the error a float32 transform of these sizes costs -- the figure the GPU tests' tight gate is a multiple of."""
import numpy as np

import pusch_demod_cases as pc
import pusch_demod_model as pm


def test_planned_sizes_are_the_plans_envelope():
    """1, and every N_prb below the cell's 100 divisible by 2, 3 or 5: 74 sizes"""
    sizes = pc.planned_sizes()
    assert len(sizes) == 74 and sizes[0] == 1 and sizes[-1] == 99 and sizes == sorted(set(sizes))
    assert all(n == 1 or n % 2 == 0 or n % 3 == 0 or n % 5 == 0 for n in sizes)
    assert not [n for n in range(2, 100) if n not in sizes and (n % 2 == 0 or n % 3 == 0 or n % 5 == 0)]


def test_conditioning_of_every_case():
    """Every size and builder seed, on the float64 model alone: the smallest interpolated |h_s[k]| is >= 0.5 (the builder's magnitudes
    extrapolate to >= 0.8 - 3 * 0.45 / 7 = 0.607), the slot-to-slot phase step |7 f_ang| is <= 2.6 rad (so 0.5 rad inside the wrap at +-pi,
    where float32 and float64 could decide differently), PRB runs start at a non-zero PRB and stay inside the carrier, and the data rows are
    independent draws of unit variance."""
    worst_h, worst_step = np.inf, 0.0
    for seed in pc.SEEDS:
        for n in pc.planned_sizes():
            c = pc.case(n, seed)
            assert c.planes.shape == (2, 16, pm.N_SC) and c.planes.dtype == np.float32 and np.isfinite(c.planes).all()
            for b in range(2):
                run = [int(c.al.prb[b][i]) for i in range(n)]
                assert run[0] > 0 and run == list(range(run[0], run[0] + n)) and run[-1] < pc.N_RB, (n, b, run)
            h = pm.h_polar(c.planes, c.al, c.dmrs)
            t = []
            for b, L in ((0, 3), (1, 10)):
                sc = pm.subcarriers(c.al, b)
                y = c.planes[0, L, sc].astype(np.float64) + 1j * c.planes[1, L, sc].astype(np.float64)
                t.append(y * np.conj(c.dmrs[2 * b].astype(np.float64) + 1j * c.dmrs[2 * b + 1].astype(np.float64)))
            step = np.angle(t[1]) - np.angle(t[0])
            step = np.where(step >= np.pi, step - 2 * np.pi, np.where(step <= -np.pi, step + 2 * np.pi, step))  # = 7 f_ang of h_polar
            assert np.abs(h).min() >= 0.5, (n, seed, np.abs(h).min())
            assert np.abs(step).max() <= 2.6, (n, seed, np.abs(step).max())
            # the interpolation passes through both estimates: h one step either side of DMRS symbol b brackets t_b
            for b in range(2):
                assert np.allclose(0.5 * (np.abs(h[6 * b + 2]) + np.abs(h[6 * b + 3])), np.abs(t[b]), rtol=1e-12), (n, seed, b)
            worst_h, worst_step = min(worst_h, float(np.abs(h).min())), max(worst_step, float(np.abs(step).max()))
            rows = c.planes[0, pm.data_rows()].astype(np.float64) + 1j * c.planes[1, pm.data_rows()].astype(np.float64)
            assert 0.9 < (np.abs(rows) ** 2).mean() < 1.1, (n, seed)
            assert all((rows[i] != rows[k]).all() for i in range(12) for k in range(i))
    print("conditioning over %d sizes x %d seeds: smallest |h| %.4f, largest phase step %.4f rad" % (len(pc.planned_sizes()), len(pc.SEEDS), worst_h, worst_step))


def test_radix_plan_is_a_factorisation_in_the_kernels_order():
    """every plan multiplies to M, Ns is the product of the radices before it, the fixed radices come in the order 9, 3, 5, 8, 4, 2 and the
    primes behind them in ascending order"""
    order = {R: i for i, R in enumerate(pc.FIXED_RADICES)}
    for n in range(1, 111):
        plan, Ns = pc.radix_plan(n), 1
        for R, ns in plan:
            assert ns == Ns and (R in order or (R >= 7 and all(R % d for d in range(2, R)))), (n, plan)
            Ns *= R
        assert Ns == 12 * n, (n, plan)
        rank = [order.get(R, 100 + R) for R, _ in plan]
        assert rank == sorted(rank), (n, plan)
    assert pc.radix_plan(1) == [(3, 1), (4, 3)] and pc.radix_plan(6) == [(9, 1), (8, 9)]
    assert pc.radix_plan(98) == [(3, 1), (8, 3), (7, 24), (7, 168)] and pc.radix_plan(94) == [(3, 1), (8, 3), (47, 24)]


def test_the_planned_sizes_cover_every_radix_position_prime_and_shape():
    """Coverage as a checked claim.  At most 4 passes (the table has room for 6); 3 and 9 each open a plan; each of 9, 3, 5, 8, 4, 2 and
    the generic pass runs in a later position (Ns > 1: with twiddles); the generic pass runs with every prime from 7 to 47 and twice in one
    plan (98 PRB); the four S_par classes hold 13 / 14 / 26 / 21 sizes with largest members 16 / 35 / 70 / 99 PRB; and the sizes that run
    alone at 192 threads are 1 .. 8 PRB."""
    sizes = pc.planned_sizes()
    plans = {n: pc.radix_plan(n) for n in sizes}
    assert max(len(p) for p in plans.values()) == 4
    first = {p[0][0] for p in plans.values()}
    assert first == {3, 9}
    later = {(R if R in pc.FIXED_RADICES else "prime") for p in plans.values() for R, _ in p[1:]}
    assert later == set(pc.FIXED_RADICES) | {"prime"}, later
    primes = {R for p in plans.values() for R, _ in p if R not in pc.FIXED_RADICES}
    assert primes == {7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47}, primes
    twice = [n for n, p in plans.items() if sum(R not in pc.FIXED_RADICES for R, _ in p) == 2]
    assert twice == [98], twice
    classes = {S: [n for n in sizes if pc.s_par(12 * n) == S] for S in (12, 6, 3, 2)}
    assert sum(len(v) for v in classes.values()) == 74
    assert [len(classes[S]) for S in (12, 6, 3, 2)] == [13, 14, 26, 21]
    assert [classes[S][-1] for S in (12, 6, 3, 2)] == [16, 35, 70, 99]
    assert [n for n in sizes if pc.threads(12 * n) == 192] == [1, 2, 3, 4, 5, 6, 8]
    for S, v in classes.items():
        print("S_par %2d: %s" % (S, v))
    print("first radices %s; later positions %s; primes of the generic pass %s; twice in %s" % (sorted(first), sorted(map(str, later)), sorted(primes), twice))


def test_convention_sign_scale_and_conjugate():
    """A hand-made case: random QPSK points d on every data symbol, a flat channel h per slot, the rows z = sqrt(M) fft(d) / M h (the
    transmitter's transform precoding, 36.211 5.3.3, through the channel) and DMRS rows whose estimate is h.  equalise_predecode returns d to 1e-12:
    the backward transform, the 1 / sqrt(M) factor, the conjugate of the estimate and the row of every data symbol, tied to numpy's fft and
    not to the kernel."""
    rng = np.random.default_rng(5)
    for n in (1, 6, 35):
        c = pc.case(n, 0)
        M = c.M
        d = ((2 * rng.integers(0, 2, (12, M)) - 1) + 1j * (2 * rng.integers(0, 2, (12, M)) - 1)) / np.sqrt(2.0)
        h = 0.9 * np.exp(0.7j)
        g = np.zeros((16, pm.N_SC), np.complex128)
        for s, L in enumerate(pm.data_rows()):
            g[L, pm.subcarriers(c.al, s // 6)] = np.sqrt(M) * np.fft.fft(d[s]) / M * h
        for b, L in ((0, 3), (1, 10)):
            r = c.dmrs[2 * b].astype(np.float64) + 1j * c.dmrs[2 * b + 1].astype(np.float64)
            g[L, pm.subcarriers(c.al, b)] = h * r / np.abs(r) ** 2  # (|r| is 1 to float32 only: 1e-7 would hide behind it)
        x = pm.equalise_predecode(np.stack([g.real, g.imag]), c.al, c.dmrs)
        assert x.shape == (12, M) and np.abs(x - d).max() <= 1e-12, (n, np.abs(x - d).max())


def test_float32_restatement_is_the_transform():
    """stockham_f32 on the kernel's radix plan computes the backward DFT at every planned size (to float32 accuracy, on an impulse and on a
    single tone, whose transforms are known in closed form)"""
    for n in pc.planned_sizes():
        M = 12 * n
        z = np.zeros((2, M), np.complex128)
        z[0, 5 % M] = 1.0                                        # impulse at 5: exp(+2 pi i 5 q / M)
        z[1] = np.exp(-2j * np.pi * 7 * np.arange(M) / M)        # tone -7: M at q = 7, 0 elsewhere
        re, im = pc.stockham_f32(z, n)
        got = re.astype(np.float64) + 1j * im.astype(np.float64)
        want = np.stack([np.exp(2j * np.pi * (5 % M) * np.arange(M) / M), M * (np.arange(M) == 7 % M)])
        assert np.abs(got[0] - want[0]).max() < 1e-5, n
        assert np.abs(got[1] - want[1]).max() < 1e-5 * M, n


def test_float32_floor_and_the_gates_it_sets():
    """The float32 restatement against numpy's float64 FFT on the tests' own inputs, all 74 sizes and both seeds: the worst rel-L2 and the
    worst elementwise error over the symbol's RMS.  A float32 transform of up to four passes cannot be better than a few 2^-24 and must
    not be worse than 1e-6; the GPU gates are 8 x these figures, under the hard gates of 1e-5 and 1e-4."""
    fl = pc.float32_floor()
    assert sorted(fl) == sorted((n, s) for s in pc.SEEDS for n in pc.planned_sizes())
    l2 = max(fl, key=lambda k: fl[k][0])
    el = max(fl, key=lambda k: fl[k][1])
    g_l2, g_el = pc.gates()
    print("float32 floor: worst rel-L2 %.3g at %d PRB, worst elementwise / RMS %.3g at %d PRB; gates %.3g and %.3g" % (fl[l2][0], l2[0], fl[el][0 + 1], el[0], g_l2, g_el))
    for S in (12, 6, 3, 2):
        v = [fl[k] for k in fl if pc.s_par(12 * k[0]) == S]
        print("  S_par %2d: rel-L2 up to %.3g, elementwise up to %.3g" % (S, max(x[0] for x in v), max(x[1] for x in v)))
    v = [fl[k] for k in fl if any(R not in pc.FIXED_RADICES for R, _ in pc.radix_plan(k[0]))]
    print("  sizes with a generic pass: rel-L2 up to %.3g, elementwise up to %.3g" % (max(x[0] for x in v), max(x[1] for x in v)))
    assert 2.0 ** -24 < fl[l2][0] < 1e-6 and fl[el][1] < 1e-5
    assert g_l2 == pc.GATE_FACTOR * fl[l2][0] < pc.TOL_SYMB and g_el == pc.GATE_FACTOR * fl[el][1] < 10 * pc.TOL_SYMB

"""The PUSCH demodulator's launch rule (openlte_amd/csrc/pusch_launch.h: what pusch_run launches by and mi_lte_pusch_plan_set_rx_antennas
refuses by) against pusch_demod_model.launch, the Python restatement the GPU tests choose their sizes by, for all five families.
tools/asan/pusch_launch_driver.cc answers the queries under g++ -fsanitize=address,undefined (tools/asan/run_pusch_launch.sh).  No GPU,
nothing loaded into Python."""
import os
import subprocess

import pusch_demod_cases as pc
import pusch_demod_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = (64 * 1024, 160 * 1024)
OVERRIDES = (0, 64, 128, 192, 256)
# (maxlog, noise) per n_rx: the plain launch, the max-log launch and the noise-referenced one; combining with and without the noise gain
FAMILIES = {1: ((0, 0), (1, 0), (1, 1)), 2: ((1, 0), (1, 1)), 4: ((1, 0), (1, 1))}


def names(n_rx, maxlog, noise, mmse):
    """(family, label) of a launch by its settings"""
    if not maxlog:
        return "plain", "k_pusch_demod"
    if noise and mmse:
        return "llr_mmse", "k_pusch_demod_llr_mmse"
    return ("llr_rx", "k_pusch_demod_llr_rx") if n_rx > 1 else ("llr_noise" if noise else "llr", "k_pusch_demod_llr")


def ask(tmp_path, name, qs):
    """the driver's answers, split into fields, to the queries qs = [(n_rx, n_prb, Q_m, maxlog, noise, mmse, limit, override)].  No
    sanitizer report."""
    assert len(set(qs)) == len(qs)
    path = str(tmp_path / name)
    with open(path, "w") as f:  # (the C++ words_max is W - 1: pusch_lds adds the slack word itself)
        f.writelines("%d %d %d %d %d %d %d %d\n" % (12 * n, pm.words(n, q) - 1, maxlog, noise, n_rx, limit, over, mmse)
                     for (n_rx, n, q, maxlog, noise, mmse, limit, over) in qs)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_pusch_launch.sh"), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "pusch launch driver: %d queries answered" % len(qs) in r.stderr, r.stderr[-1000:]
    out = [line.split() for line in r.stdout.splitlines()]
    assert len(out) == len(qs)
    return out


def check(qs, out):
    """Every answer -- fits or not, family, width, S_par, the bytes in front of the LLR block, the dynamic LDS, the label -- is
    pusch_demod_model.launch's, under the family and label its settings name; a combining or MMSE launch fits exactly where
    rx_s_par is not 0, and then within the limit; every launch that fits is one pusch_variant_compiled says is compiled.  Returns the
    (n_rx, limit) refused."""
    refused = set()
    for (n_rx, n, q, maxlog, noise, mmse, limit, over), line in zip(qs, out):
        M, W, what = 12 * n, pm.words(n, q), (n_rx, n, q, maxlog, noise, mmse, limit, over, line)
        fits, family, threads, S, lds_off, lds_bytes, label, compiled = line
        want = pm.launch(n_rx, M, W, maxlog, noise, mmse, limit, over)
        assert compiled == "1" or not want[0], what  # a launch that fits is a k_pusch_demod instantiation that exists (pusch_variant_compiled)
        assert (int(fits), family, int(threads), int(S), label) == (want[0], want[1], want[2], want[3], want[6]), what
        assert (family, label) == names(n_rx, maxlog, noise, mmse), what
        if n_rx == 1 or not maxlog:
            assert want[0] == 1 and want[2] == (over or pc.threads(M)) and want[3] == pc.s_par(M) and (maxlog or want[4] == 0), what
        else:
            assert want[2] == pm.threads(M) and want[3] == pm.rx_s_par(n_rx, M, W, limit) and want[0] == (want[3] != 0), what
        if want[0]:
            assert (int(lds_off), int(lds_bytes)) == (want[4], want[5]) and (n_rx == 1 or want[5] <= limit), what
        else:
            refused.add((n_rx, limit))
    return refused


def test_launch_rule_equals_the_python_restatements(tmp_path):
    """The full product without MMSE: n_rx x the 74 planned sizes (each alone as M_max) x Q_m x the families n_rx admits x LDS limits x
    width overrides."""
    qs = [(n_rx, n, q, maxlog, noise, 0, limit, over)
          for n_rx in (1, 2, 4) for n in pc.planned_sizes() for q in (2, 4, 6) for (maxlog, noise) in FAMILIES[n_rx] for limit in LIMITS for over in OVERRIDES]
    assert len(qs) == 74 * 3 * len(LIMITS) * len(OVERRIDES) * sum(len(f) for f in FAMILIES.values())
    # the refusal is exercised, not merely present: both antenna counts at 64 KiB, four antennas at the MI355X's 160 KiB, never two there
    assert check(qs, ask(tmp_path, "queries.txt", qs)) == {(2, LIMITS[0]), (4, LIMITS[0]), (4, LIMITS[1])}


def test_mmse_launch_equals_the_python_restatement(tmp_path):
    """All 74 planned sizes (each alone as M_max) x Q_m x n_rx 1 / 2 / 4 x both LDS limits x the width overrides, MAXLOG with the noise gain
    on and mmse = 1: the family is llr_mmse, and the refusal is the combining launch's."""
    qs = [(n_rx, n, q, 1, 1, 1, limit, over) for n_rx in (1, 2, 4) for n in pc.planned_sizes() for q in (2, 4, 6) for limit in LIMITS for over in OVERRIDES]
    assert len(qs) == 74 * 3 * 3 * len(LIMITS) * len(OVERRIDES)
    out = ask(tmp_path, "mmse.txt", qs)
    assert all(line[1] == "llr_mmse" for line in out)
    assert check(qs, out) == {(2, LIMITS[0]), (4, LIMITS[0]), (4, LIMITS[1])}


def test_mmse_off_is_the_seven_field_answer(tmp_path):
    """mmse = 1 without MAXLOG or without the noise gain (which the run function refuses before it asks): line for line what mmse = 0
    answers.  With MAXLOG and the noise gain, mmse = 1 changes the family and the label and nothing else."""
    qs = [(n_rx, n, q, maxlog, noise, 0, limit, over) for n_rx in (1, 2, 4) for n in pc.planned_sizes()[::3] for q in (2, 6)
          for (maxlog, noise) in FAMILIES[n_rx] for limit in LIMITS for over in OVERRIDES[:3]]
    base = ask(tmp_path, "off.txt", qs)
    on = ask(tmp_path, "on.txt", [k[:5] + (1,) + k[6:] for k in qs])
    n_mmse = 0
    for (n_rx, n, q, maxlog, noise, _, limit, over), fb, fo in zip(qs, base, on):
        if maxlog and noise:
            assert (fo[1], fo[6]) == ("llr_mmse", "k_pusch_demod_llr_mmse") and fo[0] == fb[0] and fo[2:6] == fb[2:6], (fb, fo)
            n_mmse += 1
        else:
            assert fo == fb, (fb, fo)
        assert fo[7] == "1" or fo[0] == "0", fo  # whatever fits is compiled, with mmse on as with it off
    assert n_mmse > 100

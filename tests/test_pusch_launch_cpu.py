"""The PUSCH demodulator's launch rule (openlte_amd/csrc/pusch_launch.h: what pusch_run launches by and mi_lte_pusch_plan_set_rx_antennas
refuses by) against the Python restatements the GPU tests choose their sizes by (pusch_predecode_cases.s_par / threads,
pusch_rxdiv_model.words / lds_bytes / s_par / threads).  tools/asan/pusch_launch_driver.cc answers the queries under
g++ -fsanitize=address,undefined.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pusch_predecode_cases as pc
import pusch_rxdiv_model as rxm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = (64 * 1024, 160 * 1024)
OVERRIDES = (0, 64, 128, 192, 256)
# (maxlog, noise) per n_rx: the plain launch, the max-log launch and the noise-referenced one; combining with and without the noise gain
FAMILIES = {1: ((0, 0), (1, 0), (1, 1)), 2: ((1, 0), (1, 1)), 4: ((1, 0), (1, 1))}


def queries():
    """the full product: n_rx x the 74 planned sizes (each alone as M_max) x Q_m x the families n_rx admits x LDS limits x width overrides"""
    return [(n_rx, n, q, maxlog, noise, limit, over)
            for n_rx in (1, 2, 4) for n in pc.planned_sizes() for q in (2, 4, 6) for (maxlog, noise) in FAMILIES[n_rx] for limit in LIMITS for over in OVERRIDES]


def test_launch_rule_equals_the_python_restatements(tmp_path):
    """Every answer of the C++ rule -- fits or not, family, width, S_par, the bytes in front of the LLR block, the dynamic LDS, the label --
    equals what the Python models give: the override or pc.threads for one antenna, rxm.threads whatever the override for a combining
    launch; pc.s_par for one antenna, rxm.s_par for combining, "does not fit" exactly where that is 0; rxm.lds_bytes for the combining and
    the single-antenna noise launch, 32 bytes less for the single-antenna max-log launch, 36 M + 8 M (1 + 2 S) + 4 W for the plain one.
    Every launch that fits is one pusch_variant_compiled says is compiled.  No sanitizer report."""
    qs = queries()
    assert len(qs) == 74 * 3 * len(LIMITS) * len(OVERRIDES) * sum(len(f) for f in FAMILIES.values()) and len(set(qs)) == len(qs)
    path = str(tmp_path / "queries.txt")
    with open(path, "w") as f:  # (the C++ words_max is W - 1: pusch_lds adds the slack word itself)
        f.writelines("%d %d %d %d %d %d %d\n" % (12 * n, rxm.words(n, q) - 1, maxlog, noise, n_rx, limit, over) for (n_rx, n, q, maxlog, noise, limit, over) in qs)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_pusch_launch.sh"), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "pusch launch driver: %d queries answered" % len(qs) in r.stderr, r.stderr[-1000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(qs)
    refused = set()
    for (n_rx, n, q, maxlog, noise, limit, over), line in zip(qs, lines):
        M, W, what = 12 * n, rxm.words(n, q), (n_rx, n, q, maxlog, noise, limit, over, line)
        fits, family, threads, S, lds_off, lds_bytes, label, compiled = line.split()
        fits, threads, S, lds_off, lds_bytes = int(fits), int(threads), int(S), int(lds_off), int(lds_bytes)
        assert compiled == "1" or not fits, what  # a launch that fits is a k_pusch_demod instantiation that exists (pusch_variant_compiled)
        if n_rx == 1:
            assert fits == 1 and threads == (over or pc.threads(M)) and S == pc.s_par(M), what
            if not maxlog:
                assert (family, label, lds_off) == ("plain", "k_pusch_demod", 0) and lds_bytes == 36 * M + 8 * M * (1 + 2 * S) + 4 * W, what
            else:
                assert (family, label) == ("llr_noise" if noise else "llr", "k_pusch_demod_llr"), what
                assert lds_bytes == rxm.lds_bytes(1, M, W, S) - (0 if noise else 32) and lds_off == rxm.lds_bytes(1, M, W, S) - rxm.LLR_BLOCK_BYTES, what
        else:
            want = rxm.s_par(n_rx, M, W, limit)
            assert (family, label) == ("llr_rx", "k_pusch_demod_llr_rx") and threads == rxm.threads(M) and S == want and fits == (want != 0), what
            if fits:
                assert lds_bytes == rxm.lds_bytes(n_rx, M, W, S) <= limit and lds_off == lds_bytes - rxm.LLR_BLOCK_BYTES, what
            else:
                refused.add((n_rx, limit))
    # the refusal is exercised, not merely present: both antenna counts at 64 KiB, four antennas at the MI355X's 160 KiB, never two there
    assert refused == {(2, LIMITS[0]), (4, LIMITS[0]), (4, LIMITS[1])}

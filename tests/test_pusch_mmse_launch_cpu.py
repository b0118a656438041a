"""The MMSE launch of the PUSCH demodulator's launch rule (openlte_amd/csrc/pusch_launch.h, the trailing `mmse` argument) against
pusch_mmse_model.launch, the restatement the GPU tests choose their sizes by: the noise-on launch of the same n_rx under the family
llr_mmse, and with mmse = 0 what the seven-field form answers.  tools/asan/pusch_launch_driver.cc's --mmse mode answers the queries under
g++ -fsanitize=address,undefined (tools/asan/run_pusch_launch_mmse.sh).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pusch_mmse_model as mm
import pusch_predecode_cases as pc
import pusch_rxdiv_model as rxm
from test_pusch_launch_cpu import FAMILIES, LIMITS, OVERRIDES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ask(tmp_path, name, script, lines):
    path = str(tmp_path / name)
    with open(path, "w") as f:
        f.writelines(lines)
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", script), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "pusch launch driver: %d queries answered" % len(lines) in r.stderr, r.stderr[-1000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def test_mmse_launch_equals_the_python_restatement(tmp_path):
    """All 74 planned sizes (each alone as M_max) x Q_m x n_rx 1 / 2 / 4 x both LDS limits x the width overrides, MAXLOG with the noise gain
    on and mmse = 1: fits, family llr_mmse, width, S_par, the bytes in front of the LLR block, the dynamic LDS and the label are
    pusch_mmse_model.launch's; the refusal is the combining launch's.  Every launch that fits is one pusch_variant_compiled says is
    compiled."""
    qs = [(n_rx, n, q, limit, over) for n_rx in (1, 2, 4) for n in pc.planned_sizes() for q in (2, 4, 6) for limit in LIMITS for over in OVERRIDES]
    assert len(qs) == 74 * 3 * 3 * len(LIMITS) * len(OVERRIDES)
    out = ask(tmp_path, "mmse.txt", "run_pusch_launch_mmse.sh",
              ["%d %d 1 1 %d %d %d 1\n" % (12 * n, rxm.words(n, q) - 1, n_rx, limit, over) for (n_rx, n, q, limit, over) in qs])
    refused = set()
    for (n_rx, n, q, limit, over), line in zip(qs, out):
        M, W, what = 12 * n, rxm.words(n, q), (n_rx, n, q, limit, over, line)
        fits, family, threads, S, lds_off, lds_bytes, label, compiled = line.split()
        want = mm.launch(n_rx, M, W, limit, over)
        assert compiled == "1" or not want[0], what  # a launch that fits is a k_pusch_demod instantiation that exists (pusch_variant_compiled)
        assert (int(fits), family, int(threads), int(S), label) == (want[0], want[1], want[2], want[3], want[6]), what
        if want[0]:
            assert (int(lds_off), int(lds_bytes)) == (want[4], want[5]) and (n_rx == 1 or want[5] <= limit), what
        else:
            refused.add((n_rx, limit))
    assert refused == {(2, LIMITS[0]), (4, LIMITS[0]), (4, LIMITS[1])}


def test_mmse_off_is_the_seven_field_answer(tmp_path):
    """mmse = 0, and mmse = 1 without MAXLOG or without the noise gain (which the run function refuses before it asks): line for line what
    the seven-field form answers.  With MAXLOG and the noise gain, mmse = 1 changes the family and the label and nothing else."""
    qs = [(n_rx, n, q, maxlog, noise, limit, over) for n_rx in (1, 2, 4) for n in pc.planned_sizes()[::3] for q in (2, 6)
          for (maxlog, noise) in FAMILIES[n_rx] for limit in LIMITS for over in OVERRIDES[:3]]
    seven = ["%d %d %d %d %d %d %d\n" % (12 * n, rxm.words(n, q) - 1, maxlog, noise, n_rx, limit, over) for (n_rx, n, q, maxlog, noise, limit, over) in qs]
    base = ask(tmp_path, "seven.txt", "run_pusch_launch.sh", seven)
    off = ask(tmp_path, "off.txt", "run_pusch_launch_mmse.sh", [s[:-1] + " 0\n" for s in seven])
    on = ask(tmp_path, "on.txt", "run_pusch_launch_mmse.sh", [s[:-1] + " 1\n" for s in seven])
    assert off == base
    n_mmse = 0
    for (n_rx, n, q, maxlog, noise, limit, over), b, o in zip(qs, base, on):
        if maxlog and noise:
            fb, fo = b.split(), o.split()
            assert (fo[1], fo[6]) == ("llr_mmse", "k_pusch_demod_llr_mmse") and fo[0] == fb[0] and fo[2:6] == fb[2:6], (b, o)
            n_mmse += 1
        else:
            assert o == b, (b, o)
        assert o.split()[7] == "1" or o.split()[0] == "0", o  # whatever fits is compiled, with mmse on as with it off
    assert n_mmse > 100

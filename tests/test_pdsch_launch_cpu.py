"""The PDSCH demodulators' launch rule (openlte_amd/csrc/pdsch_launch.h: what plan_layout accumulates and pdsch_demod launches by) against a
Python restatement written from the kernels' LDS layout -- tab[max_pairs + 1] (uint2) | cw[max_words + 1] | soft bits, each part rounded
to 16 bytes; the block 64-byte rounded and used up to 32 KiB; a packed run's block sized by the byte allocations, holding one mask byte per
symbol of the longest 16QAM / 64QAM one.  tools/asan/pdsch_launch_driver.cc answers the queries under g++ -fsanitize=address,undefined.
No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERRIDES = (0, 64, 100, 128, 192, 256, 320)  # 100 (no multiple of 64) and 320 (out of range) are ignored
# (n_ant, compact, maxlog, noise): the reference demapper, its compact form on one port, max-log with either gain
VARIANTS = [(n_ant, compact, maxlog, noise) for n_ant in (1, 2, 4)
            for (compact, maxlog, noise) in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 1)) if not compact or n_ant == 1]
QM = (1, 2, 4, 6)
STATIC_LDS = {"ref_one_port": 512, "ref_one_port_compact": 512, "ref_ports": 512, "llr": 32, "llr_noise": 32}  # qam_lut: uint2[64]; w_wave: double[4]
LONG_64QAM = (110, 1, 3)  # 17 160 symbols, 3218 words


def up(x, m):
    return -(-x // m) * m


def sizes(allocs):
    """(max_pairs, max_words, max_words_lo, max_symb_hi) of a plan's allocations (N_prb, control-region size, modulation)"""
    words = [-(-(14 - c) * n * 12 * QM[m] // 32) for (n, c, m) in allocs]
    return (max(14 * n for (n, c, m) in allocs), max(words), max([w for w, (n, c, m) in zip(words, allocs) if m < 2] or [0]),
            max([(14 - c) * n * 12 for (n, c, m) in allocs if m >= 2] or [0]))


def launch(sz, n_ant, compact, maxlog, noise, pack, gold, over):
    """the launch as the driver prints it, and the bytes the block is sized by"""
    max_pairs, max_words, words_lo, symb_hi = sz
    pack = pack and not maxlog  # (the max-log kernels have no packed form)
    pairs_al, words_al = up(2 * (max_pairs + 1), 4), up(max_words + 1, 4)
    e_bytes = up((words_lo if pack else max_words) * 32, 64)
    e_cap = e_bytes if e_bytes <= 32768 else 0
    family = ("llr_noise" if noise else "llr") if maxlog else "ref_ports" if n_ant > 1 else "ref_one_port_compact" if compact else "ref_one_port"
    threads = over if not maxlog and over in (64, 128, 192, 256) else 256
    label = "k_pdsch_demod" if not maxlog else "k_pdsch_demod_llr" if n_ant == 1 else "k_pdsch_demod_llr_txd"
    lds = 4 * (pairs_al + words_al) + max(e_cap, up(symb_hi, 16) if pack else 0)
    return "%d %d %d %d %s %d %d %d %d %d %d %d %s %d 1" % (max_pairs, max_words, words_lo, symb_hi, family, n_ant, threads, pairs_al, words_al, e_cap, lds,
                                                          (1 if pack else 0) | (2 if gold else 0), label, 1 if maxlog and noise else 0), e_bytes


def plans():
    """every single allocation; the long 64QAM allocation next to a QPSK one of 1024 words (105 PRB behind one control symbol: the block's
    32 KiB exactly) and its nearest allocations (1014, 1034 words); the sizes one word either side of the edge, which no allocation has, and
    the bound of pdsch_launch.h's static_assert, as raw sizes"""
    single = [[(n, c, m)] for n in range(1, 111) for c in range(1, 5) for m in range(4)]
    edge = [[LONG_64QAM, (n, 1, 1)] for n in (104, 105, 106)]
    assert [sizes(p)[2] for p in edge] == [1014, 1024, 1034]
    raw = [(1540, 3218, w, 17160) for w in (1023, 1024, 1025)] + [(1540, 4095, 1024, 17160), (1540, 4095, 0, 0)]
    return single + edge, raw


def test_launch_rule_equals_the_python_restatement(tmp_path):
    """Over the full product -- every plan of plans() x pack x the Gold-word method x ports and variants x width overrides -- every field of
    the C++ plan equals the restatement; the launch is one pdsch_variant_compiled admits; the dynamic LDS and the kernel's static arrays fit
    64 KiB; the soft-bit block starts 16-byte aligned; e_cap is a multiple of 64 and 0 exactly where the 64-byte rounded soft bits pass
    32 768 bytes; a packed run's block holds max_symb_hi bytes whatever e_cap is; the max-log launches are 256 wide whatever the override.
    The largest dynamic LDS is 48 656 bytes for one allocation and 57 984 with the 64QAM + 1024-word QPSK pair.  No sanitizer report."""
    allocs, raw = plans()
    settings = [(v, pack, gold, over) for v in VARIANTS for pack in (0, 1) for gold in (0, 1) for over in OVERRIDES]
    qs = [(p, sizes(p), s) for p in allocs for s in settings] + [(None, sz, s) for sz in raw for s in settings]
    assert len(qs) == (110 * 4 * 4 + 3 + 5) * 10 * 2 * 2 * len(OVERRIDES)
    path = str(tmp_path / "queries.txt")
    with open(path, "w") as f:
        for (p, sz, ((n_ant, compact, maxlog, noise), pack, gold, over)) in qs:
            head = "%d %s" % (len(p), " ".join("%d %d %d" % a for a in p)) if p else "0 %d %d %d %d" % sz
            f.write("%s %d %d %d %d %d %d %d\n" % (head, n_ant, compact, maxlog, noise, pack, gold, over))
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_pdsch_launch.sh"), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "pdsch launch driver: %d queries answered" % len(qs) in r.stderr, r.stderr[-1000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(qs)
    peak_one, peak, capped = 0, 0, set()
    for (p, sz, ((n_ant, compact, maxlog, noise), pack, gold, over)), line in zip(qs, lines):
        what = (p, sz, n_ant, compact, maxlog, noise, pack, gold, over, line)
        want, e_bytes = launch(sz, n_ant, compact, maxlog, noise, pack, gold, over)
        assert line == want, what  # every field, `compiled` among them
        got = line.split()
        family, threads, pairs_al, words_al, e_cap, lds, flags = got[4], int(got[6]), int(got[7]), int(got[8]), int(got[9]), int(got[10]), int(got[11])
        assert sz[1] <= 4095 and lds + STATIC_LDS[family] <= 65536, what
        assert (4 * (pairs_al + words_al)) % 16 == 0, what
        assert e_cap % 64 == 0 and (e_cap == 0) == (e_bytes > 32768 or e_bytes == 0) and e_cap in (0, e_bytes), what
        assert not (flags & 1) or lds - 4 * (pairs_al + words_al) >= sz[3], what
        assert not maxlog or threads == 256, what
        capped.add(e_cap == 0 and e_bytes > 0)
        peak = max(peak, lds)
        if p and len(p) == 1:
            peak_one = max(peak_one, lds)
    assert capped == {False, True}  # both sides of the 32 KiB rule are exercised
    assert peak_one == 48656
    assert max(int(l.split()[10]) for (p, sz, s), l in zip(qs, lines) if p) == 57984
    assert peak == 4 * (3084 + 4096) + 32768  # the raw worst case: pdsch_launch.h's static_assert

"""The host half of the PUSCH plans (openlte_amd/csrc/pusch_plan.h: pusch_plan_layout, pusch_alloc_check, pusch_nprb_planned) and of the 3GPP
transport-block mode's code-block slots (dlsch3_layout.h: mi_dlsch3_layout) against a Python restatement written from 36.211 5.3 / 5.5,
36.212 5.1.1-5.1.3 / 5.2.2 and the headers' contracts.  tools/asan/pusch_plan_driver.cc answers the queries under
g++ -fsanitize=address,undefined; one build and one run serve every test here.  No GPU, nothing loaded into Python.

The refusal texts are the ones mi_lte_pusch_plan_create* and mi_dlsch3_create set before the layout became a function of its own, and the order
of the checks is theirs: an input with several faults reports the same one.  Two refusals are new and replace undefined behaviour: a carrier
outside 6..100 resource blocks, and a reference-mode tbs above 6120 (tbs + 24 used to be formed in 32 bits, so 0xFFFFFFF0 wrapped to B = 8).

Two of the cases one might expect have no input that reaches them, and are left out for that reason: "allocation larger than the scrambling
table" needs N_prb > 151 at 64QAM, which no carrier of <= 100 resource blocks admits; and mi_lte_ulsch_layout has no refusal that depends on
the G control information leaves (G is a multiple of Q_m by construction), so "the transport block no longer fits" shows as its neighbour,
fewer symbols than code blocks -- tested at C - 1 symbols (refused) and C (accepted).  mi_dlsch3_layout does not take N_L: the slots of a
transmit-diversity plan (n_l = 2) are those of a one-layer plan, N_L enters in k_dl3_desc only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
OK, INVALID, UNSUPPORTED = 0, -1, -4
ENVELOPE = "PUSCH allocation outside the envelope (one code block; N_prb < N_rb_ul and divisible by 2, 3 or 5) or malformed"
SPEC = "PUSCH allocation outside the 3GPP transport-block mode (BPSK, F != 0 or tbs > 75376)"
UCI_G = "control information refused: O > 2, Q' > 4 M, O without Q' or Q' without O, Q_cqi not a multiple of Q_m, or no room left for data"
UCI_SYMB = "control information leaves a code block without a symbol"
UCI_MODE = "control information on PUSCH needs a plan in the 3GPP transport-block mode"
CARRIER = "PUSCH allocation names a resource block outside the carrier"
N_RB = "PUSCH plan on a carrier outside 6..100 resource blocks"
TAP = "plan larger than the symbol tap's 32-bit offsets"
TOO_LARGE = "3GPP plan too large"
# 36.212 table 5.1.3-3: the 188 code-block sizes
ALL_K = list(range(40, 512, 8)) + list(range(512, 1024, 16)) + list(range(1024, 2048, 32)) + list(range(2048, 6144 + 1, 64))
assert len(ALL_K) == 188
QM = (1, 2, 4, 6)
G24A = 0x1864CFB  # 36.212 5.1.1, x^24 included


def up(x, m):
    return -(-x // m) * m


def alloc(N_prb, mod=1, tbs=16, unit=0, rv=0, tx_mode=1, rnti=100, first=0, last0=NONE, last1=NONE, rep=1, uci=None):
    return dict(N_prb=N_prb, mod=mod, tbs=tbs, unit=unit, rv=rv, tx_mode=tx_mode, rnti=rnti, first=first, last0=last0, last1=last1, rep=rep, uci=uci)


def rec(a, has_uci):
    s = "%d %d %d %d %d %d %d %d %d %d %d" % (a["rep"], a["unit"], a["mod"], a["tbs"], a["rv"], a["tx_mode"], a["rnti"], a["N_prb"], a["first"], a["last0"], a["last1"])
    return s + (" %d %d %d %d %d" % (a["uci"] or (0, 0, 0, 0, 0)) if has_uci else "")


def q_plan(N_rb, spec, allocs, units=((3, 7),), caller=0, has_uci=0, brief=0):
    return "P %d %d %d %d %d %d %s %d %s" % (brief, N_rb, spec, caller, has_uci, len(units), " ".join("%d %d" % u for u in units), len(allocs),
                                             " ".join(rec(a, has_uci) for a in allocs))


def q_slots(allocs, n_soft=0xFFFFFFFF, m_harq=1, brief=0):
    return "D %d %d %d %d %s" % (brief, n_soft, m_harq, len(allocs), " ".join(rec(a, 0) for a in allocs))


def q_alloc(N_rb, n_units, spec, a):
    return "A %d %d %d %d %s" % (N_rb, n_units, spec, 1 if a["uci"] else 0, rec(a, 1 if a["uci"] else 0))


# ---- the restatement

def seg(tbs):
    """36.212 5.1.2 in the 3GPP mode (F = 0, one block size): (C, K), or None where the mode refuses the size"""
    if tbs == 0 or tbs > 75376:
        return None
    B = tbs + 24
    C = 1 if B <= 6144 else -(-B // 6120)
    Bp = B if C == 1 else B + 24 * C
    K = next(k for k in ALL_K if C * k >= Bp)
    return (C, K) if C * K == Bp else None


def planned(N_prb, N_rb, spec):
    return 0 < N_prb < N_rb and (N_prb % 2 == 0 or N_prb % 3 == 0 or N_prb % 5 == 0 or (spec and N_prb == 1))


def prbs(a):
    p = [[a["first"] + i for i in range(a["N_prb"])] for s in range(2)]
    for s, last in enumerate((a["last0"], a["last1"])):
        if last != NONE and a["N_prb"]:
            p[s][-1] = last
    return p


def uci_G(N_prb, Qm, u):
    """36.212 5.2.2.7: the bits control information leaves, None where include/mi_lte.h's mi_lte_ulsch_uci_G refuses"""
    O_ack, O_ri, Qp_ack, Qp_ri, Q_cqi = u
    M = 12 * N_prb
    if O_ack > 2 or O_ri > 2 or Qp_ack > 4 * M or Qp_ri > 4 * M or (O_ack == 0) != (Qp_ack == 0) or (O_ri == 0) != (Qp_ri == 0) or Q_cqi % Qm:
        return None
    g = Qm * (12 * M - Qp_ri) - Q_cqi
    return g if g > 0 else None


def check_alloc(a, N_rb, n_units, spec):
    """(rc, err, row, G) in pusch_alloc_check's order"""
    row = 0
    if not spec:
        row = -1 if a["tbs"] > 6120 else next(i for i, k in enumerate(ALL_K) if k >= a["tbs"] + 24)
    if row < 0 or not planned(a["N_prb"], N_rb, spec) or a["N_prb"] > 110 or a["mod"] > 3 or a["unit"] >= n_units:
        return UNSUPPORTED, ENVELOPE, -1, 0
    if spec and (a["mod"] == 0 or seg(a["tbs"]) is None):
        return UNSUPPORTED, SPEC, -1, 0
    G = 0
    if a["uci"]:
        Qm = QM[a["mod"]]
        G = uci_G(a["N_prb"], Qm, a["uci"])
        if G is None:
            return INVALID, UCI_G, -1, 0
        if G // Qm < seg(a["tbs"])[0]:
            return INVALID, UCI_SYMB, -1, G
    if any(p >= N_rb for s in prbs(a) for p in s):
        return INVALID, CARRIER, -1, G
    return OK, "", row, G


def xs_of(tbs, r, C, K):
    """x^s mod gCRC24A bit by bit, s = the transport-block bits (CRC24A included) behind block r's payload; C = 1: the block is the transport block"""
    s = 0 if C == 1 else tbs + 24 - (r + 1) * (K - 24)
    w = 1
    for _ in range(s):
        w <<= 1
        if w & 0x1000000:
            w ^= G24A
    return w


def slots_py(allocs):
    """mi_dlsch3_layout's struct: sizes ascending, inside a size the allocations in their order, an allocation's blocks adjacent"""
    ck = [seg(a["tbs"]) for a in allocs]
    out = {"a_nc": [c for c, k in ck], "a_K": [k for c, k in ck], "a_tbs": [a["tbs"] for a in allocs], "a_slot": [0] * len(allocs), "a_soft": [0] * len(allocs),
           "g3_groups": [], "g_soft": [], "g_bits": [], "slots": []}
    soft = bits = 0
    for K in sorted(set(out["a_K"])):
        soft, bits = up(soft, 256), up(bits, 256)
        out["g_soft"].append(soft); out["g_bits"].append(bits)
        base = len(out["slots"])
        for i, a in enumerate(allocs):
            if ck[i][1] != K:
                continue
            out["a_slot"][i], out["a_soft"][i] = len(out["slots"]), soft
            for r in range(ck[i][0]):
                out["slots"].append((i, r, ck[i][0], K, xs_of(a["tbs"], r, ck[i][0], K), soft // 4, bits // 8, 0))
                soft += 3 * (K + 4); bits += K
        out["g3_groups"].append((K, len(out["slots"]) - base, base, 0))
    out.update(n_slot=len(out["slots"]), soft_bytes=soft, bits_bytes=bits)
    return out


def plan_py(N_rb, spec, allocs, units=((3, 7),), caller=0, has_uci=0):
    """pusch_plan_layout's struct as the driver prints it, or (rc, err)"""
    allocs = [a for a in allocs for _ in range(a["rep"])]
    if has_uci and not spec:
        return UNSUPPORTED, UCI_MODE
    if not 6 <= N_rb <= 100:
        return INVALID, N_RB
    o = {k: [] for k in ("desc", "c_init", "e_len", "e_off", "row", "x_off", "G")}
    pool, seen, off = 0, {}, 0
    for a in allocs:
        rc, err, row, G = check_alloc(dict(a, uci=a["uci"] or (0, 0, 0, 0, 0)) if has_uci else dict(a, uci=None), N_rb, len(units), spec)
        if rc != OK:
            return rc, err
        sf, cell = units[a["unit"]][0] % 10, units[a["unit"]][1]
        key = (cell, sf, a["N_prb"])
        if caller or key not in seen:
            seen[key] = pool
            pool += 48 * a["N_prb"]
        o["desc"].append((sf, cell, seen[key]))
        o["c_init"].append(((a["rnti"] << 14) | (sf << 9) | cell) & 0xFFFFFFFF)
        E = 144 * a["N_prb"] * QM[a["mod"]]
        o["e_len"].append(E); o["e_off"].append(off // 64); o["row"].append(row)
        off += up(E, 64)
        if has_uci:
            o["G"].append(G)
    o.update(n=len(allocs), e_bytes=off, dmrs_n=pool, dmrs_ok=[1] * len(allocs), M_max=max(12 * a["N_prb"] for a in allocs),
             words_max=max((e + 31) // 32 + 1 for e in o["e_len"]), max_tbs=max(a["tbs"] for a in allocs))
    o["out_stride"] = up(o["max_tbs"], 64)
    o["groups"], o["cb_alloc"], o["x_end"] = [], [0] * len(allocs), 0
    if not spec:
        o["cb_alloc"] = []
        for row in sorted(set(o["row"])):
            mine = [i for i, r in enumerate(o["row"]) if r == row]
            o["groups"].append((ALL_K[row], len(mine), len(o["cb_alloc"]), max(o["e_len"][i] for i in mine)))
            o["cb_alloc"] += mine
    else:
        o.update(slots_py(allocs))
        at = 0
        for a in allocs:
            o["x_off"].append(at)
            at += 144 * a["N_prb"]
        o["x_off"].append(at); o["x_end"] = at
    return OK, o


# ---- the driver's answers

def parse(line):
    head, err = line.split(" err=", 1)
    out = {}
    for tok in head.split():
        k, v = tok.split("=", 1)
        items = [tuple(int(x) for x in it.split(":")) if ":" in it else int(it) for it in v.split(",")] if v else []
        out[k] = items if ("," in v or ":" in v or not v or k in LISTS) else int(v)
    return out, err


LISTS = {"groups", "desc", "dmrs_ok", "c_init", "e_len", "e_off", "row", "cb_alloc", "x_off", "G", "g3_groups", "g_soft", "g_bits", "a_slot", "a_nc", "a_K", "a_tbs",
         "a_soft", "slots"}


class Cases:
    def __init__(self):
        self.queries, self.want, self.names = [], [], {}

    def add(self, name, query, want):
        assert name not in self.names
        self.names[name] = len(self.queries)
        self.queries.append(query); self.want.append(want)


def plan_case(c, name, N_rb, spec, allocs, **kw):
    c.add(name, q_plan(N_rb, spec, allocs, **kw), plan_py(N_rb, spec, allocs, **kw))


CELLS = ((6, 5), (25, 24), (100, 99))  # N_rb and the largest admissible N_prb below it
UCI_NONE = (0, 0, 0, 0, 0)
BIG = alloc(2, tbs=75376)          # C = 13, K = 5824
N_TAP = -(-2 ** 32 // (144 * 99))  # 99-PRB allocations whose symbols pass 2^32
N_SOFT = -(-4 * 2 ** 32 // (13 * 3 * (5824 + 4)))  # 13-block allocations whose soft values pass 4 * 2^32 bytes


def build_cases():
    c = Cases()
    for N_rb, top in CELLS:
        for spec in (0, 1):
            for n in sorted({1, 2, 3, 5, 7, 11, top, N_rb}):
                for mod in range(5):
                    a = alloc(n, mod=mod, tbs=16 if not spec else 6200)
                    c.add("single %d %d %d %d" % (N_rb, spec, n, mod), q_alloc(N_rb, 1, spec, a), check_alloc(a, N_rb, 1, spec))
            # the unit index, and the last resource block on and past the carrier's edge, in one slot at a time
            tb = 16 if not spec else 6200
            plan_case(c, "unit last %d %d" % (N_rb, spec), N_rb, spec, [alloc(2, unit=2, tbs=tb)], units=((3, 7), (4, 8), (15, 9)))
            plan_case(c, "unit past %d %d" % (N_rb, spec), N_rb, spec, [alloc(2, unit=3, tbs=tb)], units=((3, 7), (4, 8), (15, 9)))
            for s in (0, 1):
                for last in (N_rb - 1, N_rb):
                    a = alloc(2, tbs=tb, last0=last if s == 0 else NONE, last1=last if s == 1 else NONE)
                    plan_case(c, "edge %d %d %d %d" % (N_rb, spec, s, last), N_rb, spec, [a])
    for tbs in (16, 6120, 6121, 0xFFFFFFF0):
        plan_case(c, "ref tbs %d" % tbs, 25, 0, [alloc(4, tbs=tbs)])
    for tbs in (75376, 76208, 75384, 6128, 100):  # the largest size; the next size of 36.213's tables and the next multiple of 8; two sizes with filler bits
        plan_case(c, "3gpp tbs %d" % tbs, 25, 1, [alloc(24, mod=3, tbs=tbs)])
    for N_rb in (5, 101, 200):
        for spec in (0, 1):
            plan_case(c, "N_rb %d %d" % (N_rb, spec), N_rb, spec, [alloc(2, tbs=16 if not spec else 6200)])
    # control information: every clause of the descriptor's refusal once, on QPSK over 2 PRB (M = 24: 4 M = 96, 12 M = 288 cells)
    for i, u in enumerate(((3, 0, 4, 0, 0), (0, 3, 0, 4, 0), (1, 0, 97, 0, 0), (0, 1, 0, 97, 0), (1, 0, 0, 0, 0), (0, 0, 4, 0, 0), (0, 1, 0, 0, 0), (0, 0, 0, 4, 0),
                           (0, 0, 0, 0, 3), (0, 0, 0, 0, 576), UCI_NONE, (2, 1, 96, 96, 100))):
        plan_case(c, "uci clause %d" % i, 25, 1, [alloc(2, tbs=6200, uci=u)], has_uci=1)
    # 13 code blocks on one PRB of QPSK (M = 12): 96 cells behind the rank indication, 2 * (96 - n) CQI bits leave n symbols
    for n in (12, 13):
        plan_case(c, "uci symbols %d" % n, 25, 1, [alloc(1, tbs=75376, uci=(0, 1, 0, 48, 2 * (96 - n)))], has_uci=1)
    plan_case(c, "uci reference mode", 25, 0, [alloc(2, uci=UCI_NONE)], has_uci=1)
    # layout
    trio = [alloc(4, mod=1, tbs=2000, unit=0, rnti=0x1234), alloc(2, mod=0, tbs=16, unit=1, rnti=0xFFFF, first=5), alloc(4, mod=2, tbs=6120, unit=2, rnti=1, first=10)]
    units = ((3, 7), (13, 503), (23, 7))  # subframes 13 and 23 are 3: allocations 0 and 2 share (cell 7, subframe 3, 4 PRB)
    plan_case(c, "layout ref", 25, 0, trio, units=units)
    plan_case(c, "layout ref caller", 25, 0, trio, units=units, caller=1)
    desc = [alloc(99, mod=3, tbs=6120), alloc(24, mod=2, tbs=3000, unit=1), alloc(5, mod=1, tbs=3000), alloc(3, mod=1, tbs=16, unit=1), alloc(2, mod=3, tbs=3000)]
    plan_case(c, "layout ref descending", 100, 0, desc, units=((9, 1), (0, 2)))
    spec3 = [alloc(24, mod=3, tbs=75376), alloc(1, mod=1, tbs=16, unit=1, first=9), alloc(24, mod=2, tbs=6200, unit=2, rv=5), alloc(99, mod=3, tbs=6120, rv=2),
             alloc(24, mod=3, tbs=75376, unit=2)]
    plan_case(c, "layout 3gpp", 100, 1, spec3, units=units)
    plan_case(c, "layout 3gpp caller", 100, 1, spec3, units=units, caller=1)
    plan_case(c, "layout 3gpp uci", 100, 1, [dict(a, uci=u) for a, u in zip(spec3, ((2, 2, 40, 20, 600), None, (1, 0, 4, 0, 0), (0, 1, 0, 4, 12), None))], units=units, has_uci=1)
    # several faults at once: the first allocation's comes first, and inside an allocation envelope < 3GPP layout < control information < carrier
    plan_case(c, "faults across", 25, 0, [alloc(2, last1=25), alloc(7)])
    plan_case(c, "faults envelope carrier", 25, 0, [alloc(7, last0=25)])
    plan_case(c, "faults envelope tbs carrier", 25, 0, [alloc(2, tbs=6121, last0=25)])
    plan_case(c, "faults bpsk carrier", 25, 1, [alloc(2, mod=0, tbs=6200, last0=25)])
    plan_case(c, "faults envelope bpsk", 25, 1, [alloc(7, mod=0, tbs=6128)])
    plan_case(c, "faults uci carrier", 25, 1, [alloc(2, tbs=6200, last0=25, uci=(3, 0, 4, 0, 0))], has_uci=1)
    plan_case(c, "faults size uci", 25, 1, [alloc(2, tbs=6128, uci=(3, 0, 4, 0, 0))], has_uci=1)
    plan_case(c, "faults uci mode N_rb", 200, 0, [alloc(7, uci=UCI_NONE)], has_uci=1)
    plan_case(c, "faults N_rb envelope", 200, 0, [alloc(7)])
    # the two size refusals, each reached by count, and the count before it
    for n in (N_TAP - 1, N_TAP):
        c.add("tap %d" % n, q_plan(100, 1, [alloc(99, rep=n)], brief=1), (UNSUPPORTED, TAP) if n == N_TAP else (OK, {"n": n, "x_end": n * 144 * 99, "n_slot": n}))
    for n in (N_SOFT - 1, N_SOFT):
        want = (UNSUPPORTED, TOO_LARGE) if n == N_SOFT else (OK, {"n_slot": 13 * n, "soft_bytes": 13 * n * 3 * 5828, "bits_bytes": 13 * n * 5824})
        c.add("soft plan %d" % n, q_plan(100, 1, [dict(BIG, rep=n)], brief=1), want)
        c.add("soft slots %d" % n, q_slots([dict(BIG, rep=n)], brief=1), want)
    # mi_dlsch3_layout alone: K = 40, C = 1 at the largest block, the first two-block size and the 13 blocks, not in ascending order, twice each
    mix = [alloc(2, tbs=t, tx_mode=m) for t, m in ((75376, 1), (16, 2), (6200, 3), (6120, 1), (16, 1), (75376, 4), (6200, 1), (6120, 2))]
    for n_soft, m_harq in ((0xFFFFFFFF, 1), (1827072, 8)):
        c.add("slots %d" % m_harq, q_slots(mix, n_soft, m_harq), (OK, slots_py(mix)))
    c.add("slots refused", q_slots([alloc(2, tbs=6200), alloc(2, tbs=6128)]), (UNSUPPORTED, "transport block size outside the 3GPP mode (F != 0 or tbs > 75376)"))
    return c


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """One sanitizer build and one run for the whole module: {name: (want, parsed answer, message)}"""
    c = build_cases()
    path = str(tmp_path_factory.mktemp("pusch_plan") / "queries.txt")
    with open(path, "w") as f:
        f.write("\n".join(c.queries) + "\n")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "run_pusch_plan.sh"), path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr + r.stdout, (r.stdout[-2000:] + r.stderr)[-4000:]
    assert "pusch plan driver: %d queries answered" % len(c.queries) in r.stderr, r.stderr[-1000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(c.queries)
    return {name: (c.want[i],) + parse(lines[i]) for name, i in c.names.items()}


def check(answers, name):
    """every field of the answer against the restatement (a brief answer: the fields the restatement names)"""
    want, got, err = answers[name]
    if want[0] != OK:
        assert (got["rc"], err) == want and set(got) == {"rc"}, (name, got, err)
        return None
    assert got["rc"] == OK and err == "", (name, got["rc"], err)
    for k, v in want[1].items():
        assert got[k] == v, (name, k, got[k], v)
    return got


def names(answers, prefix):
    found = [n for n in answers if n.startswith(prefix)]
    assert found
    return found


def test_single_allocations_on_6_25_and_100_resource_blocks(answers):
    """pusch_alloc_check and the bare N_prb rule on every cell x mode x N_prb {1, 2, 3, 5, 7, 11, the largest admissible, N_rb} x mod_type 0..4:
    code, text and row.  1 PRB only in the 3GPP mode; 7 and 11, N_rb itself and mod_type 4 refused; BPSK refused in the 3GPP mode only."""
    seen = set()
    for name in names(answers, "single "):
        (rc, err, row, G), got, text = answers[name]
        N_rb, spec, n, mod = (int(x) for x in name.split()[1:])
        assert (got["rc"], text, got["row"], got["G"]) == (rc, err, [row], [G]), (name, got, text)
        assert got["planned"] == (1 if planned(n, N_rb, spec) else 0), name
        fine = (n in (2, 3, 5, N_rb - 1) or (n == 1 and spec)) and n < N_rb and mod <= 3 and not (spec and mod == 0)
        assert (rc == OK) == fine, name
        seen.add((rc, err))
    assert seen == {(OK, ""), (UNSUPPORTED, ENVELOPE), (UNSUPPORTED, SPEC)}


def test_unit_index_and_carrier_edge(answers):
    """unit = n_units - 1 is taken (its subframe 15 counts as 5) and unit = n_units refused; a last resource block of N_rb - 1 is taken and one of
    N_rb refused with INVALID_ARG, in slot 0 alone and in slot 1 alone."""
    for N_rb, _ in CELLS:
        for spec in (0, 1):
            got = check(answers, "unit last %d %d" % (N_rb, spec))
            assert got["desc"] == [(5, 9, 0)]
            assert answers["unit past %d %d" % (N_rb, spec)][0] == (UNSUPPORTED, ENVELOPE)
            check(answers, "unit past %d %d" % (N_rb, spec))
            for s in (0, 1):
                assert check(answers, "edge %d %d %d %d" % (N_rb, spec, s, N_rb - 1)) is not None
                assert answers["edge %d %d %d %d" % (N_rb, spec, s, N_rb)][0] == (INVALID, CARRIER)
                check(answers, "edge %d %d %d %d" % (N_rb, spec, s, N_rb))


def test_transport_block_sizes(answers):
    """Reference mode: 16 (K = 40) and 6120 (row 187, K = 6144) are taken, 6121 and 0xFFFFFFF0 -- which used to wrap to B = 8 -- refused as outside
    the envelope.  3GPP mode: 75376 is taken (13 blocks of 5824), the sizes above it and the sizes with filler bits are not."""
    assert check(answers, "ref tbs 16")["row"] == [0] and check(answers, "ref tbs 6120")["row"] == [187]
    assert check(answers, "ref tbs 6120")["groups"] == [(6144, 1, 0, 144 * 4 * 2)]
    for tbs in (6121, 0xFFFFFFF0):
        assert answers["ref tbs %d" % tbs][0] == (UNSUPPORTED, ENVELOPE)
        check(answers, "ref tbs %d" % tbs)
    got = check(answers, "3gpp tbs 75376")
    assert (got["a_nc"], got["a_K"], got["out_stride"]) == ([13], [5824], 75392)
    for tbs in (76208, 75384, 6128, 100):
        assert answers["3gpp tbs %d" % tbs][0] == (UNSUPPORTED, SPEC)
        check(answers, "3gpp tbs %d" % tbs)


def test_carrier_width_outside_6_to_100_is_refused(answers):
    """cfg->N_rb_dl 5, 101 and 200: INVALID_ARG in either mode (with 200 the resource-block loop used to read past the allocation's 112 entries)"""
    for name in names(answers, "N_rb "):
        assert answers[name][0] == (INVALID, N_RB)
        check(answers, name)


def test_control_information(answers):
    """Each clause of mi_lte_ulsch_uci_G's refusal once (O > 2, Q' > 4 M, O without Q', Q' without O -- for ACK and for RI --, Q_cqi no multiple of
    Q_m, nothing left for data); a descriptor of zeros and a full one accepted with their G; 13 code blocks over 12 symbols refused and over 13
    accepted; descriptors on a reference-mode plan refused before anything else."""
    for i in range(10):
        assert answers["uci clause %d" % i][0] == (INVALID, UCI_G), i
        check(answers, "uci clause %d" % i)
    assert check(answers, "uci clause 10")["G"] == [2 * 288]
    assert check(answers, "uci clause 11")["G"] == [2 * (288 - 96) - 100]
    assert answers["uci symbols 12"][0] == (INVALID, UCI_SYMB)
    check(answers, "uci symbols 12")
    assert check(answers, "uci symbols 13")["G"] == [26]
    assert answers["uci reference mode"][0] == (UNSUPPORTED, UCI_MODE)
    check(answers, "uci reference mode")


def test_layout(answers):
    """Every field of the laid-out plan.  Three allocations of which the first and third share (cell, subframe mod 10, N_prb): two generated DMRS
    blocks in first-seen order, three with the caller's; c_init = rnti 2^14 + subframe 2^9 + cell; E = 144 N_prb Q_m; 64-byte offsets; the
    output stride; reference-mode groups in ascending K from allocations in descending size, cb_alloc slot by slot; the 3GPP mode's tap offsets
    cumulative at 144 N_prb and its slots; G per allocation with control information."""
    got = check(answers, "layout ref")
    assert [d[2] for d in got["desc"]] == [0, 192, 0] and got["dmrs_n"] == 192 + 96 and [d[0] for d in got["desc"]] == [3, 3, 3]
    assert got["c_init"] == [(0x1234 << 14) | (3 << 9) | 7, (0xFFFF << 14) | (3 << 9) | 503, (1 << 14) | (3 << 9) | 7]
    assert got["e_len"] == [1152, 288, 2304] and got["e_off"] == [0, 18, 23] and got["e_bytes"] == 64 * 59 and got["words_max"] == 73 and got["M_max"] == 48
    got = check(answers, "layout ref caller")
    assert [d[2] for d in got["desc"]] == [0, 192, 288] and got["dmrs_n"] == 480
    got = check(answers, "layout ref descending")
    assert [g[0] for g in got["groups"]] == [40, 3072, 6144] and got["cb_alloc"] == [3, 1, 2, 4, 0] and [g[3] for g in got["groups"]] == [864, 13824, 85536]
    got = check(answers, "layout 3gpp")
    assert got["x_off"] == [0, 3456, 3600, 7056, 21312, 24768] and got["dmrs_n"] == 48 * (24 + 1 + 99) and got["groups"] == []
    assert check(answers, "layout 3gpp caller")["dmrs_n"] == 48 * (24 + 1 + 24 + 99 + 24)
    got = check(answers, "layout 3gpp uci")
    assert got["G"] == [6 * (12 * 288 - 20) - 600, 2 * 144, 4 * 12 * 288, 6 * (12 * 1188 - 4) - 12, 6 * 12 * 288]


def test_several_faults_report_the_first_check_that_fails(answers):
    want = {"faults across": (INVALID, CARRIER), "faults envelope carrier": (UNSUPPORTED, ENVELOPE), "faults envelope tbs carrier": (UNSUPPORTED, ENVELOPE),
            "faults bpsk carrier": (UNSUPPORTED, SPEC), "faults envelope bpsk": (UNSUPPORTED, ENVELOPE), "faults uci carrier": (INVALID, UCI_G),
            "faults size uci": (UNSUPPORTED, SPEC), "faults uci mode N_rb": (UNSUPPORTED, UCI_MODE), "faults N_rb envelope": (INVALID, N_RB)}
    assert set(want) == set(names(answers, "faults "))
    for name, w in want.items():
        assert answers[name][0] == w, name
        check(answers, name)


def test_size_refusals_reached_by_count(answers):
    """301 275 allocations of 99 PRB hold 2^32 + 9 504 symbols: the tap's offsets refuse, one allocation fewer is laid out.  75 586 allocations of
    13 blocks hold more than 4 * 2^32 bytes of soft values: "3GPP plan too large" from pusch_plan_layout and from mi_dlsch3_layout alone, 75 585
    are laid out.  All six run under the sanitizers."""
    assert N_TAP == 301275 and N_SOFT == 75586
    for n in (N_TAP - 1, N_TAP):
        check(answers, "tap %d" % n)
    for n in (N_SOFT - 1, N_SOFT):
        check(answers, "soft plan %d" % n)
        check(answers, "soft slots %d" % n)
    assert answers["tap %d" % N_TAP][0] == (UNSUPPORTED, TAP) and answers["soft slots %d" % N_SOFT][0] == (UNSUPPORTED, TOO_LARGE)


def test_dlsch3_slots(answers):
    """mi_dlsch3_layout over tbs 16 (K = 40), 6120 (C = 1, K = 6144), 6200 (the first two-block size, K = 3136) and 75376 (13 x 5824), each twice,
    out of order and with transmission modes of either K_MIMO, under the uplink's and a downlink soft-buffer configuration (neither moves a slot):
    every field equals the restatement, and on its own terms: groups ascending in K; an allocation's blocks adjacent with r = 0 .. C - 1 from its
    first slot and soft offset; every group's start on 256 bytes; no two slots' soft or bit ranges overlapping; xs = x^(B - (r + 1)(K - 24))
    mod gCRC24A for C > 1 and 1 for C = 1, bit by bit."""
    for name in ("slots 1", "slots 8"):
        got = check(answers, name)
        Ks = [g[0] for g in got["g3_groups"]]
        assert Ks == [40, 3136, 5824, 6144] and got["n_slot"] == 2 * (1 + 1 + 2 + 13)
        assert all(x % 256 == 0 for x in got["g_soft"] + got["g_bits"])
        for a, (s0, C, K, tbs, soft) in enumerate(zip(got["a_slot"], got["a_nc"], got["a_K"], got["a_tbs"], got["a_soft"])):
            for r in range(C):
                al, r_, C_, K_, xs, soft4, bits8, pad = got["slots"][s0 + r]
                assert (al, r_, C_, K_, pad) == (a, r, C, K, 0)
                assert xs == (1 if C == 1 else xs_of(tbs, r, C, K)) and (C > 1 or xs == 1)
            assert got["slots"][s0][5] * 4 == soft
        for lo, hi, size in ((5, 4, lambda K: 3 * (K + 4)), (6, 8, lambda K: K)):
            spans = sorted((s[lo] * hi, s[lo] * hi + size(s[3])) for s in got["slots"])
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
            assert spans[-1][1] == (got["soft_bytes"] if lo == 5 else got["bits_bytes"])
        for (K, n_cb, base, _), g_soft, g_bits in zip(got["g3_groups"], got["g_soft"], got["g_bits"]):
            assert got["slots"][base][5] * 4 == g_soft and got["slots"][base][6] * 8 == g_bits
            assert all(s[3] == K for s in got["slots"][base:base + n_cb])
    assert answers["slots 1"][1] == answers["slots 8"][1]
    check(answers, "slots refused")

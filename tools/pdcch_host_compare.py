#!/usr/bin/env python3
"""The PDCCH host arithmetic of two builds of the library, byte for byte: the DCI unpackers, the search-space list, the REG tables and the
control-region synthesiser over the grids below, every out-struct filled with 0xA5 before each call so that "left untouched" is compared too.
None of these entry points needs a device.

    python tools/pdcch_host_compare.py --pkg DIR           one sha256 per family from DIR's openlte_amd (DIR holds the built package)
    python tools/pdcch_host_compare.py --parent-pkg DIR    one child process per library (DIR's and this tree's); exit 0 when all digests agree
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BW = (6, 15, 25, 50, 75, 100)
SIZES = {6: (21, 9), 15: (22, 11), 25: (25, 13), 50: (27, 13), 75: (27, 14), 100: (28, 15)}


def families(m, synth):
    L = m.load_library()
    u32, rng = C.c_uint32, np.random.default_rng(20)

    def poisoned(t):
        o = t()
        C.memset(C.byref(o), 0xA5, C.sizeof(o))
        return o

    def dci_unpack(h):
        pay = [int(x) for x in rng.integers(0, 1 << 32, 2000)]
        cases = [(f, nrb, nb, rnti, ant, p) for f in (L.mi_lte_dci_1a_unpack, L.mi_lte_dci_1c_unpack) for nrb in BW for nb in SIZES[nrb]
                 for rnti in (0xFFFF, 0xFFFE, 1, 0x3C, 0x100) for ant in (1, 2, 4) for p in pay]
        cases += [(f, 50, nb, 0xFFFF, 2, pay[0]) for f in (L.mi_lte_dci_1a_unpack, L.mi_lte_dci_1c_unpack) for nb in range(34)]
        for f, nrb, nb, rnti, ant, p in cases:
            o = poisoned(m.PdcchDci)
            h.update(b"%d" % f(p, nb, rnti, nrb, ant, C.byref(o)) + bytes(o))
        return len(cases)

    def dci_crnti(h):
        n = 0
        for nrb in list(range(1, 111)) + [0, 111]:
            for nb in range(66):
                for p in [int(x) for x in rng.integers(0, 1 << 63, 6)] + [0, (1 << 64) - 1]:
                    o = poisoned(m.DciCrnti)
                    h.update(b"%d" % L.mi_lte_dci_0_1a_unpack_crnti(p, nb, 0x1234, nrb, 2, C.byref(o)) + bytes(o))
                    n += 1
        for rnti, ant, null in ((0, 1, 0), (0x10000, 1, 0), (5, 3, 0), (5, 1, 1)):  # the other refusals
            o = poisoned(m.DciCrnti)
            h.update(b"%d" % L.mi_lte_dci_0_1a_unpack_crnti(1 << 40, 43, rnti, 100, ant, None if null else C.byref(o)) + bytes(o))
            n += 1
        return n

    def search_space(h):
        n = 0
        for rnti in (0, 1, 0x3C, 0x100, 0xFFFF, 0x10000):
            for sf in range(11):
                for n_cce in range(122):
                    for lv in (1, 2, 3, 4, 8):
                        first, cnt = np.full(6, 0xA5A5A5A5, np.uint32), poisoned(u32)  # (the library's u32p arguments are numpy arrays)
                        h.update(b"%d" % L.mi_lte_pdcch_search_space(rnti, sf, n_cce, lv, first, C.byref(cnt)) + bytes(first) + bytes(cnt))
                        n += 1
        return n

    L.mi_lte_ctrl_reg_positions.argtypes = [u32, u32, C.c_float, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u32)]

    def reg_tables(h):
        def one(nrb, cell, ng, ns, ant):
            pcf, cand = np.full(16, 0xA5A5A5A5, np.uint32), np.full(6 * 288, 0xA5A5A5A5, np.uint32)
            h.update(b"%d" % L.mi_lte_pdcch_re_tables(nrb, ant, cell, ng, ns, pcf, cand) + bytes(pcf) + bytes(cand))

        def pos(nrb, cell, ng):
            k, nn, nreg, pk = poisoned(u32 * 4), poisoned(C.c_float * 4), poisoned(u32), poisoned(u32 * 75)
            h.update(b"%d" % L.mi_lte_ctrl_reg_positions(nrb, cell, ng, k, nn, C.byref(nreg), pk) + bytes(k) + bytes(nn) + bytes(nreg) + bytes(pk))
        n = 0
        for nrb in BW:
            for cell in range(504):
                for ng in (1 / 6, 0.5, 1.0, 2.0):
                    pos(nrb, cell, ng)
                    n += 1
                    for ns in (1, 2, 3, 4):
                        for ant in (1, 2, 4):
                            one(nrb, cell, ng, ns, ant)
                            n += 1
        for nrb, cell, ng, ns, ant in ((7, 0, 1.0, 2, 1), (25, 0, 0.0, 2, 1), (25, 0, 2.5, 2, 1), (25, 0, float("nan"), 2, 1), (25, 504, 1.0, 2, 1),
                                       (25, 0, 1.0, 0, 1), (25, 0, 1.0, 5, 1), (25, 0, 1.0, 2, 3)):
            one(nrb, cell, ng, ns, ant)
            pos(nrb, cell, ng)
            n += 2
        return n

    def synth_grids(h):
        n = 0
        for nrb in BW:
            for ant in (1, 2, 4):
                cfg = m.DlCfg(2048, nrb, ant, 0)
                for cfi in (1, 2, 3, 4) if nrb > 10 else (1, 2, 3):
                    for seed in (3, 11):
                        for snr in (200.0, 10.0):
                            sf, cell = (seed + cfi) % 10, (37 * seed + nrb) % 504
                            dcis = [(0xFFFF, 3, 2, 1, 0), (0xFFFE, 5, 3, 0, 1), (0, 0, 0, 0, 0), (0x3C, 26, 1, nrb - 1, 2)]
                            h.update(synth.ctrl_grids(cfg, [sf], [cell], [cfi], [dcis], snr_db=snr, seed=seed).tobytes())
                            for recs in ([(0x1234, 1, 0, 28, 0xABCDEF1), (0xFFFF, 1, 1, 64, (1 << 64) - 3)],
                                         [(0x1234, 1, 0, 43, 0x5A5A5A5A5A5), (0x77, 2, 2, 9, 0x155), (0xFFF3, 4, 4, 28, 0x2345678), (0xFFFF, 8, 8, 1, 1)]):
                                try:
                                    h.update(synth.ctrl_grids_dci(cfg, [sf], [cell], [cfi], [recs], snr_db=snr, seed=seed).tobytes())
                                except m.MiLteError as e:  # (a record past the region's last CCE: the refusal is compared)
                                    h.update(str(e).encode())
                            n += 3
        return n

    return (("dci_unpack", dci_unpack), ("dci_0_1a_unpack_crnti", dci_crnti), ("pdcch_search_space", search_space), ("reg_tables", reg_tables),
            ("synth_ctrl_grids", synth_grids))


def digests(pkg):
    sys.path.insert(0, os.path.abspath(pkg))
    import openlte_amd as m
    from openlte_amd import synth
    assert os.path.abspath(m.__file__).startswith(os.path.abspath(pkg) + os.sep)
    for name, fn in families(m, synth):
        h = hashlib.sha256()
        n = fn(h)
        print("%s %d %s" % (name, n, h.hexdigest()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg")
    ap.add_argument("--parent-pkg")
    a = ap.parse_args()
    if a.pkg:
        digests(a.pkg)
        return 0
    out = [subprocess.run([sys.executable, os.path.abspath(__file__), "--pkg", d], capture_output=True, text=True, check=True).stdout.splitlines()
           for d in (a.parent_pkg, HERE)]
    same = len(out[0]) == len(out[1]) == 5
    for p, t in zip(*out):
        print("%-24s %8s calls  parent %s  this tree %s  %s" % (p.split()[0], p.split()[1], p.split()[2][:16], t.split()[2][:16], "equal" if p == t else "DIFFERENT"))
        same = same and p == t
    print("all families equal" if same else "NOT equal")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

"""ctypes binding of libmi_lte.so (include/mi_lte.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SOFT_F32, SOFT_I8, SOFT_I16 = 0, 1, 2
TURBO_REF, TURBO_BCJR, TURBO_BCJR_BLOCK, TURBO_BCJR_EARLY = 0, 1, 2, 3  # BCJR_BLOCK: one code block per wavefront, one launch (a handful of blocks; its own model)
_SOFT_OF_DTYPE = {np.dtype(np.float32): SOFT_F32, np.dtype(np.int8): SOFT_I8, np.dtype(np.int16): SOFT_I16}


IQ_I8, IQ_F32_PLANAR = 0, 1
IQ_ALL_ROWS = 0x100  # OR into DlCfg.sample_format: symbol row 15 also for one or two ports (MI_LTE_IQ_ALL_ROWS)
CE_COMPACT = 0x200   # OR into DlCfg.sample_format of the front end AND the PDSCH plan: magnitude / phase rows instead of estimate rows (MI_LTE_CE_COMPACT)


class DlCfg(C.Structure):
    """mi_lte_dl_cfg"""
    _fields_ = [("fft_size", C.c_uint32), ("N_rb_dl", C.c_uint32), ("N_ant", C.c_uint32), ("sample_format", C.c_uint32)]


class UlCfg(C.Structure):
    """mi_lte_ul_cfg: the liblte_phy_ul_init arguments the PUSCH DMRS depends on"""
    _fields_ = [(n, C.c_uint32) for n in ("group_assignment_pusch", "group_hopping_enabled", "sequence_hopping_enabled",
                                          "cyclic_shift", "cyclic_shift_dci")]


class PrachCfg(C.Structure):
    """mi_lte_prach_cfg"""
    _fields_ = [(n, C.c_uint32) for n in ("root_seq_idx", "preamble_format", "zczc", "hs_flag", "freq_offset")]


class PdschAlloc(C.Structure):
    """mi_lte_pdsch_alloc"""
    _fields_ = [(n, C.c_uint32) for n in ("unit", "mod_type", "tbs", "rv_idx", "tx_mode", "rnti", "N_prb", "n_pdcch_symbs")] + \
               [("prb", (C.c_uint8 * 112) * 2)]


class DlschCfg(C.Structure):
    """mi_lte_dlsch_cfg: the soft-buffer parameters of the 3GPP transport-block mode"""
    _fields_ = [("N_soft", C.c_uint32), ("M_dl_harq", C.c_uint32)]


class DlschLayout(C.Structure):
    """mi_lte_dlsch_layout_t"""
    _fields_ = [(n, C.c_uint32) for n in ("C", "K", "B", "N_cb", "k0")] + [("E", C.c_uint32 * 13), ("off", C.c_uint32 * 13)]


def dlsch_layout(tbs, G, Q_m, tx_mode=1, rv=0, n_soft=1237248, m_dl_harq=8, n_l=None):
    """mi_lte_dlsch_layout (host arithmetic): 36.212 segmentation and code-block concatenation of one transport block.  Returns a dict
    {C, K, B, N_cb, k0, E: [C], off: [C]}; raises MiLteError with the status on a refusal.  n_l: mi_lte_dlsch_layout_nl with that N_L
    (2: a transmit-diversity plan)."""
    L = load_library()
    out = DlschLayout()
    if n_l is None:
        rc = L.mi_lte_dlsch_layout(tbs, G, Q_m, tx_mode, rv, C.byref(DlschCfg(n_soft, m_dl_harq)), C.byref(out))
    else:
        rc = L.mi_lte_dlsch_layout_nl(tbs, G, Q_m, n_l, tx_mode, rv, C.byref(DlschCfg(n_soft, m_dl_harq)), C.byref(out))
    if rc != 0:
        raise MiLteError("mi_lte_dlsch_layout(%d, %d, %d) failed: %d" % (tbs, G, Q_m, rc), rc)
    return {"C": out.C, "K": out.K, "B": out.B, "N_cb": out.N_cb, "k0": out.k0, "E": list(out.E[:out.C]), "off": list(out.off[:out.C])}


def ulsch_layout(tbs, G, Q_m, rv=0):
    """mi_lte_ulsch_layout (host arithmetic): dlsch_layout for the uplink -- no soft-buffer limit (N_cb = K_w).  The same dict."""
    out = DlschLayout()
    rc = load_library().mi_lte_ulsch_layout(tbs, G, Q_m, rv, C.byref(out))
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_layout(%d, %d, %d) failed: %d" % (tbs, G, Q_m, rc), rc)
    return {"C": out.C, "K": out.K, "B": out.B, "N_cb": out.N_cb, "k0": out.k0, "E": list(out.E[:out.C]), "off": list(out.off[:out.C])}


class UlschUci(C.Structure):
    """mi_lte_ulsch_uci: the control information multiplexed on one PUSCH allocation (36.212 5.2.2.6-5.2.2.8); all zero: none"""
    _fields_ = [("O_ack", C.c_uint8), ("O_ri", C.c_uint8), ("Qp_ack", C.c_uint16), ("Qp_ri", C.c_uint16), ("Q_cqi", C.c_uint32)]


class UlschUciResult(C.Structure):
    """mi_lte_ulsch_uci_result"""
    _fields_ = [("ack", C.c_uint8 * 2), ("ri", C.c_uint8 * 2), ("S_ack", C.c_int32 * 3), ("S_ri", C.c_int32 * 3)]


UCI_ACK, UCI_RI, UCI_CQI = 0, 1, 2
UCI_CELL_DATA, UCI_CELL_CQI, UCI_CELL_RI, UCI_CELL_ACK_DATA, UCI_CELL_ACK_CQI = range(5)


def ulsch_uci_qprime(kind, O, beta_x8, M_sc_initial, N_symb_initial, sum_K_r, N_prb, Qp_ri=0):
    """mi_lte_ulsch_uci_qprime (host arithmetic): Q' of 36.212 5.2.2.6 for kind UCI_ACK / UCI_RI / UCI_CQI, beta as eighths."""
    out = C.c_uint32()
    rc = load_library().mi_lte_ulsch_uci_qprime(kind, O, beta_x8, M_sc_initial, N_symb_initial, sum_K_r, N_prb, Qp_ri, C.byref(out))
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_uci_qprime failed: %d" % rc, rc)
    return out.value


def ulsch_uci_G(N_prb, Q_m, uci):
    """mi_lte_ulsch_uci_G (host arithmetic): the coded data bits an allocation with control information `uci` leaves, 36.212 5.2.2.7."""
    out = C.c_uint32()
    rc = load_library().mi_lte_ulsch_uci_G(N_prb, Q_m, C.byref(uci), C.byref(out))
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_uci_G failed: %d" % rc, rc)
    return out.value


def ulsch_uci_map(N_prb, Q_m, uci):
    """mi_lte_ulsch_uci_map (host arithmetic): (kind uint8 [M, 12], index uint32 [M, 12, 2]) of the interleaver matrix, M = 12 N_prb:
    a cell's class (UCI_CELL_*), its symbol's number in its own stream, and for an ACK cell the data / CQI symbol it overwrote."""
    M = 12 * N_prb
    kind, index = np.zeros(12 * max(M, 1), np.uint8), np.zeros(24 * max(M, 1), np.uint32)
    rc = load_library().mi_lte_ulsch_uci_map(N_prb, Q_m, C.byref(uci), kind.ctypes.data, index.ctypes.data)
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_uci_map failed: %d" % rc, rc)
    return kind.reshape(M, 12), index.reshape(M, 12, 2)


class CqiResult(C.Structure):
    """mi_lte_cqi_result: one decoded CQI run.  O = 0: nothing decoded; crc: CQI_NONE / CQI_NO_CRC (block code) / CQI_CRC_OK / CQI_CRC_FAIL;
    metric: the decided code word's correlation with the combined soft bits, energy: the sum of their magnitudes; bits: information bit n
    at bit n & 31 of word n >> 5."""
    _fields_ = [("O", C.c_uint32), ("crc", C.c_uint32), ("metric", C.c_int32), ("energy", C.c_int32), ("bits", C.c_uint32 * 4)]

    def as_dict(self):
        return {"O": self.O, "crc": self.crc, "metric": self.metric, "energy": self.energy, "bits": list(self.bits)}


class CqiDesc(C.Structure):
    """mi_lte_cqi_desc: a run of Q_cqi soft bits at byte `off` (even) of the batch's soft bits, O information bits"""
    _fields_ = [("off", C.c_uint32), ("Q_cqi", C.c_uint32), ("O", C.c_uint32), ("pad", C.c_uint32)]


CQI_NONE, CQI_NO_CRC, CQI_CRC_OK, CQI_CRC_FAIL = range(4)
CQI_MAX_BITS, CQI_MAX_Q = 128, 6 * 12 * 1320


def cqi_encode(O, bits, Q_cqi):
    """mi_lte_cqi_encode (host arithmetic): the Q_cqi coded bits of O CQI information bits (36.212 5.2.2.6.4), one per byte -- what
    synth.ul_units_3gpp takes as `cqi`."""
    bits = np.ascontiguousarray(bits, np.uint8)
    if len(bits) < O:
        raise ValueError("cqi_encode: %d information bits given, O = %d" % (len(bits), O))
    out = np.zeros(Q_cqi if 0 < Q_cqi <= CQI_MAX_Q else 1, np.uint8)  # (a refused size is not allocated)
    rc = load_library().mi_lte_cqi_encode(O, bits.ctypes.data, Q_cqi, out.ctypes.data)
    if rc != 0:
        raise MiLteError("mi_lte_cqi_encode(%d, %d) failed: %d" % (O, Q_cqi, rc), rc)
    return out


class Pucch2Tab(C.Structure):
    """mi_lte_pucch2_tab: the sequences r[7 s + l][k] of all 14 symbols, the resource-block pair and the 20 scrambling bits of one
    (cell, subframe, n2, RNTI)"""
    _fields_ = [("r_re", (C.c_float * 12) * 14), ("r_im", (C.c_float * 12) * 14), ("prb", C.c_uint32 * 2), ("c_scr", C.c_uint32)]

    @property
    def r(self):
        """complex64 [14, 12]"""
        return (np.ctypeslib.as_array(self.r_re) + 1j * np.ctypeslib.as_array(self.r_im)).astype(np.complex64)


class Pucch2Res(C.Structure):
    """mi_lte_pucch2_res: format 0 / 1 / 2 = PUCCH format 2 / 2a / 2b, tab the index into the call's tables, A information bits"""
    _fields_ = [("unit", C.c_uint32), ("format", C.c_uint32), ("tab", C.c_uint32), ("A", C.c_uint32)]


class Pucch2Result(C.Structure):
    """mi_lte_pucch2_result (64 bytes): bits = a_n at bit n; metric of the decided word, energy = sum |e|; D, P and the 20 soft bits e are
    the decoder's stage taps (mi_lte.h)"""
    _fields_ = [("A", C.c_uint32), ("bits", C.c_uint32), ("metric", C.c_int32), ("energy", C.c_int32), ("ack", C.c_uint8 * 2), ("n_ack", C.c_uint8),
                ("pad0", C.c_uint8), ("D_re", C.c_float), ("D_im", C.c_float), ("P", C.c_float), ("e", C.c_int8 * 20), ("pad", C.c_uint8 * 12)]


PUCCH2_MAX_BITS, UL_GRID_SC = 13, 1200


def pucch2_table(ulcfg, n_id_cell, n_subfr, n_rb_ul, n_2_pucch, n_rb_2, n_cs_1, rnti):
    """mi_lte_ul_pucch2_table (host arithmetic): the Pucch2Tab of one (cell, subframe, resource n2, RNTI); 36.211 5.4.2, 5.4.3."""
    out = Pucch2Tab()
    rc = load_library().mi_lte_ul_pucch2_table(C.byref(ulcfg), n_id_cell, n_subfr, n_rb_ul, n_2_pucch, n_rb_2, n_cs_1, rnti, C.byref(out))
    if rc != 0:
        raise MiLteError("mi_lte_ul_pucch2_table(n2 = %d) failed: %d" % (n_2_pucch, rc), rc)
    return out


def pucch2_encode(A, bits):
    """mi_lte_pucch2_encode (host arithmetic): the 20 coded bits of A <= 13 CQI information bits (36.212 5.2.3.3), one per byte."""
    bits = np.ascontiguousarray(bits, np.uint8)
    if len(bits) < A:
        raise ValueError("pucch2_encode: %d information bits given, A = %d" % (len(bits), A))
    out = np.zeros(20, np.uint8)
    rc = load_library().mi_lte_pucch2_encode(A, bits.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise MiLteError("mi_lte_pucch2_encode(%d) failed: %d" % (A, rc), rc)
    return out


def pucch2_modulate(tab, fmt, b, ack=None, grid=None):
    """mi_lte_pucch2_modulate (host arithmetic): one UE's elements written into `grid` (float32 [2, 14, 1200], real and imaginary halves; a
    zeroed one is made when None), which is returned.  fmt 0 / 1 / 2 = format 2 / 2a / 2b, ack the one or two HARQ-ACK bits."""
    b = np.ascontiguousarray(b, np.uint8)
    if len(b) != 20:
        raise ValueError("pucch2_modulate: 20 coded bits, not %d" % len(b))
    if grid is None:
        grid = np.zeros((2, 14, UL_GRID_SC), np.float32)
    if grid.shape != (2, 14, UL_GRID_SC) or grid.dtype != np.float32 or not grid.flags.c_contiguous:
        raise ValueError("pucch2_modulate: grid must be contiguous float32 [2, 14, %d]" % UL_GRID_SC)
    a = None if ack is None else np.ascontiguousarray(list(ack) + [0, 0], np.uint8)[:2].copy()
    rc = load_library().mi_lte_pucch2_modulate(C.byref(tab), fmt, b.ctypes.data, None if a is None else a.ctypes.data, grid[0].ctypes.data, grid[1].ctypes.data)
    if rc != 0:
        raise MiLteError("mi_lte_pucch2_modulate failed: %d" % rc, rc)
    return grid


class PhichResult(C.Structure):
    """mi_lte_phich_result (32 bytes): metric = rep[0] + rep[1] + rep[2] (about -1 ACK, +1 NACK, 0 nothing sent), power = P_tot, hi = 1 for
    metric < 0; rep and power are the decoder's stage taps (mi_lte.h: "PHICH, 3GPP mode")"""
    _fields_ = [("metric", C.c_float), ("power", C.c_float), ("rep", C.c_float * 3), ("hi", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


PHICH_NO_POWER, PHICH_UNKNOWN_CELL, PHICH_N_SEQ = 1, 2, 8


class Pcfich(C.Structure):
    """mi_lte_pcfich: LIBLTE_PHY_PCFICH_STRUCT as mi_lte_pdcch_channel_encode reads (cfi) and writes (N_reg, k, n) it"""
    _fields_ = [("n", C.c_float * 4), ("k", C.c_uint32 * 4), ("cfi", C.c_uint32), ("N_reg", C.c_uint32)]


class Phich(C.Structure):
    """mi_lte_phich: LIBLTE_PHY_PHICH_STRUCT; present[m][n] / b[m][n]: indicator n of group m is sent / its value (1 = ACK)"""
    _fields_ = [("z_re", C.c_float * 3), ("z_im", C.c_float * 3), ("k", C.c_uint32 * 75), ("N_reg", C.c_uint32), ("b", (C.c_uint8 * 8) * 25),
                ("present", (C.c_uint8 * 8) * 25)]


def phich_n_group(n_rb_dl, phich_res):
    """mi_lte_phich_n_group (host arithmetic): ceil(N_g N_rb_dl / 8); 0 for a non-standard bandwidth or an N_g outside (0, 2]."""
    return int(load_library().mi_lte_phich_n_group(n_rb_dl, float(phich_res)))


def phich_resource(i_prb_ra_lowest, n_dmrs, n_group, i_phich=0):
    """mi_lte_phich_resource (host arithmetic, 36.213 9.1.2 with N_SF = 4): (n_group, n_seq) of the PHICH that answers a PUSCH."""
    g, s = C.c_uint32(), C.c_uint32()
    rc = load_library().mi_lte_phich_resource(i_prb_ra_lowest, n_dmrs, n_group, i_phich, C.byref(g), C.byref(s))
    if rc != 0:
        raise MiLteError("mi_lte_phich_resource(%d, %d, %d, %d) failed: %d" % (i_prb_ra_lowest, n_dmrs, n_group, i_phich, rc), rc)
    return g.value, s.value


def phich_re_table(n_rb_dl, n_id_cell, phich_res):
    """mi_lte_phich_re_table (host arithmetic): uint32 [N_group, 12], the sub-carrier in symbol 0 of RE(4 i + j) of every group of a cell."""
    n, re = C.c_uint32(), np.zeros(25 * 12, np.uint32)
    rc = load_library().mi_lte_phich_re_table(n_rb_dl, n_id_cell, float(phich_res), C.byref(n), re)
    if rc != 0:
        raise MiLteError("mi_lte_phich_re_table(%d, %d, %g) failed: %d" % (n_rb_dl, n_id_cell, phich_res, rc), rc)
    return re[:12 * n.value].reshape(n.value, 12).copy()


HARQ_NONE, HARQ_NEW_DATA = 0xFFFFFFFF, 1
EQ_ZF, EQ_MMSE = 0, 1  # mi_lte_pusch_plan_set_equaliser (3GPP plans)
DEMAP_REF, DEMAP_MAXLOG = 0, 1  # mi_lte_pdsch_plan_set_demapper, mi_lte_pusch_plan_set_demapper (3GPP plans)
DEMAP_AUTO_T = 16               # MI_LTE_DEMAP_AUTO_T


class HarqBind(C.Structure):
    """mi_lte_harq_bind"""
    _fields_ = [("buf", C.c_uint32), ("flags", C.c_uint32)]


class HarqState(C.Structure):
    """mi_lte_harq_state"""
    _fields_ = [(n, C.c_uint32) for n in ("tbs", "C", "K", "N_cb", "n_tx")] + [("status", C.c_int32)]


def harq_buffer_bytes(max_tbs):
    """mi_lte_harq_buffer_bytes (host arithmetic): soft bytes per buffer of a HARQ pool for max_tbs."""
    return int(load_library().mi_lte_harq_buffer_bytes(max_tbs))


def harq_binds(n_alloc, bufs, new_data=False):
    """A ctypes array of n_alloc mi_lte_harq_bind: bufs[a] is a buffer index or None (MI_LTE_HARQ_NONE); new_data a bool or one per
    allocation (MI_LTE_HARQ_NEW_DATA)."""
    bufs = list(bufs)
    nd = list(new_data) if isinstance(new_data, (list, tuple, np.ndarray)) else [new_data] * n_alloc
    if len(bufs) != n_alloc or len(nd) != n_alloc:
        raise ValueError("one binding per allocation: %d allocations, %d buffers, %d flags" % (n_alloc, len(bufs), len(nd)))
    arr = (HarqBind * max(n_alloc, 1))()
    for a in range(n_alloc):
        arr[a].buf = HARQ_NONE if bufs[a] is None else int(bufs[a])
        arr[a].flags = HARQ_NEW_DATA if nd[a] else 0
    return arr


def make_alloc(unit, mod_type, tbs, prbs, rnti, rv_idx=0, tx_mode=1, prbs_slot1=None, n_pdcch_symbs=0):
    a = PdschAlloc()
    a.unit, a.mod_type, a.tbs, a.rv_idx, a.tx_mode, a.rnti, a.N_prb = unit, mod_type, tbs, rv_idx, tx_mode, rnti, len(prbs)
    a.n_pdcch_symbs = n_pdcch_symbs
    for i, p in enumerate(prbs):
        a.prb[0][i] = p
        a.prb[1][i] = (prbs_slot1 or prbs)[i]
    return a


def tile_allocs(template, n_units):
    """The allocation list of n_units units that all carry the same template (a list of PdschAlloc for one unit): a ctypes array of
    n_units * len(template) structs with `unit` = 0 .. n_units - 1, built by numpy (half a million Python-made structs take a minute)."""
    k, sz = len(template), C.sizeof(PdschAlloc)
    base = np.frombuffer((PdschAlloc * k)(*template), np.uint8).reshape(k, sz)
    full = np.ascontiguousarray(np.broadcast_to(base, (n_units, k, sz))).reshape(n_units * k, sz)
    off = PdschAlloc.unit.offset
    full[:, off:off + 4] = np.repeat(np.arange(n_units, dtype=np.uint32), k).view(np.uint8).reshape(-1, 4)
    return (PdschAlloc * (n_units * k)).from_buffer(full)


class PipelineDevStats(C.Structure):
    """mi_lte_pipeline_dev_stats"""
    _fields_ = [("device", C.c_uint32), ("chunks", C.c_uint32), ("units", C.c_uint32), ("n_cpus", C.c_uint32), ("numa_node", C.c_int32), ("reserved", C.c_int32),
                ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("wall_s", C.c_double), ("h2d_s", C.c_double), ("kernel_s", C.c_double), ("d2h_s", C.c_double)]


class PucchRes(C.Structure):
    """mi_lte_pucch_res"""
    _fields_ = [("unit", C.c_uint32), ("format", C.c_uint32), ("N_1_p_pucch", C.c_uint32)]


class PdcchDci(C.Structure):
    """mi_lte_pdcch_dci"""
    _fields_ = [(n, C.c_uint32) for n in ("rnti", "format", "candidate", "n_bits", "payload", "mcs", "alloc_valid", "reserved")] + [("alloc", PdschAlloc)]


class PdcchFound(C.Structure):
    """mi_lte_pdcch_found: one hit of the blind PDCCH search"""
    _fields_ = [(n, C.c_uint32) for n in ("rnti", "L", "cce", "n_bits")] + [("payload", C.c_uint64), ("metric", C.c_int32), ("energy", C.c_int32)]

    def as_tuple(self):
        return (self.rnti, self.L, self.cce, self.n_bits, self.payload, self.metric, self.energy)


class DciCrnti(C.Structure):
    """mi_lte_dci_crnti: a C-RNTI's DCI format 0 / 1A, unpacked"""
    _fields_ = [(n, C.c_uint32) for n in ("format", "flag", "riv", "rb_start", "N_prb", "mcs", "harq", "ndi", "rv", "tpc", "cyclic_shift", "cqi_request")] + \
               [("alloc", PdschAlloc)]


PDCCH_SEARCH_MAX_SIZES, PDCCH_SEARCH_MAX_FOUND, PDCCH_SEARCH_ANY_CCE, PDCCH_SEARCH_36211_REGS = 4, 16, 1, 2


class CoarseTiming(C.Structure):
    """mi_lte_coarse_timing = LIBLTE_PHY_COARSE_TIMING_STRUCT"""
    _fields_ = [("freq_offset", C.c_float * 5), ("symb_starts", (C.c_uint32 * 7) * 5), ("n_corr_peaks", C.c_uint32)]


class TxAlloc(C.Structure):
    """mi_lte_tx_alloc: LIBLTE_PHY_ALLOCATION_STRUCT as the transmit functions read it"""
    _fields_ = [("msg", C.POINTER(C.c_uint8) * 2), ("msg_bits", C.c_uint32 * 2)] + \
               [(n, C.c_uint32) for n in ("pre_coder_type", "mod_type", "chan_type", "tbs", "rv_idx", "N_prb")] + [("prb", (C.c_uint32 * 110) * 2)] + \
               [(n, C.c_uint32) for n in ("N_codewords", "N_layers", "tx_mode", "rnti", "mcs", "tpc", "ndi", "dl_alloc")]


class MiLteError(RuntimeError):
    pass


def library_path():
    return os.path.join(_HERE, "libmi_lte.so")


def build_library():
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")])
    return library_path()


def load_library():
    """Load libmi_lte.so; raises if it has not been built -- there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise MiLteError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(the HIP extension is the only implementation; no CPU fallback exists)" % path)
    L = C.CDLL(path)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    L.mi_lte_version.restype = C.c_int
    L.mi_lte_device_count.restype = C.c_int
    L.mi_lte_build_id.restype = C.c_char_p
    L.mi_lte_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mi_lte_ctx_destroy.argtypes = [vp]
    L.mi_lte_last_error.argtypes = [vp]
    L.mi_lte_last_error.restype = C.c_char_p
    L.mi_lte_device_name.argtypes = [vp]
    L.mi_lte_device_name.restype = C.c_char_p
    L.mi_lte_last_kernels.argtypes = [vp]
    L.mi_lte_last_kernels.restype = C.c_char_p
    L.mi_lte_stream.argtypes = [vp]
    L.mi_lte_stream.restype = vp
    L.mi_lte_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.mi_lte_free.argtypes = [vp, vp]
    L.mi_lte_memset.argtypes = [vp, vp, C.c_int, sz]
    L.mi_lte_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.mi_lte_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.mi_lte_sync.argtypes = [vp]
    L.mi_lte_timer_start.argtypes = [vp]
    L.mi_lte_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.mi_lte_profile_enable.argtypes = [vp, C.c_int]
    L.mi_lte_profile_reset.argtypes = [vp]
    L.mi_lte_profile_report.argtypes = [vp]
    L.mi_lte_profile_report.restype = C.c_char_p
    L.mi_lte_subframe_floats.argtypes = [u32]
    L.mi_lte_subframe_floats.restype = sz
    L.mi_lte_dl_frontend_batch.argtypes = [vp, C.POINTER(DlCfg), vp, vp, vp, vp, vp, u32, vp]
    L.mi_lte_pdsch_plan_create.argtypes = [vp, C.POINTER(DlCfg), u32, vp, u32, C.POINTER(vp)]
    L.mi_lte_pdsch_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_pdsch_plan_set_decoder.argtypes = [vp, u32, u32, C.c_int]
    L.mi_lte_pdsch_plan_set_output.argtypes = [vp, u32]
    L.mi_lte_host_alloc.argtypes = [sz]
    L.mi_lte_host_alloc.restype = vp
    L.mi_lte_host_alloc_on.argtypes = [C.c_int, sz]
    L.mi_lte_host_alloc_on.restype = vp
    L.mi_lte_host_alloc_node.argtypes = [vp]
    L.mi_lte_host_alloc_node.restype = C.c_int
    L.mi_lte_device_numa_node.argtypes = [C.c_int]
    L.mi_lte_device_numa_node.restype = C.c_int
    L.mi_lte_dl_pipeline_device_stats.argtypes = [vp, u32, C.POINTER(PipelineDevStats)]
    L.mi_lte_host_free.argtypes = [vp]
    L.mi_lte_pdsch_plan_create_dynamic.argtypes = [vp, C.POINTER(DlCfg), u32, sz, C.POINTER(vp)]
    L.mi_lte_pdsch_plan_assign.argtypes = [vp, vp, u32, vp, u32]
    L.mi_lte_pdsch_plan_n_alloc.argtypes = [vp]
    L.mi_lte_pdsch_plan_n_alloc.restype = u32
    L.mi_lte_pdsch_alloc_decodable.argtypes = [C.POINTER(DlCfg), C.POINTER(PdschAlloc), u32]
    L.mi_lte_pdsch_alloc_decodable.restype = C.c_int
    L.mi_lte_iq_i8_to_planar.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.mi_lte_freq_shift_run.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_float, u32]
    L.mi_lte_dl_pipeline_create.argtypes = [C.c_int, C.POINTER(DlCfg), u32, vp, u32, u32, u32, C.POINTER(vp)]
    L.mi_lte_dl_pipeline_create_multi.argtypes = [C.POINTER(C.c_int), u32, C.POINTER(DlCfg), u32, vp, u32, sz, u32, u32, C.POINTER(vp)]
    L.mi_lte_dl_pipeline_n_devices.argtypes = [vp]
    L.mi_lte_dl_pipeline_n_devices.restype = u32
    L.mi_lte_dl_pipeline_run_units.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, vp]
    L.mi_lte_dl_pipeline_run_capture.argtypes = [vp, vp, C.c_uint64, C.c_uint64, u32, u32, u32, vp, vp, u32, vp, vp]
    L.mi_lte_dl_pipeline_destroy.argtypes = [vp]
    L.mi_lte_dl_pipeline_out_stride.argtypes = [vp]
    L.mi_lte_dl_pipeline_out_stride.restype = u32
    L.mi_lte_dl_pipeline_unit_samples.argtypes = [vp]
    L.mi_lte_dl_pipeline_unit_samples.restype = sz
    L.mi_lte_dl_pipeline_last_error.argtypes = [vp]
    L.mi_lte_dl_pipeline_last_error.restype = C.c_char_p
    L.mi_lte_dl_pipeline_run.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.mi_lte_pdsch_plan_out_stride.argtypes = [vp]
    L.mi_lte_pdsch_plan_out_stride.restype = u32
    L.mi_lte_pdsch_decode_run.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.mi_lte_pdsch_plan_soft_bits.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp)]
    L.mi_lte_dlsch_layout.argtypes = [u32, u32, u32, u32, u32, C.POINTER(DlschCfg), C.POINTER(DlschLayout)]
    L.mi_lte_pdsch_plan_create_3gpp.argtypes = [vp, C.POINTER(DlCfg), u32, C.POINTER(DlschCfg), vp, u32, C.POINTER(vp)]
    L.mi_lte_pdsch_alloc_decodable_3gpp.argtypes = [C.POINTER(DlCfg), C.POINTER(DlschCfg), C.POINTER(PdschAlloc), u32]
    L.mi_lte_pdsch_alloc_decodable_3gpp.restype = C.c_int
    L.mi_lte_dlsch_layout_nl.argtypes = [u32, u32, u32, u32, u32, u32, C.POINTER(DlschCfg), C.POINTER(DlschLayout)]
    L.mi_lte_pdsch_plan_create_3gpp_txdiv.argtypes = L.mi_lte_pdsch_plan_create_3gpp.argtypes
    L.mi_lte_pdsch_alloc_decodable_3gpp_txdiv.argtypes = L.mi_lte_pdsch_alloc_decodable_3gpp.argtypes
    L.mi_lte_pdsch_alloc_decodable_3gpp_txdiv.restype = C.c_int
    L.mi_lte_pdsch_plan_cb_soft.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_pdsch_plan_cb_ok.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pdsch_plan_set_demapper.argtypes = [vp, u32, C.c_float]
    L.mi_lte_pdsch_plan_llr_gain.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pdsch_plan_set_llr_noise.argtypes = [vp, C.c_float]
    L.mi_lte_pdsch_plan_llr_noise.argtypes = [vp, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_dl_crs_noise_run.argtypes = [vp, C.POINTER(DlCfg), vp, vp, vp, u32, vp]
    L.mi_lte_harq_buffer_bytes.argtypes = [u32]
    L.mi_lte_harq_buffer_bytes.restype = sz
    L.mi_lte_harq_pool_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.mi_lte_harq_pool_destroy.argtypes = [vp, vp]
    L.mi_lte_harq_pool_destroy.restype = None
    L.mi_lte_harq_pool_reset.argtypes = [vp, vp, u32]
    L.mi_lte_harq_pool_soft.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(vp)]
    L.mi_lte_pdsch_decode_run_harq.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mi_lte_ul_subframe_floats.restype = sz
    L.mi_lte_ul_frontend_batch.argtypes = [vp, C.POINTER(DlCfg), vp, vp, vp, u32, vp]
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
    L.mi_lte_ul_dmrs_pusch.argtypes = [C.POINTER(UlCfg), u32, u32, u32, f32p, f32p, f32p, f32p]
    L.mi_lte_pusch_plan_create.argtypes = [vp, C.POINTER(DlCfg), C.POINTER(UlCfg), u32p, u32p, u32, vp, u32, C.POINTER(vp)]
    L.mi_lte_pusch_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_pusch_plan_out_stride.argtypes = [vp]
    L.mi_lte_pusch_plan_out_stride.restype = u32
    L.mi_lte_pusch_decode_run.argtypes = [vp, vp, vp, vp, vp]
    L.mi_lte_pusch_plan_soft_bits.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_pusch_plan_create_3gpp.argtypes = L.mi_lte_pusch_plan_create.argtypes
    L.mi_lte_pusch_plan_set_decoder.argtypes = [vp, u32, u32, C.c_int]
    L.mi_lte_pusch_plan_set_output.argtypes = [vp, u32]
    L.mi_lte_pusch_plan_cb_soft.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_pusch_plan_cb_ok.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_ulsch_layout.argtypes = [u32, u32, u32, u32, C.POINTER(DlschLayout)]
    L.mi_lte_ulsch_uci_qprime.argtypes = [u32] * 8 + [C.POINTER(u32)]
    L.mi_lte_ulsch_uci_G.argtypes = [u32, u32, C.POINTER(UlschUci), C.POINTER(u32)]
    L.mi_lte_ulsch_uci_map.argtypes = [u32, u32, C.POINTER(UlschUci), vp, vp]
    L.mi_lte_pusch_plan_create_3gpp_uci.argtypes = L.mi_lte_pusch_plan_create.argtypes[:-1] + [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_uci_results.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_cqi_soft.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_pusch_plan_data_soft.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_cqi_encode.argtypes = [u32, vp, u32, vp]
    L.mi_lte_cqi_decode_batch.argtypes = [vp, vp, vp, u32, vp]
    L.mi_lte_pusch_plan_set_cqi_decode.argtypes = [vp, vp]
    L.mi_lte_pusch_plan_cqi_results.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_set_demapper.argtypes = [vp, u32, C.c_float]
    L.mi_lte_pusch_plan_llr_gain.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_llr_rho.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_set_llr_tap.argtypes = [vp, u32]
    L.mi_lte_pusch_plan_set_llr_noise.argtypes = [vp, C.c_float]
    L.mi_lte_pusch_plan_llr_noise.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_plan_set_rx_antennas.argtypes = [vp, u32, u32]
    L.mi_lte_pusch_plan_rx_antennas.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_pusch_plan_set_equaliser.argtypes = [vp, u32]
    L.mi_lte_pusch_plan_equaliser.argtypes = [vp, C.POINTER(u32)]
    L.mi_lte_pusch_plan_llr_nu.argtypes = [vp, C.POINTER(vp)]
    L.mi_lte_pusch_decode_run_harq.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.mi_lte_pusch_plan_llr_symbols.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_prach_plan_create.argtypes = [vp, C.POINTER(DlCfg), C.POINTER(PrachCfg), C.POINTER(vp)]
    L.mi_lte_prach_plan_create_roots.argtypes = [vp, C.POINTER(DlCfg), C.POINTER(PrachCfg), f32p, f32p, u32, C.POINTER(vp)]
    L.mi_lte_prach_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_prach_plan_n_roots.argtypes = [vp]
    L.mi_lte_prach_plan_n_roots.restype = u32
    L.mi_lte_prach_occasion_samples.argtypes = [vp]
    L.mi_lte_prach_occasion_samples.restype = u32
    L.mi_lte_prach_detect_run.argtypes = [vp, vp, vp, vp, vp, u32, u32p, u32p, u32p]
    L.mi_lte_prach_detect_launch.argtypes = [vp, vp, vp, vp, vp, u32]
    L.mi_lte_prach_detect_fetch.argtypes = [vp, vp, u32p, u32p, u32p, u32]
    L.mi_lte_prach_detect_tap.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp]
    L.mi_lte_device_copy_rate.argtypes = [vp, C.c_size_t, u32, C.POINTER(C.c_double)]
    L.mi_lte_device_copy_rates.argtypes = [vp, C.POINTER(C.c_double)]
    L.mi_lte_pdcch_plan_create.argtypes = [vp, C.POINTER(DlCfg), C.c_float, u32, u32, u32p, u32, C.POINTER(vp)]
    L.mi_lte_pdcch_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_pdcch_decode_run.argtypes = [vp, vp, vp, vp, vp, u32, u32p, u32p, u32p, u32p, C.POINTER(PdcchDci)]
    L.mi_lte_pucch_decode_run.argtypes = [vp, u32, u32, vp, C.POINTER(PucchRes), f32p, u32, u8p, u32p, u32p]
    L.mi_lte_ul_pucch2_table.argtypes = [C.POINTER(UlCfg)] + [u32] * 7 + [C.POINTER(Pucch2Tab)]
    L.mi_lte_pucch2_encode.argtypes = [u32, vp, vp]
    L.mi_lte_pucch2_modulate.argtypes = [C.POINTER(Pucch2Tab), u32, vp, vp, vp, vp]
    L.mi_lte_pucch2_decode_run.argtypes = [vp, u32, vp, u32, C.POINTER(Pucch2Res), u32, C.POINTER(Pucch2Tab), u32, vp]
    L.mi_lte_pdcch_channel_encode.argtypes = [vp, u32, u32, u32, u32, u32, C.POINTER(Pcfich), C.POINTER(Phich), C.POINTER(TxAlloc), u32, C.POINTER(u32), u32, u32, u32, u32,
                                              f32p, f32p]
    L.mi_lte_phich_n_group.argtypes = [u32, C.c_float]
    L.mi_lte_phich_n_group.restype = u32
    L.mi_lte_phich_resource.argtypes = [u32, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_phich_re_table.argtypes = [u32, u32, C.c_float, C.POINTER(u32), u32p]
    L.mi_lte_phich_plan_create.argtypes = [vp, C.POINTER(DlCfg), C.c_float, u32, u32, u32p, u32, C.POINTER(vp)]
    L.mi_lte_phich_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_phich_plan_n_group.argtypes = [vp]
    L.mi_lte_phich_plan_n_group.restype = u32
    L.mi_lte_phich_decode_run.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    L.mi_lte_coarse_timing_samples.argtypes = [u32, u32]
    L.mi_lte_coarse_timing_samples.restype = C.c_size_t
    L.mi_lte_coarse_timing_run.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, u32, C.POINTER(CoarseTiming)]
    L.mi_lte_find_pss_run.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, u32p, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.mi_lte_find_sss_run.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, u32, u32p, C.c_float, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_coarse_timing_tap.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, u32, vp, vp]
    L.mi_lte_find_pss_tap.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, vp, u32, u32, C.c_int32, vp, vp, vp, vp]
    L.mi_lte_find_sss_tap.argtypes = [vp, C.POINTER(DlCfg), vp, vp, C.c_uint64, u32, vp, vp, vp]
    L.mi_lte_pbch_decode_run.argtypes = [vp, C.POINTER(DlCfg), vp, vp, u32, u32p, u32p, u32p]
    L.mi_lte_pdcch_re_tables.argtypes = [u32, u32, u32, C.c_float, u32, u32p, u32p]
    L.mi_lte_dci_1a_unpack.argtypes = [u32, u32, u32, u32, u32, C.POINTER(PdcchDci)]
    L.mi_lte_dci_1c_unpack.argtypes = [u32, u32, u32, u32, u32, C.POINTER(PdcchDci)]
    L.mi_lte_pdcch_search_space.argtypes = [u32, u32, u32, u32, u32p, C.POINTER(u32)]
    L.mi_lte_pdcch_cce_tables.argtypes = [u32, u32, u32, C.c_float, u32, u32, C.POINTER(u32), u32p, u32]
    L.mi_lte_pdcch_search_plan_create.argtypes = [vp, C.POINTER(DlCfg), C.c_float, u32, u32, u32p, u32, u32p, u32, C.POINTER(vp)]
    L.mi_lte_pdcch_search_plan_set_rntis.argtypes = [vp, vp, u32p, u32]
    L.mi_lte_pdcch_search_plan_destroy.argtypes = [vp, vp]
    L.mi_lte_pdcch_search_run.argtypes = [vp, vp, vp, vp, vp, u32, u32p, u32p, u32p, C.POINTER(PdcchFound)]
    L.mi_lte_pdcch_search_soft.argtypes = [vp, C.POINTER(vp), C.POINTER(u32)]
    L.mi_lte_dci_0_1a_unpack_crnti.argtypes = [C.c_uint64, u32, u32, u32, u32, C.POINTER(DciCrnti)]
    L.mi_lte_turbo_decode_batch.argtypes = [vp, vp, C.c_int, u32, u32, C.c_int, u32, C.c_int, vp]
    L.mi_lte_set_turbo_small_batch.argtypes = [vp, u32]
    L.mi_lte_turbo_early_exit_iterations.argtypes = [vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    L.mi_lte_turbo_scratch_bytes.argtypes = [u32, u32]
    L.mi_lte_turbo_scratch_bytes.restype = sz
    L.mi_lte_tbs.argtypes = [u32, u32]
    L.mi_lte_tbs.restype = u32
    # the transmit side (host code): the handle and the grid functions
    L.mi_lte_tx_create.argtypes = [C.POINTER(vp)]
    L.mi_lte_tx_destroy.argtypes = [vp]
    L.mi_lte_pdsch_channel_encode.argtypes = [vp, u32, u32, C.POINTER(TxAlloc), u32, u32, u32, u32, u32, f32p, f32p]
    L.mi_lte_bch_channel_encode.argtypes = [vp, u32, u32, u8p, u32, u32, u32, u32, f32p, f32p]
    L.mi_lte_map_crs.argtypes = [u32, u32, u32, u32, u32, f32p, f32p]
    L.mi_lte_map_pss.argtypes = [u32, u32, u32, u32, f32p, f32p]
    L.mi_lte_map_sss.argtypes = [u32, u32, u32, u32, u32, u32, f32p, f32p]
    L.mi_lte_create_dl_subframe.argtypes = [u32, u32, u32, u32, f32p, f32p, u32, f32p, f32p]
    _LIB = L
    return L


class DeviceBuffer:
    """A block of HBM owned by a Context (hipMalloc through the C-ABI)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        ctx._check(ctx.L.mi_lte_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        self.ctx._check(self.ctx.L.mi_lte_memcpy_h2d(self.ctx.h, self.ptr + offset, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        if count is None:
            count = (self.nbytes - offset) // dtype.itemsize
        out = np.empty(count, dtype)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def zero(self):
        self.ctx._check(self.ctx.L.mi_lte_memset(self.ctx.h, self.ptr, 0, self.nbytes))

    def free(self):
        if self.ptr:
            self.ctx.L.mi_lte_free(self.ctx.h, self.ptr)
            self.ptr = None


class PdschPlan:
    """mi_lte_pdsch_plan: device copy of an allocation list, grouped by code-block size.  allocs=None: a dynamic plan of the given
    capacity (mi_lte_pdsch_plan_create_dynamic), filled and re-filled by assign()."""

    def __init__(self, ctx, cfg, n_pdcch_symbs, allocs, max_alloc=0, max_soft_bytes=0, dlsch=None, txdiv=False):
        """dlsch: a DlschCfg -- a plan in the 3GPP transport-block mode (mi_lte_pdsch_plan_create_3gpp; txdiv: on a cell of two or four ports,
        mi_lte_pdsch_plan_create_3gpp_txdiv)."""
        self.ctx = ctx
        h = C.c_void_p()
        if dlsch is not None:
            self.n_alloc = len(allocs)
            arr = (PdschAlloc * len(allocs))(*allocs)
            create = ctx.L.mi_lte_pdsch_plan_create_3gpp_txdiv if txdiv else ctx.L.mi_lte_pdsch_plan_create_3gpp
            ctx._check(create(ctx.h, C.byref(cfg), n_pdcch_symbs, C.byref(dlsch), C.cast(arr, C.c_void_p), len(allocs), C.byref(h)))
            self.h, self.tbs, self._arr = h, [a.tbs for a in allocs], arr
        elif allocs is None:
            ctx._check(ctx.L.mi_lte_pdsch_plan_create_dynamic(ctx.h, C.byref(cfg), max_alloc, max_soft_bytes, C.byref(h)))
            self.h, self.n_alloc, self.tbs = h, 0, []
        else:
            self.n_alloc = len(allocs)
            arr = allocs if isinstance(allocs, C.Array) else (PdschAlloc * len(allocs))(*allocs)  # (a ready-made ctypes array: tile_allocs below)
            ctx._check(ctx.L.mi_lte_pdsch_plan_create(ctx.h, C.byref(cfg), n_pdcch_symbs, C.cast(arr, C.c_void_p), len(allocs),
                                                      C.byref(h)))
            self.h = h
            self.tbs = None if isinstance(allocs, C.Array) else [a.tbs for a in allocs]  # (a ctypes array: read on demand, run() below)
            self._arr = arr
        self.out_stride = ctx.L.mi_lte_pdsch_plan_out_stride(h)

    def assign(self, n_pdcch_symbs, allocs):
        """Re-plan a dynamic plan (no allocation, no wait); allocations may carry their own n_pdcch_symbs."""
        arr = (PdschAlloc * len(allocs))(*allocs)
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_assign(self.ctx.h, self.h, n_pdcch_symbs, C.cast(arr, C.c_void_p), len(allocs)))
        self.n_alloc, self.tbs = len(allocs), [a.tbs for a in allocs]
        self.out_stride = self.ctx.L.mi_lte_pdsch_plan_out_stride(self.h)

    def set_decoder(self, mode, n_iter=8, qpp_spec=0):
        """TURBO_REF (default, the reference's decoder) or TURBO_BCJR (max-log-MAP, n_iter iterations)."""
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_set_decoder(self.h, mode, n_iter, qpp_spec))

    def set_packed(self, packed=True):
        """Eight bits per byte (first bit in the most significant position) instead of the reference's one bit per byte; changes out_stride."""
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_set_output(self.h, 1 if packed else 0))
        self.packed = bool(packed)
        self.out_stride = self.ctx.L.mi_lte_pdsch_plan_out_stride(self.h)

    def run_dev(self, d_subframes, d_sf, d_cell, d_out, d_status):
        self.ctx._check(self.ctx.L.mi_lte_pdsch_decode_run(self.ctx.h, self.h, d_subframes.ptr, d_sf.ptr, d_cell.ptr,
                                                           d_out.ptr, d_status.ptr))

    def run_harq_dev(self, pool, binds, d_subframes, d_sf, d_cell, d_out, d_status):
        """mi_lte_pdsch_decode_run_harq (3GPP mode): binds is a ctypes array of HarqBind, one per allocation (harq_binds), or None -- a NULL
        binding, which the library refuses."""
        self.ctx._check(self.ctx.L.mi_lte_pdsch_decode_run_harq(self.ctx.h, self.h, pool.h, None if binds is None else C.cast(binds, C.c_void_p),
                                                                d_subframes.ptr, d_sf.ptr, d_cell.ptr, d_out.ptr, d_status.ptr))

    def run(self, d_subframes, subfr_num, n_id_cell, harq=None):
        """Returns (status int32 [n_alloc], list of uint8 bit arrays).  harq = (pool, bufs, new_data): a HARQ run (3GPP mode) that combines
        allocation a into pool buffer bufs[a] (None: not combined); new_data a bool or one per allocation."""
        ctx = self.ctx
        binds = None if harq is None else harq_binds(self.n_alloc, harq[1], harq[2] if len(harq) > 2 else False)
        d_sf, d_cell = ctx.to_device(np.asarray(subfr_num, np.uint32)), ctx.to_device(np.asarray(n_id_cell, np.uint32))
        d_out, d_st = ctx.alloc(self.n_alloc * self.out_stride), ctx.alloc(4 * self.n_alloc)
        d_out.zero()
        try:
            if harq is None:
                self.run_dev(d_subframes, d_sf, d_cell, d_out, d_st)
            else:
                self.run_harq_dev(harq[0], binds, d_subframes, d_sf, d_cell, d_out, d_st)
            st = d_st.download(np.int32)
            bits = d_out.download(np.uint8).reshape(self.n_alloc, self.out_stride)
            if getattr(self, "packed", False):  # back to one bit per byte for the caller
                return st, [np.unpackbits(bits[a, :(self._tbs()[a] + 7) // 8])[:self._tbs()[a]] for a in range(self.n_alloc)]
            return st, [bits[a, :self._tbs()[a]] for a in range(self.n_alloc)]
        finally:
            for b in (d_sf, d_cell, d_out, d_st):
                b.free()

    def _tbs(self):
        if self.tbs is None:
            self.tbs = [a.tbs for a in self._arr]
        return self.tbs

    def soft_bits(self, alloc):
        """Descrambled int8 soft bits of one allocation (stage tap)."""
        pe, pn = C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_soft_bits(self.h, alloc, C.byref(pe), C.byref(pn)))
        n = np.empty(1, np.uint32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, n.ctypes.data, pn.value, 4))
        out = np.empty(int(n[0]), np.int8)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, pe.value, out.nbytes))
        return out

    def cb_soft(self, alloc):
        """3GPP mode, after a run: the C rate-un-matched code blocks of one allocation, int8 [C, 3 (K + 4)] (stage tap)."""
        p, nc, k = C.c_void_p(), C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_cb_soft(self.h, alloc, C.byref(p), C.byref(nc), C.byref(k)))
        out = np.empty((nc.value, 3 * (k.value + 4)), np.int8)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def cb_ok(self):
        """3GPP mode, after a run: uint32 [n_alloc], bit r set when code block r's CRC24B passed (one block: bit 0 = the CRC24A verdict)."""
        p = C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_cb_ok(self.h, C.byref(p)))
        out = np.empty(self.n_alloc, np.uint32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def set_demapper(self, mode, gain=0.0):
        """3GPP mode: DEMAP_REF (default, the reference's demapper) or DEMAP_MAXLOG (max-log LLRs; gain 0: automatic per allocation,
        > 0: that gain for every allocation)."""
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_set_demapper(self.h, mode, gain))

    def llr_gain(self):
        """3GPP mode, after a run: float32 [n_alloc], the gain the MAXLOG demapper used per allocation (stage tap)."""
        p = C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_llr_gain(self.h, C.byref(p)))
        out = np.empty(self.n_alloc, np.float32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def set_llr_noise(self, scale):
        """3GPP mode: scale > 0: MAXLOG runs use the noise-referenced gain g_a = scale / sigma2[unit] of the CRS noise estimate in place of
        set_demapper's gain (so retransmissions combine on one scale); 0: off."""
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_set_llr_noise(self.h, scale))

    def llr_noise(self):
        """3GPP mode: float32 [n_units], sigma2 per unit of the last MAXLOG run with the noise gain on (stage tap; zeros before one);
        n_units = 1 + the largest unit an allocation of the plan names."""
        p, n = C.c_void_p(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pdsch_plan_llr_noise(self.h, C.byref(p), C.byref(n)))
        out = np.empty(n.value, np.float32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_pdsch_plan_destroy(self.ctx.h, self.h)
            self.h = None


class HarqPool:
    """mi_lte_harq_pool: n_buf device soft buffers for HARQ combining in the 3GPP mode, owned by a Context and shared by its plans."""

    def __init__(self, ctx, n_buf, max_tbs=75376):
        self.ctx, self.n_buf, self.max_tbs = ctx, int(n_buf), int(max_tbs)
        h = C.c_void_p()
        ctx._check(ctx.L.mi_lte_harq_pool_create(ctx.h, self.n_buf, self.max_tbs, C.byref(h)))
        self.h = h
        self.buffer_bytes = harq_buffer_bytes(self.max_tbs)

    def reset(self, buf=None):
        """Empty buffer buf, or every buffer (None)."""
        self.ctx._check(self.ctx.L.mi_lte_harq_pool_reset(self.ctx.h, self.h, HARQ_NONE if buf is None else int(buf)))

    def _ptrs(self, buf):
        ps, pst = C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_harq_pool_soft(self.h, int(buf), C.byref(ps), C.byref(pst)))
        return ps.value, pst.value

    def state(self, buf):
        """The buffer's state record as a dict {tbs, C, K, N_cb, n_tx, status}."""
        st = HarqState()
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, C.addressof(st), self._ptrs(buf)[1], C.sizeof(st)))
        return {n: getattr(st, n) for n, _ in HarqState._fields_}

    def soft_raw(self, buf):
        """The whole int16 buffer (buffer_bytes / 2 positions), whatever it holds."""
        out = np.empty(self.buffer_bytes // 2, np.int16)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, self._ptrs(buf)[0], out.nbytes))
        return out

    def soft(self, buf):
        """The held transport block's code blocks, int16 [C, 3 (K + 4)] (C and K from the state; [0, 0] when empty)."""
        st = self.state(buf)
        n = st["C"] * 3 * (st["K"] + 4)
        return self.soft_raw(buf)[:n].reshape(st["C"], 3 * (st["K"] + 4) if st["C"] else 0)

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_harq_pool_destroy(self.ctx.h, self.h)
            self.h = None


class HostBuffer:
    """Pinned host memory (mi_lte_host_alloc) viewed as a numpy array: what the host-batch pipeline wants its arrays in."""

    def __init__(self, shape, dtype, device=None):
        """device: bind the pages to that device's NUMA node (mi_lte_host_alloc_on); self.node says whether that happened (-1: no)."""
        self.L = load_library()
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self.ptr = self.L.mi_lte_host_alloc(max(n, 1)) if device is None else self.L.mi_lte_host_alloc_on(device, max(n, 1))
        if not self.ptr:
            raise MiLteError("mi_lte_host_alloc(%d) failed" % n)
        self.node = self.L.mi_lte_host_alloc_node(self.ptr)
        self.arr = np.frombuffer((C.c_uint8 * max(n, 1)).from_address(self.ptr), dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self.ptr:
            self.arr = None
            self.L.mi_lte_host_free(self.ptr)
            self.ptr = None


class DlPipeline:
    """mi_lte_dl_pipeline: whole-chain batches from host buffers, chunks overlapped on several lanes."""

    def __init__(self, device, cfg, n_pdcch_symbs, unit_allocs, chunk_units, n_lanes=3, max_alloc_per_unit=0, max_soft_bytes_per_unit=0):
        """device: one ordinal or a list of them (chunk c of a run goes to devices[c % len]); unit_allocs: the allocation template every
        unit carries, or None for per-unit lists only (then max_alloc_per_unit bounds a unit's list)."""
        self.L = load_library()
        devs = list(device) if isinstance(device, (list, tuple)) else [device]
        darr = (C.c_int * len(devs))(*devs)
        h = C.c_void_p()
        if unit_allocs is not None:
            arr = (PdschAlloc * len(unit_allocs))(*unit_allocs)
            rc = self.L.mi_lte_dl_pipeline_create_multi(darr, len(devs), C.byref(cfg), n_pdcch_symbs, C.cast(arr, C.c_void_p), len(unit_allocs),
                                                        max_soft_bytes_per_unit, chunk_units, n_lanes, C.byref(h))
        else:
            rc = self.L.mi_lte_dl_pipeline_create_multi(darr, len(devs), C.byref(cfg), n_pdcch_symbs, None, max_alloc_per_unit, max_soft_bytes_per_unit,
                                                        chunk_units, n_lanes, C.byref(h))
        if rc != 0:
            raise MiLteError("mi_lte_dl_pipeline_create_multi failed: %d" % rc)
        self.h, self.n_alloc = h, len(unit_allocs) if unit_allocs is not None else 0
        self.out_stride = self.L.mi_lte_dl_pipeline_out_stride(h)
        self.unit_samples = self.L.mi_lte_dl_pipeline_unit_samples(h)
        self.n_devices = self.L.mi_lte_dl_pipeline_n_devices(h)
        self.tbs = [a.tbs for a in unit_allocs] if unit_allocs is not None else []

    def _err(self, what, rc):
        raise MiLteError("%s failed: %d (%s)" % (what, rc, self.L.mi_lte_dl_pipeline_last_error(self.h).decode()))

    def device_stats(self):
        """What every device slot did in the last run (mi_lte_dl_pipeline_device_stats), as a list of dicts."""
        out = []
        for i in range(self.n_devices):
            st = PipelineDevStats()
            if self.L.mi_lte_dl_pipeline_device_stats(self.h, i, C.byref(st)) != 0:
                raise MiLteError("mi_lte_dl_pipeline_device_stats failed")
            out.append({k: getattr(st, k) for k, _ in PipelineDevStats._fields_ if k != "reserved"})
        return out

    def run_units(self, h_iq, h_sf, h_cell, n_units, allocs, first, n_pdcch_symbs, h_out, h_status):
        """Per-unit allocation lists: allocs (ctypes array of PdschAlloc, sorted by unit), first uint32 [n_units + 1]."""
        first = np.ascontiguousarray(first, np.uint32)
        rc = self.L.mi_lte_dl_pipeline_run_units(self.h, h_iq.ctypes.data, h_sf.ctypes.data, h_cell.ctypes.data, n_units, C.cast(allocs, C.c_void_p),
                                                 first.ctypes.data, n_pdcch_symbs, h_out.ctypes.data, h_status.ctypes.data)
        if rc != 0:
            self._err("mi_lte_dl_pipeline_run_units", rc)

    def run_capture(self, h_capture, first_start, n_subframes, first_sf, cell, allocs, first, n_pdcch_symbs, h_out, h_status):
        """One contiguous int8 capture [n_samples, 2], split on subframe boundaries with the look-ahead halo."""
        first = np.ascontiguousarray(first, np.uint32)
        rc = self.L.mi_lte_dl_pipeline_run_capture(self.h, h_capture.ctypes.data, h_capture.shape[0], first_start, n_subframes, first_sf, cell,
                                                   C.cast(allocs, C.c_void_p), first.ctypes.data, n_pdcch_symbs, h_out.ctypes.data, h_status.ctypes.data)
        if rc != 0:
            self._err("mi_lte_dl_pipeline_run_capture", rc)

    def run(self, h_iq, h_sf, h_cell, n_units, h_out, h_status):
        """h_iq int8 [n_units, unit_samples, 2], h_sf / h_cell uint32 [n_units], h_out uint8 [n_units * n_alloc, out_stride], h_status int32:
        numpy arrays, ideally views of HostBuffer (pinned)."""
        rc = self.L.mi_lte_dl_pipeline_run(self.h, h_iq.ctypes.data, h_sf.ctypes.data, h_cell.ctypes.data, n_units, h_out.ctypes.data, h_status.ctypes.data)
        if rc != 0:
            raise MiLteError("mi_lte_dl_pipeline_run failed: %d (%s)" % (rc, self.L.mi_lte_dl_pipeline_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.L.mi_lte_dl_pipeline_destroy(self.h)
            self.h = None


class PuschPlan:
    """mi_lte_pusch_plan: PUSCH allocations (one per scheduled UE) over a batch of uplink subframe units.  spec: a plan in the 3GPP
    transport-block mode (mi_lte_pusch_plan_create_3gpp); uci: one UlschUci per allocation (mi_lte_pusch_plan_create_3gpp_uci)."""

    def __init__(self, ctx, cfg, ulcfg, unit_subfr_num, unit_n_id_cell, allocs, spec=False, uci=None):
        self.ctx, self.n_alloc, self.packed = ctx, len(allocs), False
        arr = (PdschAlloc * len(allocs))(*allocs)
        h = C.c_void_p()
        sf, cell = np.ascontiguousarray(unit_subfr_num, np.uint32), np.ascontiguousarray(unit_n_id_cell, np.uint32)
        if uci is not None:
            if not spec:
                raise MiLteError("control information on PUSCH needs a plan in the 3GPP transport-block mode (pusch_plan_3gpp)", -4)
            if len(uci) != len(allocs):
                raise ValueError("uci: one UlschUci per allocation")
            u_arr = (UlschUci * len(allocs))(*uci)
            rc = ctx.L.mi_lte_pusch_plan_create_3gpp_uci(ctx.h, C.byref(cfg), C.byref(ulcfg), sf, cell, len(sf), C.cast(arr, C.c_void_p), len(allocs),
                                                         C.cast(u_arr, C.c_void_p), C.byref(h))
            if rc != 0:
                raise MiLteError("libmi_lte error %d: %s" % (rc, ctx.L.mi_lte_last_error(ctx.h).decode()), rc)
        else:
            create = ctx.L.mi_lte_pusch_plan_create_3gpp if spec else ctx.L.mi_lte_pusch_plan_create
            ctx._check(create(ctx.h, C.byref(cfg), C.byref(ulcfg), sf, cell, len(sf), C.cast(arr, C.c_void_p), len(allocs), C.byref(h)))
        self.h = h
        self.out_stride = ctx.L.mi_lte_pusch_plan_out_stride(h)
        self.tbs = [a.tbs for a in allocs]

    def run_dev(self, d_subframes, d_out, d_status):
        self.ctx._check(self.ctx.L.mi_lte_pusch_decode_run(self.ctx.h, self.h, d_subframes.ptr, d_out.ptr, d_status.ptr))

    def run_harq_dev(self, pool, binds, d_subframes, d_out, d_status):
        """mi_lte_pusch_decode_run_harq (3GPP mode): binds is a ctypes array of HarqBind, one per allocation (harq_binds), or None -- a NULL
        binding, which the library refuses."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_decode_run_harq(self.ctx.h, self.h, pool.h, None if binds is None else C.cast(binds, C.c_void_p),
                                                                d_subframes.ptr, d_out.ptr, d_status.ptr))

    def run(self, d_subframes):
        """Returns (status int32 [n_alloc], list of uint8 bit arrays)."""
        ctx = self.ctx
        d_out, d_st = ctx.alloc(self.n_alloc * self.out_stride), ctx.alloc(4 * self.n_alloc)
        d_out.zero()
        try:
            self.run_dev(d_subframes, d_out, d_st)
            st = d_st.download(np.int32)
            bits = d_out.download(np.uint8).reshape(self.n_alloc, self.out_stride)
            if self.packed:  # back to one bit per byte for the caller
                return st, [np.unpackbits(bits[a, :(self.tbs[a] + 7) // 8])[:self.tbs[a]] for a in range(self.n_alloc)]
            return st, [bits[a, :self.tbs[a]] for a in range(self.n_alloc)]
        finally:
            d_out.free()
            d_st.free()

    def soft_bits(self, alloc):
        """De-interleaved, descrambled int8 soft bits of one allocation (stage tap)."""
        pe, n = C.c_void_p(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_soft_bits(self.h, alloc, C.byref(pe), C.byref(n)))
        out = np.empty(int(n.value), np.int8)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, pe.value, out.nbytes))
        return out

    def set_decoder(self, mode, n_iter=8, qpp_spec=1):
        """3GPP mode: TURBO_BCJR (default, 8 iterations), TURBO_BCJR_EARLY or TURBO_BCJR_BLOCK, exact interleaver."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_decoder(self.h, mode, n_iter, qpp_spec))

    def set_packed(self, packed=True):
        """3GPP mode: eight bits per byte (first bit in the most significant position) instead of one; changes out_stride."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_output(self.h, 1 if packed else 0))
        self.packed = bool(packed)
        self.out_stride = self.ctx.L.mi_lte_pusch_plan_out_stride(self.h)

    def cb_soft(self, alloc):
        """3GPP mode, after a run: the C rate-un-matched code blocks of one allocation, int8 [C, 3 (K + 4)] (stage tap)."""
        p, nc, k = C.c_void_p(), C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_cb_soft(self.h, alloc, C.byref(p), C.byref(nc), C.byref(k)))
        out = np.empty((nc.value, 3 * (k.value + 4)), np.int8)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def cb_ok(self):
        """3GPP mode, after a run: uint32 [n_alloc], bit r set when code block r's CRC24B passed (one block: bit 0 = the CRC24A verdict)."""
        p = C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_cb_ok(self.h, C.byref(p)))
        out = np.empty(self.n_alloc, np.uint32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def _tap(self, fn, alloc):
        p, n = C.c_void_p(), C.c_uint32()
        self.ctx._check(fn(self.h, alloc, C.byref(p), C.byref(n)))
        out = np.empty(int(n.value), np.int8)
        if out.nbytes:
            self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def data_soft(self, alloc):
        """Plan with control information, after a run: the allocation's G data soft bits in sequence order (what rate un-matching reads),
        0 where an ACK symbol overwrote one."""
        return self._tap(self.ctx.L.mi_lte_pusch_plan_data_soft, alloc)

    def cqi_soft(self, alloc):
        """Plan with control information, after a run: the allocation's Q_cqi CQI soft bits, 0 where an ACK symbol overwrote one."""
        return self._tap(self.ctx.L.mi_lte_pusch_plan_cqi_soft, alloc)

    def uci_results(self):
        """Plan with control information, after a run: one dict per allocation {ack: [2], ri: [2], S_ack: [3], S_ri: [3]} -- the decided
        HARQ-ACK and RI bits and the soft-bit sums behind them (all zero where the allocation has none)."""
        p = C.c_void_p()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_uci_results(self.h, C.byref(p)))
        rec = (UlschUciResult * self.n_alloc)()
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, C.addressof(rec), p.value, C.sizeof(rec)))
        return [{"ack": list(r.ack), "ri": list(r.ri), "S_ack": list(r.S_ack), "S_ri": list(r.S_ri)} for r in rec]

    def set_cqi_decode(self, O_list):
        """Plan with control information: decode the CQI of allocation a as O_list[a] information bits (0: left opaque) from the next run
        on (k_ulsch_cqi_decode behind k_ulsch_uci_decide); None turns decoding off again.  A refusal (MiLteError, -1) leaves the plan as
        it was: a plan without control information, O > CQI_MAX_BITS, O > 0 on an allocation without CQI."""
        if O_list is None:
            arr = None
        else:
            if len(O_list) != self.n_alloc:
                raise ValueError("set_cqi_decode: one O per allocation")
            arr = np.ascontiguousarray(O_list, np.uint32)
        rc = self.ctx.L.mi_lte_pusch_plan_set_cqi_decode(self.h, None if arr is None else arr.ctypes.data)
        if rc != 0:
            raise MiLteError("mi_lte_pusch_plan_set_cqi_decode failed: %d" % rc, rc)

    def cqi_results(self):
        """Plan with control information: one CqiResult.as_dict() per allocation -- all zero before a first run with decoding on and
        for allocations left opaque."""
        p = C.c_void_p()
        rc = self.ctx.L.mi_lte_pusch_plan_cqi_results(self.h, C.byref(p))
        if rc != 0:
            raise MiLteError("mi_lte_pusch_plan_cqi_results failed: %d" % rc, rc)
        rec = (CqiResult * self.n_alloc)()
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, C.addressof(rec), p.value, C.sizeof(rec)))
        return [r.as_dict() for r in rec]

    def set_demapper(self, mode, gain=0.0):
        """3GPP mode: DEMAP_REF (default, the reference's de-mapper) or DEMAP_MAXLOG (max-log LLRs weighted by the per-symbol reliability
        rho_s; gain 0: automatic per allocation, > 0: that gain for every allocation)."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_demapper(self.h, mode, gain))

    def _llr_floats(self, fn, shape):
        p = C.c_void_p()
        self.ctx._check(fn(self.h, C.byref(p)))
        out = np.empty(shape, np.float32)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out

    def llr_gain(self):
        """3GPP mode, after a MAXLOG run: float32 [n_alloc], the gain that run used per allocation (stage tap)."""
        return self._llr_floats(self.ctx.L.mi_lte_pusch_plan_llr_gain, self.n_alloc)

    def llr_rho(self):
        """3GPP mode, after a MAXLOG run: float32 [n_alloc, 12], the reliability rho_s of every data symbol (stage tap)."""
        return self._llr_floats(self.ctx.L.mi_lte_pusch_plan_llr_rho, (self.n_alloc, 12))

    def set_llr_noise(self, scale):
        """3GPP mode: scale > 0: MAXLOG runs use the noise-referenced gain g_a = scale / sigma2_a of the DMRS noise estimate in place of
        set_demapper's gain (so retransmissions combine on one scale); 0: off."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_llr_noise(self.h, scale))

    def llr_noise(self):
        """3GPP mode: float32 [n_alloc], sigma2_a of the last MAXLOG run with the noise gain on (stage tap; zeros before one)."""
        return self._llr_floats(self.ctx.L.mi_lte_pusch_plan_llr_noise, self.n_alloc)

    def set_rx_antennas(self, n_rx, ant_stride=0):
        """3GPP mode: MAXLOG runs combine n_rx = 2 or 4 receive antennas (maximum-ratio combining); the grid of antenna r of unit u is
        subframe r * ant_stride + u of the run's d_subframes, ant_stride >= the plan's units.  n_rx = 1: off."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_rx_antennas(self.h, n_rx, ant_stride))

    def rx_antennas(self):
        """(n_rx, ant_stride) as the plan holds them: (1, 0) by default"""
        n, s = C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_rx_antennas(self.h, C.byref(n), C.byref(s)))
        return int(n.value), int(s.value)

    def set_equaliser(self, mode):
        """3GPP mode: EQ_ZF (default, one zero-forcing tap per sub-carrier) or EQ_MMSE (the tap 1 / (P + sigma2) and LLRs at the
        post-equaliser SINR); an MMSE run needs set_demapper(DEMAP_MAXLOG) and set_llr_noise(scale > 0)."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_equaliser(self.h, mode))

    def equaliser(self):
        """EQ_ZF or EQ_MMSE as the plan holds it"""
        m = C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_equaliser(self.h, C.byref(m)))
        return int(m.value)

    def llr_nu(self):
        """3GPP mode, once EQ_MMSE was set: float32 [n_alloc, 12], the residual nu_s of the last MMSE run (stage tap; zeros before one)."""
        return self._llr_floats(self.ctx.L.mi_lte_pusch_plan_llr_nu, (self.n_alloc, 12))

    def set_llr_tap(self, on=True):
        """3GPP mode: have MAXLOG runs also store the de-mapper's input symbols (llr_symbols); off frees the buffer again."""
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_set_llr_tap(self.h, 1 if on else 0))

    def llr_symbols(self, alloc):
        """With set_llr_tap, after a MAXLOG run: complex64 [12, M], the equalised, pre-decoded and 1 / sqrt(M)-scaled symbols of one allocation."""
        p, n = C.c_void_p(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pusch_plan_llr_symbols(self.h, alloc, C.byref(p), C.byref(n)))
        out = np.empty(int(n.value), np.complex64)
        self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p.value, out.nbytes))
        return out.reshape(12, -1)

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_pusch_plan_destroy(self.ctx.h, self.h)
            self.h = None


class PrachPlan:
    """mi_lte_prach_plan: root-sequence spectra of one cell's PRACH configuration."""

    def __init__(self, ctx, cfg, prach_cfg, roots_fft=None):
        self.ctx = ctx
        h = C.c_void_p()
        if roots_fft is None:
            ctx._check(ctx.L.mi_lte_prach_plan_create(ctx.h, C.byref(cfg), C.byref(prach_cfg), C.byref(h)))
        else:
            re, im = np.ascontiguousarray(roots_fft[0], np.float32), np.ascontiguousarray(roots_fft[1], np.float32)
            ctx._check(ctx.L.mi_lte_prach_plan_create_roots(ctx.h, C.byref(cfg), C.byref(prach_cfg), re, im, re.shape[0], C.byref(h)))
        self.h = h
        self.n_roots = ctx.L.mi_lte_prach_plan_n_roots(h)
        self.occasion_samples = ctx.L.mi_lte_prach_occasion_samples(h)
        self.n_zc = 139 if prach_cfg.preamble_format == 4 else 839

    STAT = np.dtype([("sum", np.float32), ("max_val", np.float32), ("max_off", np.uint32), ("pad", np.uint32)])  # mi_lte_prach_corr_stat

    def tap_dev(self, d_a, d_b, d_start, n_occ):
        """For tests (mi_lte_prach_detect_tap): what the three kernels computed for n_occ occasions -- the kept bins complex64 [n_occ, N_zc],
        the per-root records STAT [n_occ, n_roots], the correlation power profiles float32 [n_occ, n_roots, N_zc]."""
        xhat = np.zeros((n_occ, self.n_zc), np.complex64)
        stats = np.zeros((n_occ, self.n_roots), self.STAT)
        power = np.zeros((n_occ, self.n_roots, self.n_zc), np.float32)
        self.ctx._check(self.ctx.L.mi_lte_prach_detect_tap(self.ctx.h, self.h, d_a.ptr, d_b.ptr if d_b is not None else None, d_start.ptr, n_occ,
                                                            xhat.ctypes.data, stats.ctypes.data, power.ctypes.data))
        return xhat, stats, power

    def detect_dev(self, d_a, d_b, d_start, n_occ):
        """(N_det_pre, det_pre, det_ta) uint32 arrays, one entry per occasion."""
        out = [np.zeros(n_occ, np.uint32) for _ in range(3)]
        self.ctx._check(self.ctx.L.mi_lte_prach_detect_run(self.ctx.h, self.h, d_a.ptr, d_b.ptr if d_b is not None else None, d_start.ptr,
                                                            n_occ, out[0], out[1], out[2]))
        return out

    def launch_dev(self, d_a, d_b, d_start, n_occ):
        """Queue the detection of n_occ occasions and return at once (mi_lte_prach_detect_launch); fetch() has the verdicts."""
        self.ctx._check(self.ctx.L.mi_lte_prach_detect_launch(self.ctx.h, self.h, d_a.ptr, d_b.ptr if d_b is not None else None, d_start.ptr, n_occ))
        self._pending = n_occ

    def fetch(self):
        """(N_det_pre, det_pre, det_ta) of the launch before it (waits for that launch only)."""
        n = self._pending
        out = [np.zeros(n, np.uint32) for _ in range(3)]
        self.ctx._check(self.ctx.L.mi_lte_prach_detect_fetch(self.ctx.h, self.h, out[0], out[1], out[2], n))
        self._pending = 0
        return out

    def detect(self, iq, occ_start):
        d_a, d_s = self.ctx.to_device(iq.astype(np.int8)), self.ctx.to_device(np.asarray(occ_start, np.uint64))
        try:
            return self.detect_dev(d_a, None, d_s, len(occ_start))
        finally:
            d_a.free()
            d_s.free()

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_prach_plan_destroy(self.ctx.h, self.h)
            self.h = None


class PdcchPlan:
    """mi_lte_pdcch_plan: PCFICH / PDCCH resource-element tables of the listed cells."""

    def __init__(self, ctx, cfg, cells, phich_res=1.0, phich_dur_extended=0, per_port_estimates=False):
        self.ctx = ctx
        h = C.c_void_p()
        cells = np.ascontiguousarray(cells, np.uint32)
        ctx._check(ctx.L.mi_lte_pdcch_plan_create(ctx.h, C.byref(cfg), float(phich_res), int(phich_dur_extended), 1 if per_port_estimates else 0, cells,
                                                  len(cells), C.byref(h)))
        self.h = h

    def decode_raw(self, d_subframes, d_sf, d_cell, n_units):
        """(rc[n], cfi[n], n_symbs[n], n_dci[n], ctypes array PdcchDci[n * 6]); the buffers are the plan's and are reused by the next call."""
        if getattr(self, "_n", None) != n_units:
            self._n = n_units
            self._out = [np.zeros(n_units, np.uint32) for _ in range(4)]
            self._dci = (PdcchDci * (6 * n_units))()
        rc, cfi, nsym, ndci = self._out
        self.ctx._check(self.ctx.L.mi_lte_pdcch_decode_run(self.ctx.h, self.h, d_subframes.ptr, d_sf.ptr, d_cell.ptr, n_units, rc, cfi, nsym, ndci,
                                                            self._dci))
        return rc, cfi, nsym, ndci, self._dci

    def decode_dev(self, d_subframes, d_sf, d_cell, n_units):
        """(rc[n], cfi[n], n_symbs[n], list of per-unit lists of PdcchDci)"""
        rc, cfi, nsym, ndci, dci = self.decode_raw(d_subframes, d_sf, d_cell, n_units)
        return rc.copy(), cfi.copy(), nsym.copy(), [[dci[6 * u + k] for k in range(int(ndci[u]))] for u in range(n_units)]

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_pdcch_plan_destroy(self.ctx.h, self.h)
            self.h = None


class PhichPlan:
    """mi_lte_phich_plan: the PHICH resource elements of the listed cells (include/mi_lte.h: "PHICH, 3GPP mode"); n_group groups of eight
    sequences per subframe."""

    def __init__(self, ctx, cfg, cells, phich_res=1.0, phich_dur_extended=0):
        self.ctx = ctx
        h = C.c_void_p()
        cells = np.ascontiguousarray(cells, np.uint32)
        ctx._check(ctx.L.mi_lte_phich_plan_create(ctx.h, C.byref(cfg), float(phich_res), int(phich_dur_extended), 0, cells, len(cells), C.byref(h)))
        self.h = h
        self.n_group = int(ctx.L.mi_lte_phich_plan_n_group(h))

    def out_bytes(self, n_units):
        return C.sizeof(PhichResult) * n_units * self.n_group * PHICH_N_SEQ

    def decode_dev(self, d_subframes, d_sf, d_cell, n_units, d_out=None):
        """mi_lte_phich_decode_run: every group and sequence of n_units device subframes.  With d_out (device memory, out_bytes(n_units))
        the call queues the kernel and returns None; without, it returns the records as a numpy record array [n_units, n_group, 8] with
        PhichResult's fields."""
        own = d_out is None
        if own:
            d_out = self.ctx.alloc(self.out_bytes(max(n_units, 1)))
        try:
            self.ctx._check(self.ctx.L.mi_lte_phich_decode_run(self.ctx.h, self.h, d_subframes.ptr, d_sf.ptr, d_cell.ptr, n_units, d_out.ptr))
            if not own:
                return None
            return d_out.download(np.uint8, self.out_bytes(n_units)).view(np.dtype(PhichResult)).reshape(n_units, self.n_group, PHICH_N_SEQ)
        finally:
            if own:
                d_out.free()

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_phich_plan_destroy(self.ctx.h, self.h)
            self.h = None


class PdcchSearchPlan:
    """mi_lte_pdcch_search_plan: the blind search over the whole control region (include/mi_lte.h: "PDCCH, 3GPP mode") for the listed cells
    and DCI sizes; the RNTI set is exactly what set_rntis was given last (empty at first)."""

    def __init__(self, ctx, cfg, cells, sizes, rntis=(), phich_res=1.0, any_cce=False, phich_dur_extended=0, regs_36211=False):
        self.ctx, self.cfg = ctx, cfg
        h = C.c_void_p()
        cells, sizes = np.ascontiguousarray(cells, np.uint32), np.ascontiguousarray(sizes, np.uint32)
        ctx._check(ctx.L.mi_lte_pdcch_search_plan_create(ctx.h, C.byref(cfg), float(phich_res), int(phich_dur_extended),
                                                         (PDCCH_SEARCH_ANY_CCE if any_cce else 0) | (PDCCH_SEARCH_36211_REGS if regs_36211 else 0), cells,
                                                         len(cells), sizes, len(sizes), C.byref(h)))
        self.h = h
        if len(rntis):
            try:
                self.set_rntis(rntis)
            except Exception:
                self.close()
                raise

    def set_rntis(self, rntis):
        """Replace the RNTI set (an empty list empties it); a value of 0 or above 0xFFFF is refused and the set stays as it was."""
        r = np.ascontiguousarray(rntis, np.int64).reshape(-1)
        if len(r) and (r.min() < 0 or r.max() > 0xFFFFFFFF):
            raise MiLteError("mi_lte_pdcch_search_plan_set_rntis: RNTI out of range", -1)
        self.ctx._check(self.ctx.L.mi_lte_pdcch_search_plan_set_rntis(self.ctx.h, self.h, np.ascontiguousarray(r, np.uint32), len(r)))

    def search_raw(self, d_subframes, d_sf, d_cell, n_units):
        """(cfi[n], n_cce[n], n_found[n], ctypes array PdcchFound[n * 16]); the buffers are the plan's and are reused by the next call."""
        if getattr(self, "_n", None) != n_units:
            self._n = n_units
            self._out = [np.zeros(n_units, np.uint32) for _ in range(3)]
            self._found = (PdcchFound * (PDCCH_SEARCH_MAX_FOUND * n_units))()
        cfi, ncce, nf = self._out
        self.ctx._check(self.ctx.L.mi_lte_pdcch_search_run(self.ctx.h, self.h, d_subframes.ptr, d_sf.ptr, d_cell.ptr, n_units, cfi, ncce, nf, self._found))
        return cfi, ncce, nf, self._found

    def search_dev(self, d_subframes, d_sf, d_cell, n_units):
        """(cfi[n], n_cce[n], n_found[n] -- the total, which may exceed the 16 kept --, per unit the list of PdcchFound.as_tuple() =
        (rnti, L, first CCE, n_bits, payload, metric, energy) in the order (L descending, CCE ascending, size position ascending))"""
        cfi, ncce, nf, found = self.search_raw(d_subframes, d_sf, d_cell, n_units)
        M = PDCCH_SEARCH_MAX_FOUND
        return cfi.copy(), ncce.copy(), nf.copy(), [[found[M * u + k].as_tuple() for k in range(min(int(nf[u]), M))] for u in range(n_units)]

    def soft(self, n_units):
        """The int8 soft bits of the last run, [n_units, 72 * the tables' largest N_cce] (positive = bit 0; 72 n_cce[u] valid per unit)."""
        p, stride = C.c_void_p(), C.c_uint32()
        self.ctx._check(self.ctx.L.mi_lte_pdcch_search_soft(self.h, C.byref(p), C.byref(stride)))
        out = np.zeros((n_units, stride.value), np.int8)
        if out.size:
            self.ctx._check(self.ctx.L.mi_lte_memcpy_d2h(self.ctx.h, out.ctypes.data, p, out.nbytes))
        return out

    def close(self):
        if self.h:
            self.ctx.L.mi_lte_pdcch_search_plan_destroy(self.ctx.h, self.h)
            self.h = None


class Transmitter:
    """The host-side transmit functions of one cell (mi_lte_tx): the reference's liblte_phy_map_crs / _pss / _sss, _bch_channel_encode,
    _pdsch_channel_encode and _create_dl_subframe on a grid of the reference's layout (tx_symb_re / _im: [4][16][1200]).  Host code, no GPU."""

    def __init__(self, fft_size, n_rb_dl, n_id_cell, n_ant=1):
        self.L = load_library()
        self.fft, self.n_rb, self.cell, self.n_ant = fft_size, n_rb_dl, n_id_cell, n_ant
        self.h = C.c_void_p()
        if self.L.mi_lte_tx_create(C.byref(self.h)) != 0:
            raise MiLteError("mi_lte_tx_create failed")
        self.re, self.im = np.zeros((4, 16, 1200), np.float32), np.zeros((4, 16, 1200), np.float32)
        self._keep = []

    def _g(self):
        return self.re, self.im

    def _ok(self, rc, what):
        if rc != 0:
            raise MiLteError("%s: %d (the reference's LIBLTE_ERROR_INVALID_INPUTS)" % (what, rc))

    def clear(self):
        self.re[:], self.im[:] = 0, 0

    def signals(self, subfr_num):
        """CRS in every subframe, PSS / SSS in subframes 0 and 5 (what LTE_fdd_dl_file_gen maps first)."""
        re, im = self._g()
        if subfr_num in (0, 5):
            self._ok(self.L.mi_lte_map_pss(self.n_rb, 12, self.cell % 3, self.n_ant, re, im), "mi_lte_map_pss")
            self._ok(self.L.mi_lte_map_sss(self.n_rb, 12, subfr_num, self.cell // 3, self.cell % 3, self.n_ant, re, im), "mi_lte_map_sss")
        self._ok(self.L.mi_lte_map_crs(self.n_rb, 12, subfr_num, self.cell, self.n_ant, re, im), "mi_lte_map_crs")

    def bch(self, mib_bits, sfn):
        re, im = self._g()
        b = np.ascontiguousarray(mib_bits, np.uint8)
        self._ok(self.L.mi_lte_bch_channel_encode(self.h, self.n_rb, 12, b, len(b), self.cell, self.n_ant, sfn, re, im), "mi_lte_bch_channel_encode")

    def pdsch(self, subfr_num, n_pdcch_symbs, allocs):
        """allocs: (PdschAlloc, transport-block bits) pairs -- the receive side's own allocation struct, so that the same list goes to a PDSCH plan."""
        arr = (TxAlloc * len(allocs))()
        self._keep = []
        for t, (a, bits) in zip(arr, allocs):
            b = np.ascontiguousarray(bits, np.uint8)
            self._keep.append(b)
            t.msg[0], t.msg_bits[0] = b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b)
            t.pre_coder_type, t.mod_type, t.chan_type, t.tbs, t.rv_idx, t.N_prb = 0, a.mod_type, 0, a.tbs, a.rv_idx, a.N_prb
            t.N_codewords, t.N_layers, t.tx_mode, t.rnti = 1, 1, a.tx_mode, a.rnti
            for s in range(2):
                for i in range(a.N_prb):
                    t.prb[s][i] = a.prb[s][i]
        re, im = self._g()
        self._ok(self.L.mi_lte_pdsch_channel_encode(self.h, self.n_rb, 12, arr, len(allocs), n_pdcch_symbs, self.cell, self.n_ant, subfr_num, re, im), "mi_lte_pdsch_channel_encode")

    def control(self, subfr_num, cfi, n_group_phich, phich_present=None, phich_b=None, dcis=(), n_rb_ul=None):
        """mi_lte_pdcch_channel_encode: the PCFICH, n_group_phich PHICH groups (phich_present / phich_b: uint8 [n_group, 8], which indicators
        are sent and their values, 1 = ACK) and one DCI per TxAlloc of dcis (format 1A for chan_type 0, format 0 for uplink grants) written
        into the grid.  Returns (Pcfich, Phich, N_pdcch_symbs) as the call leaves them."""
        pc, ph, n_symbs = Pcfich(), Phich(), C.c_uint32(0)
        pc.cfi = cfi
        for name, src in (("present", phich_present), ("b", phich_b)):
            if src is not None:
                src = np.asarray(src, np.uint8)
                for g in range(min(n_group_phich, 25)):
                    for s in range(8):
                        getattr(ph, name)[g][s] = int(src[g][s])
        arr = (TxAlloc * max(len(dcis), 1))(*dcis)
        re, im = self._g()
        self._ok(self.L.mi_lte_pdcch_channel_encode(self.h, self.n_rb, self.n_rb if n_rb_ul is None else n_rb_ul, 12, n_group_phich, 4, C.byref(pc), C.byref(ph), arr,
                                                    len(dcis), C.byref(n_symbs), self.cell, self.n_ant, 0, subfr_num, re, im), "mi_lte_pdcch_channel_encode")
        return pc, ph, n_symbs.value

    def samples(self, ant=0):
        """OFDM modulation of the grid's 14 symbols: (i, q) float32 of one subframe."""
        s = self.fft // 128
        n = 14 * self.fft + 2 * 10 * s + 12 * 9 * s
        i, q = np.zeros(n, np.float32), np.zeros(n, np.float32)
        re, im = self._g()
        self._ok(self.L.mi_lte_create_dl_subframe(self.fft, 12 * self.n_rb, 10 * s, 9 * s, re, im, ant, i, q),
                 "mi_lte_create_dl_subframe")
        return i, q

    def close(self):
        if self.h:
            self.L.mi_lte_tx_destroy(self.h)
            self.h = None


def pdcch_re_tables(n_rb_dl, n_ant, cell, phich_res, n_symbs):
    """(pcfich[16], cand[6, 288]) uint32 grid indices l*1200 + k (host function of the library)."""
    pc, cand = np.zeros(16, np.uint32), np.zeros((6, 288), np.uint32)
    rc = load_library().mi_lte_pdcch_re_tables(n_rb_dl, n_ant, cell, float(phich_res), n_symbs, pc, cand)
    if rc != 0:
        raise MiLteError("mi_lte_pdcch_re_tables failed: %d" % rc)
    return pc, cand


def dci_unpack(fmt, payload, n_bits, rnti, n_rb_dl, n_ant):
    """(rc, PdcchDci): the library's DCI 1A (fmt 0) / 1C (fmt 1) unpacker (host arithmetic)."""
    d = PdcchDci()
    L = load_library()
    f = L.mi_lte_dci_1a_unpack if fmt == 0 else L.mi_lte_dci_1c_unpack
    return f(int(payload), int(n_bits), int(rnti), int(n_rb_dl), int(n_ant), C.byref(d)), d


def pdcch_cce_tables(n_rb_dl, n_ant, cell, phich_res, n_symbs, regs_36211=False):
    """mi_lte_pdcch_cce_tables: (N_cce, uint32 [N_cce, 36] grid indices of every CCE's resource elements) as a search plan holds them."""
    n, out = C.c_uint32(), np.zeros(36 * 128, np.uint32)
    rc = load_library().mi_lte_pdcch_cce_tables(n_rb_dl, n_ant, cell, float(phich_res), n_symbs, PDCCH_SEARCH_36211_REGS if regs_36211 else 0, C.byref(n), out, 128)
    if rc != 0:
        raise MiLteError("mi_lte_pdcch_cce_tables failed: %d" % rc, rc)
    return n.value, out[:36 * n.value].reshape(-1, 36).copy()


def pdcch_search_space(rnti, subfr_num, n_cce, L):
    """mi_lte_pdcch_search_space: the first CCEs of the RNTI's UE-specific candidates at aggregation level L (36.213 9.1.1), duplicates kept."""
    out, n = np.zeros(6, np.uint32), C.c_uint32()
    rc = load_library().mi_lte_pdcch_search_space(int(rnti), int(subfr_num), int(n_cce), int(L), out, C.byref(n))
    if rc != 0:
        raise MiLteError("mi_lte_pdcch_search_space failed: %d" % rc, rc)
    return [int(x) for x in out[:n.value]]


def dci_0_1a_unpack_crnti(payload, n_bits, rnti, n_rb, n_ant=1):
    """(rc, DciCrnti): a C-RNTI's DCI format 0 / 1A (mi_lte_dci_0_1a_unpack_crnti, host arithmetic); rc 0, or 4 = no transport block of its own."""
    d = DciCrnti()
    rc = load_library().mi_lte_dci_0_1a_unpack_crnti(int(payload), int(n_bits), int(rnti), int(n_rb), int(n_ant), C.byref(d))
    if rc < 0:
        raise MiLteError("mi_lte_dci_0_1a_unpack_crnti failed: %d" % rc, rc)
    return rc, d


def ul_dmrs_pusch(ulcfg, n_id_cell, n_subfr, n_prb):
    """float32 [4, 12*n_prb]: dmrs_0_re, dmrs_0_im, dmrs_1_re, dmrs_1_im (host function of the library)."""
    out = np.zeros((4, 12 * n_prb), np.float32)
    rc = load_library().mi_lte_ul_dmrs_pusch(C.byref(ulcfg), n_id_cell, n_subfr, n_prb, out[0], out[1], out[2], out[3])
    if rc != 0:
        raise MiLteError("mi_lte_ul_dmrs_pusch failed: %d" % rc)
    return out


class Context:
    """One GPU + one stream.  Mirrors the role of LIBLTE_PHY_STRUCT: all scratch lives here."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.mi_lte_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise MiLteError("mi_lte_ctx_create(device=%d) failed with %d: no usable gfx950 GPU "
                             "(the product path has no CPU fallback)" % (device, rc))
        self.h = h
        self.device = device

    def _check(self, rc):
        if rc != 0:
            raise MiLteError("libmi_lte error %d: %s" % (rc, self.L.mi_lte_last_error(self.h).decode()))

    @property
    def device_name(self):
        return self.L.mi_lte_device_name(self.h).decode()

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def sync(self):
        self._check(self.L.mi_lte_sync(self.h))

    def timer_start(self):
        self._check(self.L.mi_lte_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._check(self.L.mi_lte_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile(self, on=True):
        self._check(self.L.mi_lte_profile_enable(self.h, 1 if on else 0))
        self._check(self.L.mi_lte_profile_reset(self.h))

    def profile_report(self):
        """{kernel: (launches, total_ms)} for every launch bracketed since profile() / the last reset."""
        out = {}
        for item in self.L.mi_lte_profile_report(self.h).decode().split(";"):
            if item:
                name, n, ms = item.rsplit(":", 2)
                out[name] = (int(n), float(ms))
        return out

    def last_kernels(self):
        return self.L.mi_lte_last_kernels(self.h).decode()

    # ---- front end --------------------------------------------------------------------------
    def subframe_floats(self, n_ant):
        return self.L.mi_lte_subframe_floats(n_ant)

    def dl_frontend_dev(self, cfg, d_a, d_b, d_start, d_sf, d_cell, n_units, d_subframes):
        self._check(self.L.mi_lte_dl_frontend_batch(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None,
                                                    d_start.ptr, d_sf.ptr, d_cell.ptr, n_units, d_subframes.ptr))

    def dl_crs_noise_dev(self, cfg, d_subframes, d_sf, d_cell, n_units, d_sigma2):
        """mi_lte_dl_crs_noise_run: the CRS noise estimate of n_units units of subframe planes (full or CE_COMPACT), float32 [n_units] into
        d_sigma2; asynchronous on the context's stream."""
        self._check(self.L.mi_lte_dl_crs_noise_run(self.h, C.byref(cfg), d_subframes.ptr, d_sf.ptr, d_cell.ptr, n_units, d_sigma2.ptr))

    def dl_crs_noise(self, cfg, d_subframes, subfr_num, n_id_cell):
        """Host convenience: float32 [n_units] for device planes d_subframes and host subframe / cell numbers."""
        n = len(subfr_num)
        d_sf, d_cell = self.to_device(np.asarray(subfr_num, np.uint32)), self.to_device(np.asarray(n_id_cell, np.uint32))
        d_s2 = self.alloc(4 * n)
        try:
            self.dl_crs_noise_dev(cfg, d_subframes, d_sf, d_cell, n, d_s2)
            return d_s2.download(np.float32)
        finally:
            for b in (d_sf, d_cell, d_s2):
                b.free()

    def dl_frontend(self, cfg, samples, unit_start, subfr_num, n_id_cell):
        """Host convenience.  samples: int8 [..., 2] interleaved I,Q, or a (i, q) pair of float32 arrays.
        Returns float32 [n_units, 2 + 2*N_ant, 16, 1200] = (symb_re, symb_im, ce_re[p].., ce_im[p]..)."""
        n = len(unit_start)
        if isinstance(samples, tuple):
            d_a, d_b = self.to_device(samples[0].astype(np.float32)), self.to_device(samples[1].astype(np.float32))
            cfg.sample_format = IQ_F32_PLANAR
        else:
            d_a, d_b = self.to_device(samples.astype(np.int8)), None
            cfg.sample_format = IQ_I8
        d_start = self.to_device(np.asarray(unit_start, np.uint64))
        d_sf = self.to_device(np.asarray(subfr_num, np.uint32))
        d_cell = self.to_device(np.asarray(n_id_cell, np.uint32))
        nf = self.subframe_floats(cfg.N_ant)
        d_out = self.alloc(n * nf * 4)
        d_out.zero()
        try:
            self.dl_frontend_dev(cfg, d_a, d_b, d_start, d_sf, d_cell, n, d_out)
            return d_out.download(np.float32).reshape(n, 2 + 2 * cfg.N_ant, 16, 1200)
        finally:
            for b in (d_a, d_b, d_start, d_sf, d_cell, d_out):
                if b is not None:
                    b.free()

    # ---- uplink ------------------------------------------------------------------------------
    def ul_subframe_floats(self):
        return self.L.mi_lte_ul_subframe_floats()

    def ul_frontend_dev(self, cfg, d_a, d_b, d_start, n_units, d_subframes):
        self._check(self.L.mi_lte_ul_frontend_batch(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None,
                                                    d_start.ptr, n_units, d_subframes.ptr))

    def ul_frontend(self, cfg, samples, unit_start, keep=False):
        """Host convenience: int8 [..., 2] samples -> float32 [n_units, 2, 16, 1200] (symb_re, symb_im); keep=True
        also returns the device buffer (caller frees)."""
        n = len(unit_start)
        d_a = self.to_device(samples.astype(np.int8))
        cfg.sample_format = IQ_I8
        d_start = self.to_device(np.asarray(unit_start, np.uint64))
        d_out = self.alloc(n * self.ul_subframe_floats() * 4)
        d_out.zero()
        try:
            self.ul_frontend_dev(cfg, d_a, None, d_start, n, d_out)
            host = d_out.download(np.float32).reshape(n, 2, 16, 1200)
            return (host, d_out) if keep else host
        finally:
            d_a.free()
            d_start.free()
            if not keep:
                d_out.free()

    def ul_subframe_decode(self, fft_size, n_rb_ul, i_samps, q_samps, subfr_num, cell, ulcfg, allocs, pucch=(), pucch_tables=None):
        """mi_lte_ul_subframe_decode_host: one uplink subframe (float32 sample arrays) in one call.  allocs: list of PdschAlloc; pucch: list of
        (format 0/1/2, N_1_p_pucch) with tables float32 [n, 352].  Returns (status int32 [n_alloc], list of bit arrays (None where the CRC failed),
        (pucch bits uint8 [n, 2], n_bits, rc))."""
        L = self.L
        if not getattr(L, "_ul_sf_bound", False):
            L.mi_lte_ul_subframe_decode_host.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(UlCfg), C.c_void_p,
                                                         C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
            L._ul_sf_bound = True
        n, npu = len(allocs), len(pucch)
        arr = (PdschAlloc * max(n, 1))(*allocs)
        i_s, q_s = np.ascontiguousarray(i_samps, np.float32), np.ascontiguousarray(q_samps, np.float32)
        out, nb, st = np.zeros((max(n, 1), 6144), np.uint8), np.zeros(max(n, 1), np.uint32), np.full(max(n, 1), -7, np.int32)
        pr = (PucchRes * max(npu, 1))(*[PucchRes(0, f, n1) for (f, n1) in pucch])
        tabs = np.ascontiguousarray(pucch_tables if pucch_tables is not None else np.zeros((1, 352)), np.float32)
        pb, pnb, prc = np.zeros((max(npu, 1), 2), np.uint8), np.zeros(max(npu, 1), np.uint32), np.zeros(max(npu, 1), np.uint32)
        rc = L.mi_lte_ul_subframe_decode_host(self.h, fft_size, n_rb_ul, i_s.ctypes.data, q_s.ctypes.data, subfr_num, cell, C.byref(ulcfg), C.cast(arr, C.c_void_p), n,
                                              out.ctypes.data, 6144, nb.ctypes.data, st.ctypes.data, C.cast(pr, C.c_void_p), tabs.ctypes.data, npu, pb.ctypes.data,
                                              pnb.ctypes.data, prc.ctypes.data)
        if rc < 0:
            self._check(rc)
        if rc != 0:
            raise MiLteError("mi_lte_ul_subframe_decode_host: invalid arguments (%d)" % rc)
        return st[:n], [out[a, :nb[a]].copy() if st[a] == 0 else None for a in range(n)], (pb[:npu], pnb[:npu], prc[:npu])

    def prach_plan(self, cfg, prach_cfg, roots_fft=None):
        return PrachPlan(self, cfg, prach_cfg, roots_fft)

    def pucch_decode_dev(self, n_rb_ul, d_subframes, res, tables):
        """res: list of (unit, format 0/1/2, N_1_p_pucch); tables float32 [n, 352] (mi_lte.h).  Returns (bits uint8 [n, 2], n_bits, rc)."""
        n = len(res)
        arr = (PucchRes * n)(*[PucchRes(*r) for r in res])
        bits, nb, rc = np.zeros((n, 2), np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._check(self.L.mi_lte_pucch_decode_run(self.h, n_rb_ul, 1, d_subframes.ptr, arr, np.ascontiguousarray(tables, np.float32).reshape(-1), n,
                                                   bits.reshape(-1), nb, rc))
        return bits, nb, rc

    def pucch2_decode_dev(self, n_rb_ul, d_subframes, n_units, res, tabs, d_out=None):
        """mi_lte_pucch2_decode_run: PUCCH formats 2 / 2a / 2b over n_units UL device subframes.  res: list of (unit, format 0/1/2, tab, A),
        tabs: list of Pucch2Tab (pucch2_table) that the resources index.  With d_out (device memory, 64 bytes per resource) the call
        queues the kernel and returns None; without, it returns the records as a numpy record array with Pucch2Result's fields."""
        n, nt = len(res), len(tabs)
        arr = (Pucch2Res * max(n, 1))(*[Pucch2Res(*r) for r in res])
        tarr = (Pucch2Tab * max(nt, 1))(*tabs)
        own = d_out is None
        if own:
            d_out = self.alloc(C.sizeof(Pucch2Result) * max(n, 1))
        try:
            self._check(self.L.mi_lte_pucch2_decode_run(self.h, n_rb_ul, d_subframes.ptr, n_units, arr, n, tarr, nt, d_out.ptr))
            if not own:
                return None
            return d_out.download(np.uint8, C.sizeof(Pucch2Result) * n).view(np.dtype(Pucch2Result))
        finally:
            if own:
                d_out.free()

    def coarse_timing_dev(self, cfg, d_a, d_b, n_slots, start=0):
        """CoarseTiming for samples resident in HBM (d_b None for int8 interleaved)."""
        out = CoarseTiming()
        self._check(self.L.mi_lte_coarse_timing_run(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, n_slots, C.byref(out)))
        return out

    def find_pss_dev(self, cfg, d_a, d_b, symb_starts, start=0):
        """(symb_starts[7] rewritten, N_id_2, pss_symb, pss_thresh, freq_offset)"""
        ss = np.ascontiguousarray(symb_starts, np.uint32).copy()
        n2, ps, th, fo = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float()
        self._check(self.L.mi_lte_find_pss_run(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, ss, C.byref(n2), C.byref(ps),
                                               C.byref(th), C.byref(fo)))
        return ss, n2.value, ps.value, th.value, fo.value

    def find_sss_dev(self, cfg, d_a, d_b, n_id_2, symb_starts, pss_thresh, start=0):
        """(found, N_id_1, frame_start_idx, symb_starts[7])"""
        ss = np.ascontiguousarray(symb_starts, np.uint32).copy()
        n1, fs, found = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.L.mi_lte_find_sss_run(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, n_id_2, ss, pss_thresh,
                                               C.byref(n1), C.byref(fs), C.byref(found)))
        return bool(found.value), n1.value, fs.value, ss

    # ---- taps of the three searches, for tests and not for callers (mi_lte_*_tap): what the kernels wrote, no verdicts.  `out`: the output
    # arrays to write into (float32, C-contiguous, of the documented shapes) where a test wants to see what a call leaves untouched.

    def coarse_timing_tap_dev(self, cfg, d_a, d_b, n_slots, start=0, out=None):
        """(corr complex64 [n_slots, n_slot] of k_cp_corr, acc float32 [n_slot] of k_cp_accum)"""
        n_slot = 15360 * cfg.fft_size // 2048
        corr, acc = out if out is not None else (np.zeros((n_slots, n_slot, 2), np.float32), np.zeros(n_slot, np.float32))
        assert corr.dtype == acc.dtype == np.float32 and corr.shape == (n_slots, n_slot, 2) and acc.shape == (n_slot,)
        assert corr.flags.c_contiguous and acc.flags.c_contiguous
        self._check(self.L.mi_lte_coarse_timing_tap(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, n_slots,
                                                    corr.ctypes.data, acc.ctypes.data))
        return corr.view(np.complex64)[..., 0], acc

    def find_pss_tap_dev(self, cfg, d_a, d_b, symb_starts, n_id_2, pss_symb, shift, start=0, out=None):
        """(rows float32 [84, 2, 1200], corr complex64 [84, 9], fine rows float32 [80, 2, 1200], fine corr complex64 [80]); the second pass runs
        for the caller's (n_id_2, pss_symb, shift): the tap forms no verdict of its own."""
        ss = np.ascontiguousarray(symb_starts, np.uint32)
        rows, corr, frows, fcorr = out if out is not None else (np.zeros((84, 2, 1200), np.float32), np.zeros((84, 9, 2), np.float32),
                                                                np.zeros((80, 2, 1200), np.float32), np.zeros((80, 2), np.float32))
        assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in (rows, corr, frows, fcorr))
        assert (rows.shape, corr.shape, frows.shape, fcorr.shape) == ((84, 2, 1200), (84, 9, 2), (80, 2, 1200), (80, 2))
        self._check(self.L.mi_lte_find_pss_tap(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, ss.ctypes.data, n_id_2, pss_symb,
                                               shift, rows.ctypes.data, corr.ctypes.data, frows.ctypes.data, fcorr.ctypes.data))
        return rows, corr.view(np.complex64)[..., 0], frows, fcorr.view(np.complex64)[..., 0]

    def find_sss_tap_dev(self, cfg, d_a, d_b, n_id_2, symb_starts, start=0, out=None):
        """(row float32 [2, 1200], corr complex64 [336]: N_id_1 i at 2 i (subframe 0's sequence) and 2 i + 1 (subframe 5's))"""
        ss = np.ascontiguousarray(symb_starts, np.uint32)
        row, corr = out if out is not None else (np.zeros((2, 1200), np.float32), np.zeros((336, 2), np.float32))
        assert row.dtype == corr.dtype == np.float32 and row.shape == (2, 1200) and corr.shape == (336, 2) and row.flags.c_contiguous and corr.flags.c_contiguous
        self._check(self.L.mi_lte_find_sss_tap(self.h, C.byref(cfg), d_a.ptr, d_b.ptr if d_b is not None else None, start, n_id_2, ss.ctypes.data,
                                               row.ctypes.data, corr.ctypes.data))
        return row, corr.view(np.complex64)[..., 0]

    def pbch_decode_dev(self, cfg, d_subframes, d_cell, n_units):
        """(N_ant[n] (0 = not decoded), offset[n], mib[n] = the 24 BCH bits, first bit in bit 23); cfg.N_ant must be 4."""
        out = [np.zeros(n_units, np.uint32) for _ in range(3)]
        self._check(self.L.mi_lte_pbch_decode_run(self.h, C.byref(cfg), d_subframes.ptr, d_cell.ptr, n_units, out[0], out[1], out[2]))
        return out

    def pdcch_plan(self, cfg, cells, phich_res=1.0, per_port_estimates=False):
        return PdcchPlan(self, cfg, cells, phich_res, 0, per_port_estimates)

    def phich_plan(self, cfg, cells, phich_res=1.0):
        """The PHICH decoder for the listed cells: PhichPlan.decode_dev gives metric, hi and the stage taps of every (group, sequence)."""
        return PhichPlan(self, cfg, cells, phich_res, 0)

    def pdcch_search_plan(self, cfg, cells, sizes, rntis=(), phich_res=1.0, any_cce=False, regs_36211=False):
        """The blind PDCCH search: every CCE-aligned candidate at L = 8, 4, 2, 1 against each of the DCI `sizes` (bits), hits reported for the
        RNTIs listed -- inside their own or the common search space, or anywhere with any_cce.  regs_36211: the tables of
        MI_LTE_PDCCH_SEARCH_36211_REGS (a standard eNodeB's positions, not the reference's)."""
        return PdcchSearchPlan(self, cfg, cells, sizes, rntis, phich_res, any_cce, regs_36211=regs_36211)

    def pusch_plan(self, cfg, ulcfg, unit_subfr_num, unit_n_id_cell, allocs, uci=None):
        """A reference-mode PUSCH plan.  It has no control information: a `uci` is refused (MiLteError, -4)."""
        return PuschPlan(self, cfg, ulcfg, unit_subfr_num, unit_n_id_cell, allocs, uci=uci)

    def pusch_plan_3gpp(self, cfg, ulcfg, unit_subfr_num, unit_n_id_cell, allocs, uci=None):
        """A PUSCH plan in the 3GPP transport-block mode: the spec-normalised demodulator (QPSK / 16QAM / 64QAM), 36.212 segmentation (any tbs
        of Table 7.1.7.2.1-1), BCJR x 8 with the exact interleaver by default.  uci: one UlschUci per allocation -- HARQ-ACK, RI and CQI
        multiplexed on the PUSCH (36.212 5.2.2.6-5.2.2.8); see PuschPlan.uci_results / cqi_soft / data_soft."""
        return PuschPlan(self, cfg, ulcfg, unit_subfr_num, unit_n_id_cell, allocs, spec=True, uci=uci)

    # ---- PDSCH ------------------------------------------------------------------------------
    def cqi_decode_batch(self, soft, descs):
        """mi_lte_cqi_decode_batch on host data: soft int8 [n], descs a list of (off, Q_cqi, O); one CqiResult.as_dict() per descriptor.
        A descriptor the kernel cannot serve (O of 0 or > CQI_MAX_BITS, Q_cqi of 0 or > CQI_MAX_Q, odd off) gives the all-zero record;
        one it would serve must lie inside soft."""
        soft = np.ascontiguousarray(soft, np.int8)
        arr = (CqiDesc * len(descs))(*[CqiDesc(off, q, o, 0) for off, q, o in descs])
        for d in arr:
            if 1 <= d.O <= CQI_MAX_BITS and 1 <= d.Q_cqi <= CQI_MAX_Q and d.off % 2 == 0 and d.off + d.Q_cqi > len(soft):
                raise ValueError("cqi_decode_batch: run at %d + %d past the %d soft bits" % (d.off, d.Q_cqi, len(soft)))
        d_soft, d_desc, d_out = self.alloc(max(soft.nbytes, 2)), self.alloc(C.sizeof(arr)), self.alloc(C.sizeof(CqiResult) * len(descs))
        try:
            if soft.nbytes:
                d_soft.upload(soft)
            self._check(self.L.mi_lte_memcpy_h2d(self.h, d_desc.ptr, C.addressof(arr), C.sizeof(arr)))
            self._check(self.L.mi_lte_cqi_decode_batch(self.h, d_soft.ptr, d_desc.ptr, len(descs), d_out.ptr))
            rec = (CqiResult * len(descs))()
            self._check(self.L.mi_lte_memcpy_d2h(self.h, C.addressof(rec), d_out.ptr, C.sizeof(rec)))
            return [r.as_dict() for r in rec]
        finally:
            d_soft.free()
            d_desc.free()
            d_out.free()

    def pdsch_plan(self, cfg, n_pdcch_symbs, allocs):
        return PdschPlan(self, cfg, n_pdcch_symbs, allocs)

    def pdsch_plan_3gpp(self, cfg, n_pdcch_symbs, allocs, n_soft, m_dl_harq=8):
        """A plan in the 3GPP transport-block mode (36.212 segmentation, any tbs of Table 7.1.7.2.1-1): BCJR x 8 with the exact interleaver
        by default; n_soft / m_dl_harq size the soft buffer (no default: the UE category's N_soft)."""
        return PdschPlan(self, cfg, n_pdcch_symbs, allocs, dlsch=DlschCfg(n_soft, m_dl_harq))

    def pdsch_plan_3gpp_txdiv(self, cfg, n_pdcch_symbs, allocs, n_soft, m_dl_harq=8):
        """pdsch_plan_3gpp for a cell of two or four CRS ports (mi_lte_pdsch_plan_create_3gpp_txdiv): every allocation in transmit diversity
        (tx_mode 2), code-block concatenation with N_L = 2; set_demapper(DEMAP_MAXLOG) runs the single-port plans' k_pdsch_demod_llr on the cell's port
        count (its runs are labelled k_pdsch_demod_llr_txd)."""
        return PdschPlan(self, cfg, n_pdcch_symbs, allocs, dlsch=DlschCfg(n_soft, m_dl_harq), txdiv=True)

    def harq_pool(self, n_buf, max_tbs=75376):
        """A HARQ soft-buffer pool (mi_lte_harq_pool_create) for the 3GPP plans of this context."""
        return HarqPool(self, n_buf, max_tbs)

    def pdsch_plan_dynamic(self, cfg, max_alloc, max_soft_bytes):
        return PdschPlan(self, cfg, 0, None, max_alloc, max_soft_bytes)

    def iq_to_planar(self, d_iq, n_samples, d_i, d_q):
        self._check(self.L.mi_lte_iq_i8_to_planar(self.h, d_iq.ptr, n_samples, d_i.ptr, d_q.ptr))

    def freq_shift(self, d_i, d_q, first_index, n_samples, freq_offset, fs):
        """LTE_fdd_dl_fs_samp_buf::freq_shift on planar float samples in HBM, in place."""
        self._check(self.L.mi_lte_freq_shift_run(self.h, d_i.ptr, d_q.ptr, first_index, n_samples, float(freq_offset), int(fs)))

    # ---- turbo -------------------------------------------------------------------------------
    def turbo_decode_dev(self, d_soft, soft_type, K, n_cb, d_out, mode=TURBO_REF, n_iter=8, qpp_spec=False):
        """Device-pointer form: everything already resident in HBM (what bench.py times)."""
        self._check(self.L.mi_lte_turbo_decode_batch(self.h, d_soft.ptr, soft_type, K, n_cb, mode, n_iter,
                                                     1 if qpp_spec else 0, d_out.ptr))

    def turbo_decode(self, soft, K, mode=TURBO_REF, n_iter=8, qpp_spec=False):
        """Host convenience: soft is [n_cb, 3*(K+4)] (float32 / int8 / int16), interleaved d[i*3+x]
        exactly as the reference's turbo_decode takes it; returns [n_cb, K] uint8 hard bits."""
        soft = np.ascontiguousarray(soft)
        assert soft.ndim == 2 and soft.shape[1] == 3 * (K + 4), soft.shape
        n_cb = soft.shape[0]
        d_in = self.to_device(soft)
        d_out = self.alloc(n_cb * K)
        try:
            self.turbo_decode_dev(d_in, _SOFT_OF_DTYPE[soft.dtype], K, n_cb, d_out, mode, n_iter, qpp_spec)
            return d_out.download(np.uint8).reshape(n_cb, K)
        finally:
            d_in.free()
            d_out.free()

    def device_copy_rate(self, nbytes=1 << 30, reps=10):
        """GB/s (read + written) of a 16-bytes-per-lane copy kernel on this device: the measured streaming rate."""
        out = C.c_double()
        self._check(self.L.mi_lte_device_copy_rate(self.h, C.c_size_t(nbytes), reps, C.byref(out)))
        return out.value

    def device_copy_rates(self):
        """The last device_copy_rate call's three kernel shapes: (one access per thread, the same non-temporal, grid-stride loop), GB/s."""
        out = (C.c_double * 3)()
        self._check(self.L.mi_lte_device_copy_rates(self.h, out))
        return tuple(round(v, 1) for v in out)

    def turbo_early_exit_iterations(self):
        """Iterations each tile pair (128 code blocks) of the last TURBO_BCJR_EARLY decode ran: uint32 [n_pairs]."""
        n, ni = C.c_uint32(), C.c_uint32()
        out = np.zeros(1 << 16, np.uint32)
        self._check(self.L.mi_lte_turbo_early_exit_iterations(self.h, out.ctypes.data, len(out), C.byref(n), C.byref(ni)))
        return out[:n.value].copy()

    def set_turbo_merged(self, on=True):
        """Several code-block sizes in one decode: one launch set over all of them (default) or, off, size by size (mi_lte_set_turbo_merged)."""
        self.L.mi_lte_set_turbo_merged.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.L.mi_lte_set_turbo_merged(self.h, 1 if on else 0))

    def set_soft_packed(self, on=True):
        """PDSCH plans hand 16QAM / 64QAM soft bits to the REF decoder one bit per soft bit (default) or, off, one byte (mi_lte_set_soft_packed)."""
        self.L.mi_lte_set_soft_packed.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.L.mi_lte_set_soft_packed(self.h, 1 if on else 0))

    def set_gold_recurrence(self, on=True):
        """The PDSCH demodulators' scrambling words in runs by recurrence (default) or, off, word by word from the tables (mi_lte_set_gold_recurrence)."""
        self.L.mi_lte_set_gold_recurrence.argtypes = [C.c_void_p, C.c_uint32]
        self._check(self.L.mi_lte_set_gold_recurrence(self.h, 1 if on else 0))

    def set_turbo_small_batch(self, n_cb_max):
        """Code blocks per decode up to which the REF decoder's state-parallel trellis kernel runs (0: always the lock-step one)."""
        self._check(self.L.mi_lte_set_turbo_small_batch(self.h, int(n_cb_max)))

    def close(self):
        if getattr(self, "h", None):
            self.L.mi_lte_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

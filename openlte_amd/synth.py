"""Synthetic inputs for benchmarks and tests, produced by the library's host-side transmitter
(csrc/synth.cc); independent of the test-side CPU checkers."""
import ctypes as C

import numpy as np

from .lib import load_library, MiLteError, DlCfg, UlCfg, PrachCfg, PdschAlloc, DlschCfg, UlschUci

_i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")


class SynthChannel(C.Structure):
    """mi_lte_synth_channel"""
    _fields_ = [("gain_min", C.c_double), ("gain_max", C.c_double), ("max_delay", C.c_double), ("snr_db", C.c_double),
                ("peak", C.c_double), ("seed", C.c_uint64)]


class SynthPaths(C.Structure):
    """mi_lte_synth_paths"""
    _fields_ = [("n_paths", C.c_uint32), ("delay", C.c_uint32 * 4), ("amp", C.c_double * 4)]


def _lib():
    L = load_library()
    if not getattr(L, "_synth_bound", False):
        L.mi_lte_synth_turbo_soft_i8.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_uint64, C.c_int, _i8p, _u8p]
        L.mi_lte_synth_turbo_soft_f32.argtypes = [C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_int, _f32p, _u8p]
        L.mi_lte_synth_unit_len.argtypes = [C.c_uint32]
        L.mi_lte_synth_unit_len.restype = C.c_size_t
        L.mi_lte_synth_dl_units_i8.argtypes = [C.POINTER(DlCfg), C.c_uint32, _u32p, _u32p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.POINTER(SynthChannel), _i8p, _u8p, C.c_uint32]
        L.mi_lte_synth_dl_units_3gpp_i8.argtypes = [C.POINTER(DlCfg), C.c_uint32, _u32p, _u32p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.POINTER(DlschCfg), C.POINTER(SynthChannel), _i8p, _u8p, C.c_uint32]
        L.mi_lte_synth_dl_units_3gpp_payload_i8.argtypes = [C.POINTER(DlCfg), C.c_uint32, _u32p, _u32p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                            C.POINTER(DlschCfg), C.POINTER(SynthChannel), C.c_void_p, C.c_uint32, _i8p]
        L.mi_lte_dlsch_encode_3gpp.argtypes = [C.c_uint32, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DlschCfg), _u8p]
        L.mi_lte_dlsch_encode_3gpp_nl.argtypes = [C.c_uint32, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DlschCfg), _u8p]
        L.mi_lte_txdiv_precode.argtypes = [C.c_uint32, _f32p, _f32p, C.c_uint32, _f32p, _f32p]
        L.mi_lte_synth_dl_units_3gpp_txdiv_i8.argtypes = [C.POINTER(DlCfg), C.c_uint32, _u32p, _u32p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                          C.POINTER(DlschCfg), C.POINTER(SynthChannel), C.c_void_p, C.c_uint32, _i8p, C.c_void_p]
        L.mi_lte_synth_ul_unit_len.argtypes = [C.c_uint32]
        L.mi_lte_synth_ul_unit_len.restype = C.c_size_t
        L.mi_lte_synth_ul_units_i8.argtypes = [C.POINTER(DlCfg), C.POINTER(UlCfg), C.c_uint32, _u32p, _u32p, C.c_void_p, C.c_uint32,
                                               C.POINTER(SynthChannel), _i8p, _u8p, C.c_uint32]
        L.mi_lte_synth_ul_units_3gpp_i8.argtypes = L.mi_lte_synth_ul_units_i8.argtypes
        L.mi_lte_ulsch_encode_3gpp.argtypes = [C.c_uint32, _u8p, C.c_uint32, C.c_uint32, C.c_uint32, _u8p]
        L.mi_lte_synth_ul_units_3gpp_uci_i8.argtypes = [C.POINTER(DlCfg), C.POINTER(UlCfg), C.c_uint32, _u32p, _u32p, C.c_void_p, C.c_uint32,
                                                        C.POINTER(SynthChannel), C.c_void_p, _u8p, _u8p, _u8p, C.c_uint32, _i8p, _u8p, C.c_uint32]
        L.mi_lte_synth_ul_units_3gpp_payload_i8.argtypes = [C.POINTER(DlCfg), C.POINTER(UlCfg), C.c_uint32, _u32p, _u32p, C.c_void_p, C.c_uint32,
                                                            C.POINTER(SynthChannel), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                            C.c_void_p, C.c_uint32, _i8p]
        L.mi_lte_synth_ul_units_3gpp_paths_i8.argtypes = [C.POINTER(DlCfg), C.POINTER(UlCfg), C.c_uint32, _u32p, _u32p, C.c_void_p, C.c_uint32,
                                                          C.POINTER(SynthChannel), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                                          C.c_void_p, C.c_uint32, C.POINTER(SynthPaths), _i8p]
        L.mi_lte_ulsch_mux_3gpp.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(UlschUci), _u8p, _u8p, _u8p, _u8p, C.c_uint32, _u8p, _u8p]
        L.mi_lte_synth_prach_len.argtypes = [C.c_uint32, C.c_uint32]
        L.mi_lte_synth_prach_len.restype = C.c_size_t
        L.mi_lte_synth_prach_i8.argtypes = [C.POINTER(DlCfg), C.POINTER(PrachCfg), C.c_uint32, _u32p, _u32p, C.POINTER(SynthChannel), _i8p]
        L.mi_lte_synth_ctrl_grids.argtypes = [C.POINTER(DlCfg), C.c_float, C.c_uint32, _u32p, _u32p, _u32p, _u32p, C.c_uint32,
                                              C.POINTER(SynthChannel), _f32p]
        L.mi_lte_synth_ctrl_grids_dci.argtypes = [C.POINTER(DlCfg), C.c_float, C.c_uint32, _u32p, _u32p, _u32p, C.c_void_p, C.c_uint32,
                                                  C.POINTER(SynthChannel), _f32p]
        L._synth_bound = True
    return L


class SynthDciRec(C.Structure):
    """mi_lte_synth_dci_rec"""
    _fields_ = [("rnti", C.c_uint32), ("L", C.c_uint32), ("cce", C.c_uint32), ("n_bits", C.c_uint32), ("payload", C.c_uint64)]


def turbo_soft_blocks(K, n, flip=0.02, amp=127, seed=1, ref_wrap=True):
    """(tx_bits [n,K] uint8, soft [n,3(K+4)] int8): turbo-encoded random blocks as hard +-amp soft values."""
    soft = np.zeros((n, 3 * (K + 4)), np.int8)
    tx = np.zeros((n, K), np.uint8)
    rc = _lib().mi_lte_synth_turbo_soft_i8(K, n, float(flip), int(amp), int(seed), 1 if ref_wrap else 0, soft, tx)
    if rc != 0:
        raise MiLteError("mi_lte_synth_turbo_soft_i8 failed: %d" % rc)
    return tx, soft


def turbo_soft_blocks_awgn(K, n, sigma=0.5, seed=1, ref_wrap=True):
    soft = np.zeros((n, 3 * (K + 4)), np.float32)
    tx = np.zeros((n, K), np.uint8)
    rc = _lib().mi_lte_synth_turbo_soft_f32(K, n, float(sigma), int(seed), 1 if ref_wrap else 0, soft, tx)
    if rc != 0:
        raise MiLteError("mi_lte_synth_turbo_soft_f32 failed: %d" % rc)
    return tx, soft


def unit_len(fft_size=2048):
    return int(_lib().mi_lte_synth_unit_len(fft_size))


def dl_units(cfg, subfr_num, n_id_cell, allocs, n_alloc, n_pdcch_symbs=2, gain=(0.5, 1.5), max_delay=8, snr_db=30.0,
             peak=100.0, seed=1):
    """Synthesise len(subfr_num) single-port subframe units.

    allocs: list of PdschAlloc, n_alloc per unit (unit-major).  Returns (iq int8 [n, unit_len, 2],
    tx_bits uint8 [n, n_alloc, max_tbs])."""
    n = len(subfr_num)
    ul = unit_len(cfg.fft_size)
    iq = np.zeros((n, ul, 2), np.int8)
    max_tbs = max([a.tbs for a in allocs], default=8)
    tx = np.zeros((n, max(n_alloc, 1), max_tbs), np.uint8)
    arr = (PdschAlloc * max(len(allocs), 1))(*allocs)
    ch = SynthChannel(gain[0], gain[1], float(max_delay), float(snr_db), float(peak), int(seed))
    rc = _lib().mi_lte_synth_dl_units_i8(C.byref(cfg), n, np.ascontiguousarray(subfr_num, np.uint32),
                                         np.ascontiguousarray(n_id_cell, np.uint32), n_pdcch_symbs,
                                         C.cast(arr, C.c_void_p), n_alloc, C.byref(ch), iq, tx, max_tbs)
    if rc != 0:
        raise MiLteError("mi_lte_synth_dl_units_i8 failed: %d" % rc)
    return iq, tx


def dl_units_3gpp(cfg, subfr_num, n_id_cell, allocs, n_alloc, n_soft, m_dl_harq=8, n_pdcch_symbs=2, gain=(0.5, 1.5), max_delay=8,
                  snr_db=30.0, peak=100.0, seed=1, payload=None):
    """dl_units with the 3GPP transport-block transmitter (mi_lte_synth_dl_units_3gpp_i8): any tbs of Table 7.1.7.2.1-1, E = G.
    payload: the transport blocks to send, uint8 [n_units, n_alloc, >= max tbs] one bit per byte (mi_lte_synth_dl_units_3gpp_payload_i8:
    a HARQ retransmission is the same payload with another rv and seed); returned as tx."""
    n = len(subfr_num)
    iq = np.zeros((n, unit_len(cfg.fft_size), 2), np.int8)
    max_tbs = max([a.tbs for a in allocs], default=8)
    tx = np.zeros((n, max(n_alloc, 1), max_tbs), np.uint8)
    arr = (PdschAlloc * max(len(allocs), 1))(*allocs)
    ch = SynthChannel(gain[0], gain[1], float(max_delay), float(snr_db), float(peak), int(seed))
    if payload is not None:
        pl = np.ascontiguousarray(payload, np.uint8)
        if pl.ndim != 3 or pl.shape[0] != n or pl.shape[1] != max(n_alloc, 1):
            raise ValueError("payload: uint8 [n_units, n_alloc, >= max tbs]")
        rc = _lib().mi_lte_synth_dl_units_3gpp_payload_i8(C.byref(cfg), n, np.ascontiguousarray(subfr_num, np.uint32),
                                                          np.ascontiguousarray(n_id_cell, np.uint32), n_pdcch_symbs, C.cast(arr, C.c_void_p), n_alloc,
                                                          C.byref(DlschCfg(n_soft, m_dl_harq)), C.byref(ch), pl.ctypes.data, pl.shape[2], iq)
        if rc != 0:
            raise MiLteError("mi_lte_synth_dl_units_3gpp_payload_i8 failed: %d" % rc, rc)
        return iq, pl[:, :, :max_tbs].copy()
    rc = _lib().mi_lte_synth_dl_units_3gpp_i8(C.byref(cfg), n, np.ascontiguousarray(subfr_num, np.uint32), np.ascontiguousarray(n_id_cell, np.uint32),
                                              n_pdcch_symbs, C.cast(arr, C.c_void_p), n_alloc, C.byref(DlschCfg(n_soft, m_dl_harq)), C.byref(ch), iq,
                                              tx, max_tbs)
    if rc != 0:
        raise MiLteError("mi_lte_synth_dl_units_3gpp_i8 failed: %d" % rc)
    return iq, tx


def dlsch_encode_3gpp(bits, G, Q_m, tx_mode=1, rv=0, n_soft=1237248, m_dl_harq=8, n_l=None):
    """mi_lte_dlsch_encode_3gpp: the G rate-matched bits (one per byte) of the transport block `bits`.  n_l: mi_lte_dlsch_encode_3gpp_nl with
    that N_L (2: transmit diversity)."""
    bits = np.ascontiguousarray(bits, np.uint8)
    e = np.zeros(max(G, 1), np.uint8)
    if n_l is None:
        rc = _lib().mi_lte_dlsch_encode_3gpp(len(bits), bits, G, Q_m, tx_mode, rv, C.byref(DlschCfg(n_soft, m_dl_harq)), e)
    else:
        rc = _lib().mi_lte_dlsch_encode_3gpp_nl(len(bits), bits, G, Q_m, n_l, tx_mode, rv, C.byref(DlschCfg(n_soft, m_dl_harq)), e)
    if rc != 0:
        raise MiLteError("mi_lte_dlsch_encode_3gpp failed: %d" % rc, rc)
    return e[:G]


def txdiv_precode(n_ant, d):
    """mi_lte_txdiv_precode: complex64 [n_ant, M_symb], what each port sends for the modulation symbols d (36.211 6.3.3.3 / 6.3.4.3)."""
    d = np.asarray(d, np.complex64).reshape(-1)
    re, im = np.ascontiguousarray(d.real, np.float32), np.ascontiguousarray(d.imag, np.float32)
    y_re, y_im = np.zeros((max(n_ant, 1), max(len(d), 1)), np.float32), np.zeros((max(n_ant, 1), max(len(d), 1)), np.float32)
    rc = _lib().mi_lte_txdiv_precode(n_ant, re, im, len(d), y_re.reshape(-1), y_im.reshape(-1))
    if rc != 0:
        raise MiLteError("mi_lte_txdiv_precode failed: %d" % rc, rc)
    return (y_re + 1j * y_im)[:, :len(d)].astype(np.complex64)


def dl_units_3gpp_txdiv(cfg, subfr_num, n_id_cell, allocs, n_alloc, n_soft, m_dl_harq=8, n_pdcch_symbs=2, gain=(0.5, 1.5), max_delay=8,
                        snr_db=30.0, peak=100.0, seed=1, payload=None):
    """dl_units_3gpp for a cell of cfg.N_ant = 2 or 4 ports (mi_lte_synth_dl_units_3gpp_txdiv_i8): CRS on every port, every allocation
    (tx_mode 2) in transmit diversity over the N_L = 2 concatenation, one delay per unit and a gain and a phase per port, the ports summed.
    payload as in dl_units_3gpp.  Returns (iq int8 [n, unit_len, 2], tx uint8 [n, n_alloc, max tbs])."""
    n = len(subfr_num)
    iq = np.zeros((n, unit_len(cfg.fft_size), 2), np.int8)
    max_tbs = max([a.tbs for a in allocs], default=8)
    tx = np.zeros((n, max(n_alloc, 1), max_tbs), np.uint8)
    arr = (PdschAlloc * max(len(allocs), 1))(*allocs)
    ch = SynthChannel(gain[0], gain[1], float(max_delay), float(snr_db), float(peak), int(seed))
    pl, stride = None, max_tbs
    if payload is not None:
        pl = np.ascontiguousarray(payload, np.uint8)
        if pl.ndim != 3 or pl.shape[0] != n or pl.shape[1] != max(n_alloc, 1) or pl.shape[2] < max_tbs:
            raise ValueError("payload: uint8 [n_units, n_alloc, >= max tbs]")
        tx, stride = np.zeros(pl.shape, np.uint8), pl.shape[2]
    rc = _lib().mi_lte_synth_dl_units_3gpp_txdiv_i8(C.byref(cfg), n, np.ascontiguousarray(subfr_num, np.uint32), np.ascontiguousarray(n_id_cell, np.uint32),
                                                    n_pdcch_symbs, C.cast(arr, C.c_void_p), n_alloc, C.byref(DlschCfg(n_soft, m_dl_harq)), C.byref(ch),
                                                    None if pl is None else pl.ctypes.data, stride, iq, tx.ctypes.data)
    if rc != 0:
        raise MiLteError("mi_lte_synth_dl_units_3gpp_txdiv_i8 failed: %d" % rc, rc)
    return iq, tx[:, :, :max_tbs].copy()


def ul_unit_len(fft_size=2048):
    return int(_lib().mi_lte_synth_ul_unit_len(fft_size))


def ul_units(cfg, ulcfg, subfr_num, n_id_cell, allocs, n_alloc, gain=(0.5, 1.5), max_delay=4, snr_db=30.0, peak=100.0, seed=1, spec=False):
    """Synthesise len(subfr_num) uplink subframe units, n_alloc PUSCH transmissions each (allocs unit-major).
    Returns (iq int8 [n, ul_unit_len, 2], tx_bits uint8 [n, n_alloc, max_tbs]).  spec: ul_units_3gpp."""
    n = len(subfr_num)
    ul = ul_unit_len(cfg.fft_size)
    iq = np.zeros((n, ul, 2), np.int8)
    max_tbs = max([a.tbs for a in allocs], default=8)
    tx = np.zeros((n, max(n_alloc, 1), max_tbs), np.uint8)
    arr = (PdschAlloc * max(len(allocs), 1))(*allocs)
    ch = SynthChannel(gain[0], gain[1], float(max_delay), float(snr_db), float(peak), int(seed))
    fn = _lib().mi_lte_synth_ul_units_3gpp_i8 if spec else _lib().mi_lte_synth_ul_units_i8
    rc = fn(C.byref(cfg), C.byref(ulcfg), n, np.ascontiguousarray(subfr_num, np.uint32), np.ascontiguousarray(n_id_cell, np.uint32),
            C.cast(arr, C.c_void_p), n_alloc, C.byref(ch), iq, tx, max_tbs)
    if rc != 0:
        raise MiLteError("mi_lte_synth_ul_units%s_i8 failed: %d" % ("_3gpp" if spec else "", rc), rc)
    return iq, tx


def ul_units_3gpp(cfg, ulcfg, subfr_num, n_id_cell, allocs, n_alloc, uci=None, ack=None, ri=None, cqi=None, gain=(0.5, 1.5), max_delay=4,
                  snr_db=30.0, peak=100.0, seed=1, payload=None, paths=None):
    """ul_units with the 3GPP UL-SCH transmitter (mi_lte_synth_ul_units_3gpp_i8): any tbs of Table 7.1.7.2.1-1, the exact interleaver.
    uci: one UlschUci per allocation (unit-major, as allocs) -- mi_lte_synth_ul_units_3gpp_uci_i8, with the control values the caller's:
    ack[k], ri[k] the allocation's information bits (sequences of O_ack / O_ri bits) and cqi[k] its Q_cqi coded CQI bits.
    payload: the transport blocks to send, uint8 [n_units, n_alloc, >= max tbs] one bit per byte (mi_lte_synth_ul_units_3gpp_payload_i8:
    a HARQ retransmission is the same payload with another rv and seed); returned as tx.
    paths: (delays, amps), a channel of 1 .. 4 paths (mi_lte_synth_ul_units_3gpp_paths_i8): delays[0] = 0, the further ones extra integer
    samples; amps relative, normalised inside.  Every path behind the first draws a phase of its own from the seed.  Without a payload one
    is drawn from numpy's generator seeded with `seed`."""
    n, na = len(subfr_num), len(allocs)
    max_tbs = max([a.tbs for a in allocs], default=8)
    arr = (PdschAlloc * max(na, 1))(*allocs)
    ch = SynthChannel(gain[0], gain[1], float(max_delay), float(snr_db), float(peak), int(seed))
    sf, cell = np.ascontiguousarray(subfr_num, np.uint32), np.ascontiguousarray(n_id_cell, np.uint32)
    iq = np.zeros((n, ul_unit_len(cfg.fft_size), 2), np.int8)
    ctrl = (None, None, None, None, 0)  # descriptors, ack, ri, cqi, cqi stride: the C entries' arguments, NULL without control information
    if uci is not None:
        if len(uci) != na:
            raise ValueError("uci: one UlschUci per allocation")
        stride = max([u.Q_cqi for u in uci] + [1])
        h_ack, h_ri, h_cqi = np.zeros((max(na, 1), 2), np.uint8), np.zeros((max(na, 1), 2), np.uint8), np.zeros((max(na, 1), stride), np.uint8)
        for k, u in enumerate(uci):
            for dst, src, cnt, what in ((h_ack, ack, u.O_ack, "ack"), (h_ri, ri, u.O_ri, "ri"), (h_cqi, cqi, u.Q_cqi, "cqi")):
                if cnt:
                    if src is None or len(src[k]) != cnt:
                        raise ValueError("%s[%d]: %d bits" % (what, k, cnt))
                    dst[k, :min(cnt, dst.shape[1])] = np.asarray(src[k], np.uint8)[:dst.shape[1]]  # (O > 2 is the library's to refuse)
        u_arr = (UlschUci * max(na, 1))(*uci)
        ctrl = (C.cast(u_arr, C.c_void_p), h_ack, h_ri, h_cqi, stride)
    if paths is not None and payload is None:
        payload = np.random.default_rng(seed).integers(0, 2, (n, max(n_alloc, 1), max_tbs), dtype=np.uint8)
    if payload is not None:
        pl = np.ascontiguousarray(payload, np.uint8)
        if pl.ndim != 3 or pl.shape[0] != n or pl.shape[1] != max(n_alloc, 1):
            raise ValueError("payload: uint8 [n_units, n_alloc, >= max tbs]")
        if paths is not None:
            delays, amps = paths
            if len(delays) != len(amps) or len(delays) > 4:
                raise ValueError("paths: (delays, amps), at most four of each")
            sp = SynthPaths(len(delays), (C.c_uint32 * 4)(*[int(d) for d in delays]), (C.c_double * 4)(*[float(a) for a in amps]))
            rc = _lib().mi_lte_synth_ul_units_3gpp_paths_i8(C.byref(cfg), C.byref(ulcfg), n, sf, cell, C.cast(arr, C.c_void_p), n_alloc, C.byref(ch),
                                                            *[None if v is None else v if isinstance(v, (int, C.c_void_p)) else v.ctypes.data for v in ctrl],
                                                            pl.ctypes.data, pl.shape[2], C.byref(sp), iq)
            if rc != 0:
                raise MiLteError("mi_lte_synth_ul_units_3gpp_paths_i8 failed: %d" % rc, rc)
            return iq, pl[:, :, :max_tbs].copy()
        rc = _lib().mi_lte_synth_ul_units_3gpp_payload_i8(C.byref(cfg), C.byref(ulcfg), n, sf, cell, C.cast(arr, C.c_void_p), n_alloc, C.byref(ch),
                                                          *[None if v is None else v if isinstance(v, (int, C.c_void_p)) else v.ctypes.data for v in ctrl],
                                                          pl.ctypes.data, pl.shape[2], iq)
        if rc != 0:
            raise MiLteError("mi_lte_synth_ul_units_3gpp_payload_i8 failed: %d" % rc, rc)
        return iq, pl[:, :, :max_tbs].copy()
    if uci is None:
        return ul_units(cfg, ulcfg, subfr_num, n_id_cell, allocs, n_alloc, gain=gain, max_delay=max_delay, snr_db=snr_db, peak=peak, seed=seed, spec=True)
    tx = np.zeros((n, max(n_alloc, 1), max_tbs), np.uint8)
    rc = _lib().mi_lte_synth_ul_units_3gpp_uci_i8(C.byref(cfg), C.byref(ulcfg), n, sf, cell, C.cast(arr, C.c_void_p), n_alloc, C.byref(ch), *ctrl, iq, tx, max_tbs)
    if rc != 0:
        raise MiLteError("mi_lte_synth_ul_units_3gpp_uci_i8 failed: %d" % rc, rc)
    return iq, tx


def ul_units_3gpp_rx(cfg, ulcfg, subfr_num, n_id_cell, allocs, n_alloc, n_rx, ant_stride=None, seeds=None, payload=None, seed=1, **kw):
    """n_rx receive-antenna captures of the same transmission, in the antenna-major order mi_lte_pusch_plan_set_rx_antennas reads: unit
    r * ant_stride + u is antenna r of unit u (ant_stride defaults to the number of units; units past it stay zero).  Every antenna is
    ul_units_3gpp with the same payload and a seed of its own (seeds[r], by default seed + 1000 r): another gain, phase, delay and noise.
    payload None: random transport blocks drawn from `seed`.  Further keywords (uci, ack, ri, cqi, gain, max_delay, snr_db, peak, paths) go to
    ul_units_3gpp.  Returns (iq int8 [n_rx * ant_stride, unit_len, 2], tx uint8 [n_units, n_alloc, max tbs])."""
    n = len(subfr_num)
    ant_stride = n if ant_stride is None else int(ant_stride)
    if ant_stride < n:
        raise ValueError("ant_stride: at least the number of units")
    seeds = [seed + 1000 * r for r in range(n_rx)] if seeds is None else list(seeds)
    if len(seeds) != n_rx:
        raise ValueError("seeds: one per antenna")
    max_tbs = max([a.tbs for a in allocs], default=8)
    if payload is None:
        payload = np.random.default_rng(seed).integers(0, 2, (n, max(n_alloc, 1), max_tbs), dtype=np.uint8)
    iq = np.zeros((n_rx * ant_stride, ul_unit_len(cfg.fft_size), 2), np.int8)
    tx = None
    for r in range(n_rx):
        iq[r * ant_stride:r * ant_stride + n], tx = ul_units_3gpp(cfg, ulcfg, subfr_num, n_id_cell, allocs, n_alloc, seed=seeds[r], payload=payload, **kw)
    return iq, tx


def ulsch_mux_3gpp(N_prb, Q_m, uci, f, ack=(), ri=(), cqi=(), c_init=0):
    """mi_lte_ulsch_mux_3gpp: (values before scrambling, 0 / 1 / 2 = x / 3 = y; bits after scrambling), each uint8 [12 * 12 N_prb * Q_m] in
    transmit order, of one allocation whose G coded data bits are f."""
    n = 12 * 12 * N_prb * Q_m
    pad = lambda v, m: np.concatenate([np.asarray(v, np.uint8).reshape(-1), np.zeros(m, np.uint8)])
    mux, scr = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    rc = _lib().mi_lte_ulsch_mux_3gpp(N_prb, Q_m, C.byref(uci), np.ascontiguousarray(f, np.uint8), pad(ack, 2), pad(ri, 2), pad(cqi, 1), c_init, mux, scr)
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_mux_3gpp failed: %d" % rc, rc)
    return mux[:n], scr[:n]


def ulsch_encode_3gpp(bits, G, Q_m, rv=0):
    """mi_lte_ulsch_encode_3gpp: the G rate-matched bits (one per byte, before the channel interleaver) of the transport block `bits`."""
    bits = np.ascontiguousarray(bits, np.uint8)
    e = np.zeros(max(G, 1), np.uint8)
    rc = _lib().mi_lte_ulsch_encode_3gpp(len(bits), bits, G, Q_m, rv, e)
    if rc != 0:
        raise MiLteError("mi_lte_ulsch_encode_3gpp failed: %d" % rc, rc)
    return e[:G]


def prach_occasions(cfg, prach_cfg, preamble_idx, delay, gain=(0.5, 1.5), snr_db=20.0, peak=100.0, seed=1):
    """int8 [n_occ, prach_len, 2]: one PRACH preamble per occasion (index preamble_idx[o] of the cell's 64, delayed by delay[o] samples)."""
    n = len(preamble_idx)
    ln = int(_lib().mi_lte_synth_prach_len(cfg.fft_size, prach_cfg.preamble_format))
    iq = np.zeros((n, ln, 2), np.int8)
    ch = SynthChannel(gain[0], gain[1], 0.0, float(snr_db), float(peak), int(seed))
    rc = _lib().mi_lte_synth_prach_i8(C.byref(cfg), C.byref(prach_cfg), n, np.ascontiguousarray(preamble_idx, np.uint32),
                                      np.ascontiguousarray(delay, np.uint32), C.byref(ch), iq)
    if rc != 0:
        raise MiLteError("mi_lte_synth_prach_i8 failed: %d" % rc)
    return iq


def ctrl_grids(cfg, subfr_num, n_id_cell, cfi, dcis, phich_res=1.0, gain=(0.6, 1.4), snr_db=10.0, seed=1):
    """Control regions as device-subframe grids, float32 [n, 2 + 2*N_ant, 16, 1200] (symbols 0-3 filled): PCFICH + the format-1A
    DCIs dcis[u] = [(rnti, mcs, N_prb, rb_start, rv_idx), ...] (at most 4, candidate = list position) with standard transmit
    diversity on cfg.N_ant ports."""
    n = len(subfr_num)
    n_dci = max([len(d) for d in dcis] + [1])
    tab = np.zeros((n, n_dci, 5), np.uint32)
    for u, lst in enumerate(dcis):
        for a, t in enumerate(lst):
            tab[u, a] = t
    g = np.zeros((n, 2 + 2 * cfg.N_ant, 16, 1200), np.float32)
    ch = SynthChannel(gain[0], gain[1], 0.0, float(snr_db), 0.0, int(seed))
    rc = _lib().mi_lte_synth_ctrl_grids(C.byref(cfg), float(phich_res), n, np.ascontiguousarray(subfr_num, np.uint32),
                                        np.ascontiguousarray(n_id_cell, np.uint32), np.ascontiguousarray(cfi, np.uint32), tab.reshape(-1), n_dci,
                                        C.byref(ch), g.reshape(-1))
    if rc != 0:
        raise MiLteError("mi_lte_synth_ctrl_grids failed: %d" % rc)
    return g


def ctrl_grids_dci(cfg, subfr_num, n_id_cell, cfi, recs, phich_res=1.0, gain=(0.6, 1.4), snr_db=10.0, seed=1):
    """ctrl_grids with any DCI anywhere (mi_lte_synth_ctrl_grids_dci): recs[u] = [(rnti, L, first CCE, n_bits, payload), ...], at most 8 per unit,
    the payload's first bit in bit n_bits - 1.  Records that overlap or reach past the unit's last CCE are refused (MiLteError, -1)."""
    n = len(subfr_num)
    n_rec = max([len(r) for r in recs] + [1])
    arr = (SynthDciRec * (n * n_rec))()
    for u, lst in enumerate(recs):
        for a, (rnti, L, cce, n_bits, payload) in enumerate(lst):
            arr[u * n_rec + a] = SynthDciRec(int(rnti), int(L), int(cce), int(n_bits), int(payload))
    g = np.zeros((n, 2 + 2 * cfg.N_ant, 16, 1200), np.float32)
    ch = SynthChannel(gain[0], gain[1], 0.0, float(snr_db), 0.0, int(seed))
    rc = _lib().mi_lte_synth_ctrl_grids_dci(C.byref(cfg), float(phich_res), n, np.ascontiguousarray(subfr_num, np.uint32),
                                            np.ascontiguousarray(n_id_cell, np.uint32), np.ascontiguousarray(cfi, np.uint32), C.cast(arr, C.c_void_p), n_rec,
                                            C.byref(ch), g.reshape(-1))
    if rc != 0:
        raise MiLteError("mi_lte_synth_ctrl_grids_dci failed: %d" % rc, rc)
    return g

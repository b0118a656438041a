"""openlte_amd -- MI355X-native LTE downlink receive chain behind the liblte_phy hot-path API.

The product is ``libmi_lte.so`` (hand-written HIP for gfx950 + a C-ABI, ``include/mi_lte.h``);
this package is only its ctypes binding plus small host-side helpers.  There is no CPU fallback:
importing works anywhere (so the C-ABI can be inspected), but creating a ``Context`` without the
built library or without a gfx950 GPU raises.
"""
from .lib import (Pucch2Tab, Pucch2Res, Pucch2Result, pucch2_table, pucch2_encode, pucch2_modulate, PUCCH2_MAX_BITS, PdcchSearchPlan, PdcchFound, DciCrnti, pdcch_search_space, pdcch_cce_tables, dci_0_1a_unpack_crnti, PDCCH_SEARCH_MAX_FOUND, PDCCH_SEARCH_ANY_CCE, PDCCH_SEARCH_36211_REGS, Transmitter, TxAlloc, DlCfg, UlCfg, PrachCfg, CoarseTiming, PdcchDci, dci_unpack, pdcch_re_tables, ul_dmrs_pusch, PdschAlloc, DlschCfg, dlsch_layout, ulsch_layout, UlschUci, ulsch_uci_qprime, ulsch_uci_G, ulsch_uci_map, UCI_ACK, UCI_RI, UCI_CQI, CqiResult, cqi_encode, CQI_NONE, CQI_NO_CRC, CQI_CRC_OK, CQI_CRC_FAIL, HarqPool, HarqBind, HarqState, harq_binds, harq_buffer_bytes, HARQ_NONE, HARQ_NEW_DATA, DEMAP_REF, DEMAP_MAXLOG, DEMAP_AUTO_T, EQ_ZF, EQ_MMSE, make_alloc, tile_allocs, IQ_I8, IQ_F32_PLANAR, IQ_ALL_ROWS, CE_COMPACT, Context, DeviceBuffer, HostBuffer, DlPipeline, MiLteError, build_library, library_path, load_library,
                  SOFT_F32, SOFT_I8, SOFT_I16, TURBO_REF, TURBO_BCJR, TURBO_BCJR_BLOCK, TURBO_BCJR_EARLY)

__all__ = ["Pucch2Tab", "Pucch2Res", "Pucch2Result", "pucch2_table", "pucch2_encode", "pucch2_modulate", "PUCCH2_MAX_BITS", "PdcchSearchPlan", "PdcchFound", "DciCrnti", "pdcch_search_space", "pdcch_cce_tables", "dci_0_1a_unpack_crnti", "PDCCH_SEARCH_MAX_FOUND", "PDCCH_SEARCH_ANY_CCE", "PDCCH_SEARCH_36211_REGS", "Transmitter", "TxAlloc", "DlCfg", "UlCfg", "PrachCfg", "CoarseTiming", "PdcchDci", "dci_unpack", "pdcch_re_tables", "ul_dmrs_pusch", "PdschAlloc", "DlschCfg", "dlsch_layout", "ulsch_layout", "UlschUci", "ulsch_uci_qprime", "ulsch_uci_G", "ulsch_uci_map", "UCI_ACK", "UCI_RI", "UCI_CQI", "CqiResult", "cqi_encode", "CQI_NONE", "CQI_NO_CRC", "CQI_CRC_OK", "CQI_CRC_FAIL", "HarqPool", "HarqBind", "HarqState", "harq_binds", "harq_buffer_bytes", "HARQ_NONE", "HARQ_NEW_DATA", "DEMAP_REF", "DEMAP_MAXLOG", "EQ_ZF", "EQ_MMSE", "DEMAP_AUTO_T", "make_alloc", "tile_allocs", "IQ_I8", "IQ_F32_PLANAR", "IQ_ALL_ROWS", "CE_COMPACT", "Context", "DeviceBuffer", "HostBuffer", "DlPipeline", "MiLteError", "build_library", "library_path", "load_library",
           "SOFT_F32", "SOFT_I8", "SOFT_I16", "TURBO_REF", "TURBO_BCJR", "TURBO_BCJR_BLOCK", "TURBO_BCJR_EARLY"]
from .lib import PhichPlan, PhichResult, Pcfich, Phich, phich_n_group, phich_resource, phich_re_table, PHICH_NO_POWER, PHICH_UNKNOWN_CELL, PHICH_N_SEQ  # noqa: E402

__all__ += ["PhichPlan", "PhichResult", "Pcfich", "Phich", "phich_n_group", "phich_resource", "phich_re_table", "PHICH_NO_POWER", "PHICH_UNKNOWN_CELL", "PHICH_N_SEQ"]

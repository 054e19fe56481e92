"""ctypes binding of the C ABI in include/spm_hip.h (libspm_amd/libspm_hip.so).

There is no CPU scan path: if the shared library is missing or HIP fails, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_PKG, "libspm_hip.so")
CSRC = os.path.join(_PKG, "csrc")

ALGO_SHIFTOR, ALGO_MYERS, ALGO_MYERS_PREFIX, ALGO_HORSPOOL = 0, 1, 2, 3
ENGINE_AUTO, ENGINE_BRUTE, ENGINE_FILTER = 0, 1, 2
SCAN_IGNORE_PACKED = 1
SCAN_DEFER = 2
SCAN_ALIGNABLE = 4  # spm_hip_jst_search only: the result keeps its segment hits for spm_hip_jst_hits_align
MAX_NEEDLE = 2048


class SpmError(RuntimeError):
    pass


class Hit(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("pattern", C.c_uint32), ("score", C.c_int32)]


class ScanOpts(C.Structure):
    _fields_ = [
        ("engine", C.c_uint32),
        ("left_context", C.c_uint32),
        ("pos_offset", C.c_uint64),
        ("max_hits", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class ScanStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_main", C.c_float),
        ("ms_verify", C.c_float),
        ("engine_used", C.c_uint32),
        ("fell_back", C.c_uint32),
        ("n_candidates", C.c_uint64),
        ("n_hits", C.c_uint64),
        ("main_launches", C.c_uint32),
        ("n_bands", C.c_uint32),
        ("fallback_spans", C.c_uint32),
        ("span_symbols", C.c_uint32),
        ("fallback_symbols", C.c_uint64),
    ]


class BuildStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_tables", C.c_float),
        ("ms_index", C.c_float),
        ("ms_upload", C.c_float),
        ("threads", C.c_uint32),
        ("passes", C.c_uint32),
        ("dense", C.c_uint32),
        ("anchor_sixteenths", C.c_uint32),
        ("keys", C.c_uint64),
        ("stride", C.c_uint32),
        ("key_len", C.c_uint32),
        ("bytes_device", C.c_uint64),
    ]


class JstAllele(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("ref_len", C.c_uint32), ("alt_len", C.c_uint32), ("alt_off", C.c_uint64)]


class JstHit(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("haplotype", C.c_uint32), ("pattern", C.c_uint32), ("score", C.c_int32),
                ("reserved", C.c_uint32)]


class JstStats(C.Structure):
    _fields_ = [
        ("haplotype_symbols", C.c_uint64),
        ("context_symbols", C.c_uint64),
        ("contexts", C.c_uint64),
        ("unique_contexts", C.c_uint64),
        ("n_blocks", C.c_uint64),
        ("block_len", C.c_uint32),
        ("window", C.c_uint32),
        ("ms_index", C.c_float),
        ("ms_scan", C.c_float),
        ("ms_main", C.c_float),
        ("ms_verify", C.c_float),
        ("ms_fanout", C.c_float),
        ("engine_used", C.c_uint32),
        ("main_launches", C.c_uint32),
        ("fell_back", C.c_uint32),
        ("segment_hits", C.c_uint64),
        ("candidates", C.c_uint64),
        ("bands", C.c_uint64),
    ]


class Aln(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64), ("pattern", C.c_uint32), ("score", C.c_int32),
                ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32)]


class AlignStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_begin", C.c_float),
        ("ms_cigar", C.c_float),
        ("ms_host", C.c_float),
        ("n_alns", C.c_uint64),
        ("n_ops", C.c_uint64),
        ("begin_lane", C.c_uint32),
        ("begin_wave", C.c_uint32),
        ("cigar_lane", C.c_uint32),
        ("cigar_wave", C.c_uint32),
        ("cigar_wave_global", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class JstAln(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64), ("haplotype", C.c_uint32), ("pattern", C.c_uint32),
                ("score", C.c_int32), ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32), ("reserved", C.c_uint32)]


class JstAlignStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_begin", C.c_float),
        ("ms_cigar", C.c_float),
        ("ms_fanout", C.c_float),
        ("ms_host", C.c_float),
        ("ms_worklist", C.c_float),
        ("n_alns", C.c_uint64),
        ("n_segment_alns", C.c_uint64),
        ("n_ops", C.c_uint64),
        ("begin_lane", C.c_uint32),
        ("begin_wave", C.c_uint32),
        ("cigar_lane", C.c_uint32),
        ("cigar_wave", C.c_uint32),
        ("cigar_wave_global", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class JstRefAln(C.Structure):
    _fields_ = [("ref_begin", C.c_uint64), ("ref_end", C.c_uint64), ("haplotype", C.c_uint32), ("pattern", C.c_uint32),
                ("score", C.c_int32), ("ref_score", C.c_int32), ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32)]


class JstProjectStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_representatives", C.c_float),
        ("ms_count", C.c_float),
        ("ms_emit", C.c_float),
        ("ms_gather", C.c_float),
        ("ms_host", C.c_float),
        ("n_alns", C.c_uint64),
        ("n_projected", C.c_uint64),
        ("n_ops", C.c_uint64),
        ("n_inside_insertion", C.c_uint64),
        ("n_changed", C.c_uint64),
    ]


class JstRefLocus(C.Structure):
    _fields_ = [("ref_begin", C.c_uint64), ("ref_end", C.c_uint64), ("pattern", C.c_uint32), ("ref_score", C.c_int32),
                ("score", C.c_int32), ("n_records", C.c_uint32), ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32),
                ("member_off", C.c_uint32), ("n_haplotypes", C.c_uint32)]


class JstCollapseStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_slots", C.c_float),
        ("ms_order", C.c_float),
        ("ms_records", C.c_float),
        ("ms_emit", C.c_float),
        ("ms_host", C.c_float),
        ("n_alns", C.c_uint64),
        ("n_slots", C.c_uint64),
        ("n_loci", C.c_uint64),
        ("n_members", C.c_uint64),
        ("n_ops", C.c_uint64),
        ("n_multi_slot", C.c_uint64),
        ("max_run", C.c_uint64),
    ]


class JstRead(C.Structure):
    _fields_ = [("first_locus", C.c_uint32), ("n_loci", C.c_uint32), ("n_forward", C.c_uint32), ("primary", C.c_uint32),
                ("best", C.c_int32), ("best_ref_score", C.c_int32), ("n_best", C.c_uint32), ("n_next", C.c_uint32)]


class JstReadsStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_host", C.c_float),
        ("n_reads", C.c_uint64),
        ("n_loci", C.c_uint64),
        ("n_mapped", C.c_uint64),
        ("n_unique", C.c_uint64),
        ("n_multi", C.c_uint64),
    ]


class JstPairOpts(C.Structure):
    _fields_ = [("min_tlen", C.c_uint32), ("max_tlen", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class JstPair(C.Structure):
    _fields_ = [("locus1", C.c_uint32), ("locus2", C.c_uint32), ("tlen", C.c_int32), ("best", C.c_int32),
                ("n_pairs", C.c_uint32), ("n_best", C.c_uint32), ("n_next", C.c_uint32), ("flag1", C.c_uint16), ("flag2", C.c_uint16)]


class JstPairsStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_host", C.c_float),
        ("n_pairs", C.c_uint64),
        ("n_proper", C.c_uint64),
        ("n_unique", C.c_uint64),
        ("n_multi", C.c_uint64),
        ("n_discordant", C.c_uint64),
        ("n_one_mate", C.c_uint64),
        ("n_unmapped", C.c_uint64),
        ("max_window", C.c_uint64),
    ]


class JstRescueOpts(C.Structure):
    _fields_ = [("min_tlen", C.c_uint32), ("max_tlen", C.c_uint32), ("k", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class JstRescue(C.Structure):
    _fields_ = [("ref_begin", C.c_uint64), ("ref_end", C.c_uint64), ("pair", C.c_uint32), ("pattern", C.c_uint32),
                ("anchor", C.c_uint32), ("score", C.c_int32), ("cigar_off", C.c_uint32), ("cigar_len", C.c_uint32),
                ("tlen", C.c_int32), ("flag", C.c_uint16), ("status", C.c_uint16)]


RESCUE_RESCUED, RESCUE_NONE, RESCUE_NOT_CONCORDANT = 0, 1, 2


class JstRescuesStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_jobs", C.c_float),
        ("ms_search", C.c_float),
        ("ms_align", C.c_float),
        ("ms_emit", C.c_float),
        ("ms_host", C.c_float),
        ("n_pairs", C.c_uint64),
        ("n_jobs", C.c_uint64),
        ("n_rescued", C.c_uint64),
        ("n_none", C.c_uint64),
        ("n_not_concordant", C.c_uint64),
        ("n_short", C.c_uint64),
        ("max_window", C.c_uint64),
    ]


class SamOpts(C.Structure):
    _fields_ = [("rname", C.c_char_p), ("symbols", C.c_char_p), ("names", C.c_void_p), ("name_off", C.c_void_p),
                ("n_names", C.c_uint64), ("mapq_unique", C.c_uint8 * 4), ("mapq_multi", C.c_uint8 * 4),
                ("mapq_defaults", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class SamLine(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint32), ("read", C.c_uint32), ("source", C.c_uint32),
                ("flag", C.c_uint16), ("mapq", C.c_uint8), ("kind", C.c_uint8)]


SAM_CIGAR_M, SAM_SECONDARY = 1, 2
SAM_MD = 1  # spm_sam_extras.flags


class SamExtras(C.Structure):
    _fields_ = [("qual", C.c_void_p), ("n_qual", C.c_uint64), ("reference", C.c_void_p), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]
SAM_UNMAPPED, SAM_LOCUS, SAM_RESCUE, SAM_SECONDARY_LINE = 0, 1, 2, 3


class BamOpts(C.Structure):
    _fields_ = [("sam", SamOpts), ("ref_len", C.c_uint64), ("block_data", C.c_uint32), ("reserved", C.c_uint32)]


class BamStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_lines", C.c_float),
        ("ms_measure", C.c_float),
        ("ms_write", C.c_float),
        ("ms_frame", C.c_float),
        ("ms_stats", C.c_float),
        ("ms_host", C.c_float),
        ("reserved", C.c_uint32),
        ("n_records", C.c_uint64),
        ("n_record_bytes", C.c_uint64),
        ("n_file_bytes", C.c_uint64),
        ("header_file_bytes", C.c_uint64),
        ("n_record_blocks", C.c_uint64),
        ("n_reported", C.c_uint64),
        ("n_secondary", C.c_uint64),
        ("n_unmapped", C.c_uint64),
        ("n_rescue_lines", C.c_uint64),
    ]


class BamSortOpts(C.Structure):
    _fields_ = [("reserved", C.c_uint64)]


class BamSortStats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_keys", C.c_float), ("ms_sort", C.c_float), ("ms_place", C.c_float),
                ("ms_gather", C.c_float), ("ms_frame", C.c_float), ("ms_host", C.c_float), ("key_bits", C.c_uint32),
                ("n_records", C.c_uint64), ("n_record_bytes", C.c_uint64)]


class BamMarkdupOpts(C.Structure):
    _fields_ = [("min_qual", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class BamMarkdupStats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_keys", C.c_float), ("ms_sort", C.c_float), ("ms_mark", C.c_float),
                ("ms_write", C.c_float), ("ms_frame", C.c_float), ("ms_host", C.c_float), ("reserved", C.c_uint32),
                ("n_records", C.c_uint64), ("n_pairs", C.c_uint64), ("n_fragments", C.c_uint64), ("n_dup_pairs", C.c_uint64),
                ("n_dup_fragments", C.c_uint64), ("n_dup_records", C.c_uint64), ("n_fragments_beside_pairs", C.c_uint64)]


class PileupOpts(C.Structure):
    _fields_ = [("begin", C.c_uint64), ("end", C.c_uint64), ("exclude_flags", C.c_uint32), ("min_mapq", C.c_uint8),
                ("min_baseq", C.c_uint8), ("reserved0", C.c_uint16), ("flags", C.c_uint32), ("reserved1", C.c_uint32)]


class PileupStats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_records", C.c_float), ("ms_scan", C.c_float), ("ms_tiles", C.c_float),
                ("ms_summary", C.c_float), ("ms_host", C.c_float), ("tile_positions", C.c_uint32), ("reserved", C.c_uint32),
                ("n_records", C.c_uint64), ("n_taking_part", C.c_uint64), ("n_evidence", C.c_uint64), ("n_covered", C.c_uint64),
                ("sum_depth", C.c_uint64), ("max_depth", C.c_uint64), ("n_tile_visits", C.c_uint64)]


class PileupSite(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("depth", C.c_uint32), ("alt", C.c_uint32), ("counts", C.c_uint32 * 4), ("ref", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class PileupSiteOpts(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("min_alt_permille", C.c_uint32), ("flags", C.c_uint32)]


PILEUP_PLANES = ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")  # SPM_PILEUP_A .. SPM_PILEUP_LOWQ


class VcfOpts(C.Structure):
    _fields_ = [("ploidy", C.c_uint32), ("cost_match", C.c_uint32), ("cost_het", C.c_uint32), ("cost_miss", C.c_uint32),
                ("prior_het", C.c_uint32), ("prior_hom_alt", C.c_uint32), ("min_qual", C.c_uint32), ("flags", C.c_uint32),
                ("reserved0", C.c_uint32), ("reserved1", C.c_uint32)]


class VariantCall(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("depth", C.c_uint32), ("qual", C.c_uint32), ("len", C.c_uint32), ("offset", C.c_uint64),
                ("status", C.c_uint8), ("gq", C.c_uint8), ("gt", C.c_uint8 * 2), ("n_alt", C.c_uint8), ("alt", C.c_uint8 * 2),
                ("reserved", C.c_uint8)]


class VcfStats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_call", C.c_float), ("ms_scan", C.c_float), ("ms_write", C.c_float),
                ("ms_host", C.c_float), ("group_sites", C.c_uint32), ("n_sites", C.c_uint64), ("n_variant", C.c_uint64),
                ("n_ref", C.c_uint64), ("n_ref_n", C.c_uint64), ("n_low_qual", C.c_uint64), ("n_header_bytes", C.c_uint64),
                ("n_text_bytes", C.c_uint64)]


CALL_REF, CALL_VARIANT, CALL_REF_N = 0, 1, 2  # SPM_CALL_*


class BaiStats(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_records", C.c_float), ("ms_chunks", C.c_float), ("ms_bins", C.c_float),
                ("ms_write", C.c_float), ("ms_host", C.c_float), ("n_bins", C.c_uint64), ("n_chunks", C.c_uint64),
                ("n_intv", C.c_uint64), ("n_mapped", C.c_uint64), ("n_unmapped", C.c_uint64), ("n_no_coor", C.c_uint64),
                ("n_bytes", C.c_uint64)]


class BgzfOpts(C.Structure):
    _fields_ = [("block_data", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class BgzfStats(C.Structure):
    _fields_ = [("ms_frame", C.c_float), ("ms_host", C.c_float), ("n_in", C.c_uint64), ("n_out", C.c_uint64),
                ("n_blocks", C.c_uint64)]


BGZF_EOF, BGZF_DYNAMIC, BGZF_BLOCK_DATA = 1, 4, 65280


class BgzfDeflateOpts(C.Structure):
    _fields_ = [("block_data", C.c_uint32), ("flags", C.c_uint32), ("level", C.c_uint32), ("reserved", C.c_uint32)]


class BgzfDeflateStats(C.Structure):
    _fields_ = [("ms_parse", C.c_float), ("ms_scan", C.c_float), ("ms_place", C.c_float), ("ms_host", C.c_float),
                ("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_blocks", C.c_uint64), ("n_stored_blocks", C.c_uint64),
                ("n_matches", C.c_uint64), ("n_literals", C.c_uint64), ("n_prefix_bytes", C.c_uint64)]


class SamStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_lines", C.c_float),
        ("ms_measure", C.c_float),
        ("ms_write", C.c_float),
        ("ms_stats", C.c_float),
        ("ms_host", C.c_float),
        ("n_lines", C.c_uint64),
        ("n_bytes", C.c_uint64),
        ("n_reported", C.c_uint64),
        ("n_secondary", C.c_uint64),
        ("n_unmapped", C.c_uint64),
        ("n_rescue_lines", C.c_uint64),
    ]


class JstNormalizeStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_slots", C.c_float),
        ("ms_normalize", C.c_float),
        ("ms_offsets", C.c_float),
        ("ms_gather", C.c_float),
        ("ms_compact", C.c_float),
        ("ms_host", C.c_float),
        ("reserved", C.c_float),
        ("n_alns", C.c_uint64),
        ("n_slots", C.c_uint64),
        ("n_ops_in", C.c_uint64),
        ("n_ops", C.c_uint64),
        ("n_changed", C.c_uint64),
        ("n_steps", C.c_uint64),
        ("n_joined", C.c_uint64),
        ("n_pinned", C.c_uint64),
    ]


ALIGN_BEGIN_ONLY = 1


class SelectOpts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("window", C.c_uint32), ("strata", C.c_uint32), ("reserved", C.c_uint32)]


class SelectStats(C.Structure):
    _fields_ = [
        ("ms_total", C.c_float),
        ("ms_order", C.c_float),
        ("ms_select", C.c_float),
        ("ms_host", C.c_float),
        ("n_in", C.c_uint64),
        ("n_loci", C.c_uint64),
        ("n_out", C.c_uint64),
        ("key_bits", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


SELECT_LOCI, SELECT_BEST = 1, 2
SELECT_ACROSS = 4   # pan-genome selections only, with SELECT_BEST
SELECT_STRANDS = 8  # with SELECT_BEST: the minimum is taken per read = pattern >> 1, over both strands of a stranded set
SELECT_WINDOW_K = 0xFFFFFFFF
CIGAR_INS, CIGAR_DEL, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8


E_OVERFLOW = -5  # SPM_E_OVERFLOW: the caller's buffer is too small, and the length it needs has been written

# (restype, argtypes) of every function that include/spm_hip.h declares: lib() binds these, EXPORTS names them
_vp, _u8p, _u32p, _u16p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint16)
SIGNATURES = {
    "spm_hip_init": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "spm_hip_destroy": (None, [_vp]),
    "spm_hip_last_error": (C.c_char_p, [_vp]),
    "spm_hip_synchronize": (C.c_int, [_vp]),
    "spm_hip_text_upload": (C.c_int, [_vp, _u8p, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_text_wrap": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_text_generate": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(_vp)]),
    "spm_hip_text_generate_repeats": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_text_pack": (C.c_int, [_vp, _vp]),
    "spm_hip_text_is_packed": (C.c_int, [_vp]),
    "spm_hip_text_download": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _u8p]),
    "spm_hip_text_length": (C.c_uint64, [_vp]),
    "spm_hip_text_device_ptr": (_vp, [_vp]),
    "spm_hip_text_destroy": (None, [_vp]),
    "spm_hip_patterns_create": (C.c_int, [_vp, C.c_int, _u8p, _u32p, C.c_uint32, _u16p, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_patterns_create_stranded": (C.c_int, [_vp, C.c_int, _u8p, _u32p, C.c_uint32, _u16p, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_patterns_strands": (C.c_uint32, [_vp]),
    "spm_hip_patterns_count": (C.c_uint32, [_vp]),
    "spm_hip_patterns_needle": (C.c_int, [_vp, C.c_uint32, _u8p, C.c_uint32, _u32p]),
    "spm_hip_patterns_destroy": (None, [_vp]),
    "spm_hip_patterns_window_size": (C.c_uint64, [_vp, C.c_uint32]),
    "spm_hip_patterns_filterable": (C.c_int, [_vp]),
    "spm_hip_patterns_build_stats": (C.c_int, [_vp, C.POINTER(BuildStats)]),
    "spm_hip_patterns_state_stride": (C.c_size_t, [_vp]),
    "spm_hip_patterns_state_init": (C.c_int, [_vp, _vp]),
    "spm_hip_scan": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _vp, C.POINTER(ScanOpts), _vp, _vp, C.POINTER(_vp)]),
    "spm_hip_scan_segments": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.c_uint64, _vp, C.POINTER(ScanOpts),
                                        C.POINTER(_vp)]),
    "spm_hip_hits_view": (C.c_int, [_vp, C.POINTER(C.POINTER(Hit)), C.POINTER(C.c_uint64)]),
    "spm_hip_hits_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_hits_copy_device": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_hits_copy_fused": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_hits_copy_fused_device": (C.c_int, [_vp, _vp, C.c_uint64]),
    "spm_hip_hits_stats": (C.c_int, [_vp, C.POINTER(ScanStats)]),
    "spm_hip_hits_checksum": (C.c_uint64, [_vp]),
    "spm_hip_hits_destroy": (None, [_vp]),
    "spm_hip_hits_align": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_alns_view": (C.c_int, [_vp, C.POINTER(C.POINTER(Aln)), C.POINTER(C.c_uint64), C.POINTER(_u32p),
                                    C.POINTER(C.c_uint64)]),
    "spm_hip_alns_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_alns_stats": (C.c_int, [_vp, C.POINTER(AlignStats)]),
    "spm_hip_alns_destroy": (None, [_vp]),
    "spm_hip_hits_select": (C.c_int, [_vp, C.POINTER(SelectOpts), C.POINTER(_vp)]),
    "spm_hip_records_select": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.POINTER(SelectOpts), C.POINTER(_vp)]),
    "spm_hip_hits_select_stats": (C.c_int, [_vp, C.POINTER(SelectStats)]),
    "spm_hip_synth_pattern": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.c_uint32, _u8p]),
    "spm_hip_synth_repeat_pattern": (C.c_uint64, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, _u8p]),
    "spm_hip_synth_repeat_text": (None, [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, _u8p]),
    "spm_hip_mix64": (C.c_uint64, [C.c_uint64]),
    "spm_hip_host_selftest": (C.c_int, [C.c_int, _u8p, _u32p, C.c_uint32, _u16p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "spm_hip_version": (C.c_char_p, []),
    "spm_hip_jst_create": (C.c_int, [_vp, _vp, C.POINTER(JstAllele), C.c_uint64, _u8p, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_destroy": (None, [_vp]),
    "spm_hip_jst_haplotype_length": (C.c_uint64, [_vp, C.c_uint32]),
    "spm_hip_jst_extract": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _u8p]),
    "spm_hip_jst_index": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spm_hip_jst_search": (C.c_int, [_vp, _vp, C.POINTER(ScanOpts), C.POINTER(_vp)]),
    "spm_hip_jst_stats": (C.c_int, [_vp, C.POINTER(JstStats)]),
    "spm_hip_jst_hits_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstHit)), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_hits_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_hits_copy_device": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_jst_hits_destroy": (None, [_vp]),
    "spm_hip_jst_hits_align": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_selection_align": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_alns_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstAln)), C.POINTER(C.c_uint64), C.POINTER(_u32p),
                                        C.POINTER(C.c_uint64)]),
    "spm_hip_jst_alns_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp),
                                          C.POINTER(C.c_uint64)]),
    "spm_hip_jst_alns_stats": (C.c_int, [_vp, C.POINTER(JstAlignStats)]),
    "spm_hip_jst_alns_destroy": (None, [_vp]),
    "spm_hip_jst_alns_project": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_ref_alns_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstRefAln)), C.POINTER(C.c_uint64), C.POINTER(_u32p),
                                            C.POINTER(C.c_uint64)]),
    "spm_hip_jst_ref_alns_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp),
                                              C.POINTER(C.c_uint64)]),
    "spm_hip_jst_ref_alns_stats": (C.c_int, [_vp, C.POINTER(JstProjectStats)]),
    "spm_hip_jst_ref_alns_destroy": (None, [_vp]),
    "spm_hip_jst_ref_alns_normalize": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_ref_alns_normalize_stats": (C.c_int, [_vp, C.POINTER(JstNormalizeStats)]),
    "spm_hip_jst_ref_alns_collapse": (C.c_int, [_vp, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_ref_loci_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstRefLocus)), C.POINTER(C.c_uint64), C.POINTER(_u32p),
                                            C.POINTER(C.c_uint64), C.POINTER(_u32p), C.POINTER(C.POINTER(C.c_int32)),
                                            C.POINTER(C.c_uint64)]),
    "spm_hip_jst_ref_loci_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp),
                                              C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_ref_loci_map": (C.c_int, [_vp, C.POINTER(_u32p), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_ref_loci_stats": (C.c_int, [_vp, C.POINTER(JstCollapseStats)]),
    "spm_hip_jst_ref_loci_destroy": (None, [_vp]),
    "spm_hip_jst_ref_loci_reads": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_jst_reads_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstRead)), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_reads_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_reads_stats": (C.c_int, [_vp, C.POINTER(JstReadsStats)]),
    "spm_hip_jst_reads_destroy": (None, [_vp]),
    "spm_hip_jst_ref_loci_pairs": (C.c_int, [_vp, _vp, C.POINTER(JstPairOpts), C.POINTER(_vp)]),
    "spm_hip_jst_pairs_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstPair)), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_pairs_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_pairs_stats": (C.c_int, [_vp, C.POINTER(JstPairsStats)]),
    "spm_hip_jst_pairs_destroy": (None, [_vp]),
    "spm_hip_jst_pairs_rescue": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(JstRescueOpts), C.POINTER(_vp)]),
    "spm_hip_jst_rescues_view": (C.c_int, [_vp, C.POINTER(C.POINTER(JstRescue)), C.POINTER(C.c_uint64), C.POINTER(_u32p),
                                           C.POINTER(C.c_uint64)]),
    "spm_hip_jst_rescues_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_jst_rescues_stats": (C.c_int, [_vp, C.POINTER(JstRescuesStats)]),
    "spm_hip_jst_rescues_destroy": (None, [_vp]),
    "spm_hip_jst_ref_loci_sam": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(SamOpts), C.POINTER(_vp)]),
    "spm_hip_sam_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(SamLine)),
                                   C.POINTER(C.c_uint64)]),
    "spm_hip_sam_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_sam_stats": (C.c_int, [_vp, C.POINTER(SamStats)]),
    "spm_hip_sam_destroy": (None, [_vp]),
    "spm_hip_sam_header": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_sam_mapq": (C.c_int, [C.POINTER(SamOpts), C.c_uint32, C.c_uint32]),
    "spm_hip_jst_ref_loci_bam": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(BamOpts), C.POINTER(_vp)]),
    "spm_hip_jst_ref_loci_sam_ex": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(SamOpts), C.POINTER(SamExtras), C.POINTER(_vp)]),
    "spm_hip_jst_ref_loci_bam_ex": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(BamOpts), C.POINTER(SamExtras), C.POINTER(_vp)]),
    "spm_hip_sam_md": (C.c_int, [_u32p, C.c_uint32, _u8p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64,
                                 C.POINTER(C.c_uint64)]),
    "spm_hip_bam_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64),
                                   C.POINTER(C.POINTER(SamLine)), C.POINTER(C.c_uint64)]),
    "spm_hip_bam_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp),
                                     C.POINTER(C.c_uint64)]),
    "spm_hip_bam_stats": (C.c_int, [_vp, C.POINTER(BamStats)]),
    "spm_hip_bam_destroy": (None, [_vp]),
    "spm_hip_bam_header": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_frame": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(BgzfOpts), C.POINTER(_vp)]),
    "spm_hip_bgzf_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_stats": (C.c_int, [_vp, C.POINTER(BgzfStats)]),
    "spm_hip_bgzf_destroy": (None, [_vp]),
    "spm_hip_bgzf_frame_host": (C.c_int, [_vp, C.c_uint64, C.POINTER(BgzfOpts), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_framed_size": (C.c_int, [C.c_uint64, C.POINTER(BgzfOpts), C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_deflate": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(BgzfDeflateOpts), C.POINTER(_vp)]),
    "spm_hip_bgzf_blocks": (C.c_int, [_vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_blocks_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_deflate_stats": (C.c_int, [_vp, C.POINTER(BgzfDeflateStats)]),
    "spm_hip_bgzf_block_types": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_deflate_host": (C.c_int, [_vp, C.c_uint64, C.POINTER(BgzfDeflateOpts), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_bgzf_deflate_bound": (C.c_int, [C.c_uint64, C.POINTER(BgzfDeflateOpts), C.POINTER(C.c_uint64)]),
    "spm_hip_bam_deflate": (C.c_int, [_vp, C.POINTER(BgzfDeflateOpts), C.POINTER(_vp)]),
    "spm_hip_bam_sort": (C.c_int, [_vp, C.POINTER(BamSortOpts), C.POINTER(_vp)]),
    "spm_hip_bam_sort_stats": (C.c_int, [_vp, C.POINTER(BamSortStats)]),
    "spm_hip_sam_header_sorted": (C.c_int, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_bam_header_sorted": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_bam_index": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "spm_hip_bai_build": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "spm_hip_bai_build_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64,
                                         C.POINTER(C.c_uint64)]),
    "spm_hip_bai_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_bai_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_bai_stats": (C.c_int, [_vp, C.POINTER(BaiStats)]),
    "spm_hip_bai_destroy": (None, [_vp]),
    "spm_hip_bam_markdup": (C.c_int, [_vp, C.POINTER(BamMarkdupOpts), C.POINTER(_vp)]),
    "spm_hip_bam_markdup_stats": (C.c_int, [_vp, C.POINTER(BamMarkdupStats)]),
    "spm_hip_bam_markdup_records": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint64, C.POINTER(BamMarkdupOpts), _vp,
                                              C.POINTER(BamMarkdupStats)]),
    "spm_hip_bam_markdup_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint64, C.POINTER(BamMarkdupOpts), _vp]),
    "spm_hip_bam_pileup": (C.c_int, [_vp, C.POINTER(PileupOpts), C.POINTER(_vp)]),
    "spm_hip_bam_pileup_records": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint64, C.POINTER(PileupOpts), C.POINTER(_vp)]),
    "spm_hip_bam_pileup_host": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint64, C.POINTER(PileupOpts), _vp]),
    "spm_hip_pileup_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_pileup_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_pileup_stats": (C.c_int, [_vp, C.POINTER(PileupStats)]),
    "spm_hip_pileup_destroy": (None, [_vp]),
    "spm_hip_pileup_sites": (C.c_int, [_vp, _vp, C.POINTER(PileupSiteOpts), C.POINTER(_vp)]),
    "spm_hip_pileup_sites_view": (C.c_int, [_vp, C.POINTER(C.POINTER(PileupSite)), C.POINTER(C.c_uint64)]),
    "spm_hip_pileup_sites_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_pileup_sites_destroy": (None, [_vp]),
    "spm_hip_pileup_sites_host": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _vp, C.c_uint64, C.POINTER(PileupSiteOpts), _vp, C.c_uint64,
                                            C.POINTER(C.c_uint64)]),
    "spm_hip_pileup_sites_vcf": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(VcfOpts), C.POINTER(_vp)]),
    "spm_hip_pileup_sites_vcf_records": (C.c_int, [_vp, _vp, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(VcfOpts),
                                                   C.POINTER(_vp)]),
    "spm_hip_vcf_view": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(VariantCall)), C.POINTER(C.c_uint64)]),
    "spm_hip_vcf_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "spm_hip_vcf_stats": (C.c_int, [_vp, C.POINTER(VcfStats)]),
    "spm_hip_vcf_destroy": (None, [_vp]),
    "spm_hip_pileup_sites_calls_host": (C.c_int, [_vp, C.c_uint64, C.POINTER(VcfOpts), _vp]),
    "spm_hip_pileup_sites_vcf_host": (C.c_int, [_vp, C.c_uint64, C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(VcfOpts), _vp, C.c_uint64,
                                                C.POINTER(C.c_uint64)]),
    "spm_hip_vcf_header": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "spm_hip_jst_hits_select": (C.c_int, [_vp, C.POINTER(SelectOpts), C.POINTER(_vp)]),
    "spm_hip_jst_records_select": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.POINTER(SelectOpts), C.POINTER(_vp)]),
    "spm_hip_jst_hits_select_stats": (C.c_int, [_vp, C.POINTER(SelectStats)]),
    "spm_hip_comm_unique_id": (C.c_int, [_vp]),
    "spm_hip_comm_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "spm_hip_comm_destroy": (None, [_vp]),
    "spm_hip_gatherv_hits": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "spm_hip_gatherv_jst_hits": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64)]),
    "spm_hip_gatherv_plan": (C.c_int, [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "spm_hip_comm_selftest": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_int)]),
    "spm_hip_jst_synth_variants": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                             C.POINTER(JstAllele), C.POINTER(C.c_uint64), _u8p,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}
EXPORTS = list(SIGNATURES)


def build(force: bool = False) -> str:
    """Compile libspm_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".cpp"))]
    srcs.append(os.path.join(_PKG, "..", "include", "spm_hip.h"))
    stale = not os.path.exists(SO_PATH) or any(os.path.getmtime(s) > os.path.getmtime(SO_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return SO_PATH


_lib = None


def lib():
    """Load the shared library; fail loudly when it is absent (there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise SpmError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). libspm_amd has no CPU fallback.")
    L = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L

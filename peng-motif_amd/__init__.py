"""peng_motif_amd -- ctypes plumbing over libpengk.so (include/pengk.h), the MI355X hot path of PEnG-motif.

The product is the C-ABI library (HIP kernels for gfx950) plus the C++ host mirror of the reference's
classes under peng-motif_amd/host/.  This module only exposes the C ABI to Python so that tests/ and
bench.py can drive it; device memory is either owned here (pengk_malloc) or borrowed from torch
tensors via data_ptr().  There is no CPU fallback: without the built library, or without a GPU,
the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PENGK_LIB: A/B timing of library variants in one session (tools/ab.sh); the product loads the in-tree build
LIB_PATH = os.environ.get("PENGK_LIB") or os.path.join(_HERE, "libpengk.so")
_lib = None

PENGK_OK = 0
ERR_ARG, ERR_DEVICE, ERR_RANGE, ERR_UNSUPPORTED, ERR_NOMEM = 1, 2, 3, 4, 5
FRONT_PAD_BASES = 64

EXPORTS = [
    "pengk_version", "pengk_last_error", "pengk_error_name", "pengk_create", "pengk_destroy", "pengk_synchronize",
    "pengk_stream", "pengk_set_stream", "pengk_set_option", "pengk_get_info", "pengk_malloc", "pengk_free", "pengk_memcpy_h2d", "pengk_memcpy_d2h",
    "pengk_memset", "pengk_warmup", "pengk_host_alloc", "pengk_host_free", "pengk_timer_create", "pengk_timer_record", "pengk_timer_elapsed_ms", "pengk_timer_destroy",
    "pengk_pack", "pengk_pack_threads", "pengk_pack_append", "pengk_packed_free", "pengk_set_sequences", "pengk_synth_sizes", "pengk_synth_sequences",
    "pengk_count", "pengk_count_bg", "pengk_mirror_counts", "pengk_bg_count", "pengk_bg_model", "pengk_pattern_stats", "pengk_pattern_stats_control",
    "pengk_strata_bg_count", "pengk_pattern_stats_strata",
    "pengk_bg_count_order", "pengk_bg_model_order", "pengk_pattern_stats_order",
    "pengk_seed_candidates", "pengk_iupac_aggregate", "pengk_em", "pengk_em_device", "pengk_test_em_generation", "pengk_sequential_sum_f32", "pengk_motif_similarity", "pengk_selftest_division",
    "pengk_comm_unique_id", "pengk_comm_init", "pengk_comm_init_env", "pengk_comm_info", "pengk_comm_init_abandoned", "pengk_comm_rccl_version", "pengk_comm_destroy",
    "pengk_allreduce_tables", "pengk_comm_check_bin_bound", "pengk_allgather",
    "pengk_comm_host_init_env", "pengk_comm_host_info", "pengk_comm_host_allgather", "pengk_comm_host_allreduce_u64",
    "pengk_comm_host_shutdown",
    "pengk_scan_layout_words", "pengk_scan_layout_build", "pengk_synth_scan_sequences", "pengk_sample_background",
    "pengk_shuffle_sequences",
    "pengk_motif_scan", "pengk_score_histograms", "pengk_score_summary",
    "pengk_score_tail_pvalues", "pengk_score_threshold", "pengk_sites_count", "pengk_sites_slices", "pengk_sites_emit",
    "pengk_sites_histograms", "pengk_sites_qvalues", "pengk_qvalue_threshold",
    "pengk_mask_sites", "pengk_pack_scan_sizes", "pengk_pack_scan", "pengk_mask_low_complexity",
    "pengk_seq_strata", "pengk_match_quotas", "pengk_select_strata", "pengk_split_sequences", "pengk_holdout_summary",
    "pengk_motif_enrich", "pengk_hypergeom_log10_sf", "pengk_enrich_summary",
    "pengk_motif_best_sites", "pengk_centrality_histograms", "pengk_centrality_summary", "pengk_binomial_log10_sf",
    "pengk_dyad_count", "pengk_dyad_summary",
    "pengk_position_count", "pengk_position_summary", "pengk_position_pairs", "pengk_position_summary_null",
    "pengk_site_profiles", "pengk_profile_refine",
    "pengk_site_pair_profiles", "pengk_dinuc_model", "pengk_motif_scan_dinuc",
    "pengk_spacing_histograms", "pengk_spacing_summary",
    "pengk_compare_quantize", "pengk_compare_nulls", "pengk_compare_motifs", "pengk_compare_summary", "pengk_test_compare_tails",
]
MAX_MOTIF_LEN = 64
SCORE_SENTINEL = -2 ** 31
SITES_BLOCK = 4096
SITE = np.dtype([("seq", np.uint32), ("pos", np.uint32), ("score", np.int32), ("motif_strand", np.uint32)])
CENTRALITY_MAX_LEN = 65536
DYAD_MAX_GAP = 26
POSITION_MIN_K, POSITION_MAX_K = 4, 7
POSITION_MAX_BINS = 64
POSITION_MAX_BIN_SIZE = 65536
POSITION_ANCHORS = ("start", "end", "center")
SPACING_MAX_MOTIFS = 64
SPACING_MAX_GAP = 1024
COMPARE_BINS = 257
SPACING_CLASSES = ("same_downstream", "same_upstream", "opposite_downstream", "opposite_upstream")


class CentralityStruct(C.Structure):
    _fields_ = [("sites", C.c_uint64), ("max_offset", C.c_uint32), ("window", C.c_uint32), ("in_window", C.c_uint64),
                ("expected", C.c_double), ("log10_pvalue", C.c_double), ("log10_evalue", C.c_double)]


class DyadStruct(C.Structure):
    _fields_ = [("gap", C.c_uint32), ("key", C.c_uint32), ("count", C.c_uint64), ("positions", C.c_uint64), ("p", C.c_double),
                ("expected", C.c_double), ("log10_pvalue", C.c_double), ("log10_evalue", C.c_double),
                ("other_gaps_mean", C.c_double), ("family", C.c_uint32), ("is_head", C.c_uint32)]


class PositionWordStruct(C.Structure):
    _fields_ = [("key", C.c_uint32), ("bin", C.c_uint32), ("count", C.c_uint64), ("total", C.c_uint64),
                ("bin_positions", C.c_uint64), ("expected", C.c_double), ("log10_pvalue", C.c_double),
                ("log10_evalue", C.c_double), ("bins_significant", C.c_uint32), ("family", C.c_uint32), ("is_head", C.c_uint32)]


class EnrichmentStruct(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("n_thresholds", C.c_uint32), ("pos_hits", C.c_uint64), ("neg_hits", C.c_uint64),
                ("enrichment", C.c_double), ("log10_pvalue", C.c_double), ("log10_adj_pvalue", C.c_double)]


class HoldoutStruct(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("n_thresholds", C.c_uint32), ("train_pos_hits", C.c_uint64),
                ("train_neg_hits", C.c_uint64), ("train_log10_adj_pvalue", C.c_double), ("hold_pos_hits", C.c_uint64),
                ("hold_neg_hits", C.c_uint64), ("hold_log10_pvalue", C.c_double), ("hold_enrichment", C.c_double)]


class SpacingStruct(C.Structure):
    _fields_ = [("both", C.c_uint64), ("overlapping", C.c_uint64), ("apart", C.c_uint64), ("far", C.c_uint64),
                ("expected_both", C.c_double), ("log10_pvalue_both", C.c_double), ("orientation", C.c_uint32),
                ("gap", C.c_uint32), ("count", C.c_uint64), ("expected", C.c_double), ("log10_pvalue", C.c_double),
                ("log10_evalue", C.c_double), ("tested_gaps", C.c_uint32)]


class PengkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (lib().pengk_error_name(code).decode(), msg))
        self.code = code


class PackedStruct(C.Structure):
    _fields_ = [("words", C.POINTER(C.c_uint64)), ("n_words", C.c_uint64), ("items", C.POINTER(C.c_uint64)),
                ("n_items", C.c_uint64), ("n_bases", C.c_uint64), ("n_windows", C.c_uint64), ("max_bin_bound", C.c_uint64),
                ("bg_counts", C.c_int64 * 84), ("n_sequences", C.c_uint64), ("max_len", C.c_uint64), ("W", C.c_int),
                ("item_windows", C.c_int), ("all_whole", C.c_int)]


IUPAC_STATS = np.dtype([("sites", np.uint64), ("bg_p", np.float32), ("expected", np.float32), ("zscore", np.float32),
                        ("log_pvalue", np.float32)], align=True)


def lib():
    """Load libpengk.so (built in-tree by peng-motif_amd/build.py).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libpengk.so is not built: run `python peng-motif_amd/build.py` (needs hipcc)")
        L = C.CDLL(LIB_PATH)
        vp, u64, i64, f32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_float
        L.pengk_version.restype = C.c_int
        L.pengk_last_error.restype = C.c_char_p
        L.pengk_error_name.restype = C.c_char_p
        L.pengk_error_name.argtypes = [C.c_int]
        L.pengk_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.pengk_destroy.argtypes = [vp]
        L.pengk_synchronize.argtypes = [vp]
        L.pengk_stream.restype = vp
        L.pengk_stream.argtypes = [vp]
        L.pengk_set_stream.argtypes = [vp, vp]
        L.pengk_set_option.argtypes = [vp, C.c_char_p, i64]
        L.pengk_get_info.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        L.pengk_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.pengk_free.argtypes = [vp, vp]
        L.pengk_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
        L.pengk_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
        L.pengk_memset.argtypes = [vp, vp, C.c_int, C.c_size_t]
        L.pengk_warmup.argtypes = [vp]
        L.pengk_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.pengk_host_free.argtypes = [vp, vp]
        L.pengk_timer_create.argtypes = [vp, C.POINTER(vp)]
        L.pengk_timer_record.argtypes = [vp, vp]
        L.pengk_timer_elapsed_ms.argtypes = [vp, vp, vp, C.POINTER(f32)]
        L.pengk_timer_destroy.argtypes = [vp, vp]
        L.pengk_pack.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.POINTER(PackedStruct)]
        L.pengk_pack_threads.argtypes = [vp, vp, i64, C.c_int, C.c_int, C.c_int, C.POINTER(PackedStruct)]
        L.pengk_pack_append.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, C.POINTER(PackedStruct)]
        L.pengk_packed_free.restype = None
        L.pengk_packed_free.argtypes = [C.POINTER(PackedStruct)]
        L.pengk_set_sequences.argtypes = [vp, vp, u64, vp, u64, C.c_int, C.c_int, u64, C.c_int]
        L.pengk_synth_sizes.argtypes = [u64, C.c_uint32, C.c_int, C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.pengk_synth_sequences.argtypes = [vp, u64, u64, u64, C.c_uint32, C.c_int, C.c_int, vp, vp]
        L.pengk_count.argtypes = [vp, C.c_int, vp, vp]
        L.pengk_count_bg.argtypes = [vp, C.c_int, vp, vp, vp]
        L.pengk_mirror_counts.argtypes = [vp, C.c_int, vp]
        L.pengk_bg_count.argtypes = [vp, vp]
        L.pengk_bg_model.argtypes = [vp, vp, C.c_int, vp, vp]
        L.pengk_pattern_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.pengk_pattern_stats_control.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp]
        L.pengk_strata_bg_count.argtypes = [vp, vp, vp, vp, vp, u64, vp, C.c_int, C.c_int, vp, vp]
        L.pengk_pattern_stats_strata.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp]
        L.pengk_bg_count_order.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp]
        L.pengk_bg_model_order.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        L.pengk_pattern_stats_order.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.c_double, vp, vp, vp, vp]
        L.pengk_seed_candidates.argtypes = [vp, C.c_int, vp, vp, f32, u64, vp, vp, i64, C.POINTER(i64)]
        L.pengk_iupac_aggregate.argtypes = [vp, C.c_int, C.c_int, vp, i64, vp, vp, vp, vp]
        L.pengk_em.argtypes = [vp, C.c_int, i64, vp, f32, f32, C.c_int, vp, vp, vp, vp]
        L.pengk_em_device.argtypes = [vp, C.c_int, i64, vp, f32, f32, C.c_int, vp, vp, vp, vp]
        L.pengk_test_em_generation.argtypes = [vp, C.c_int]
        L.pengk_sequential_sum_f32.argtypes = [vp, vp, u64, u64, vp]
        L.pengk_selftest_division.argtypes = [vp, u64, C.c_uint32, vp]
        L.pengk_motif_similarity.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp]
        L.pengk_comm_unique_id.argtypes = [vp]
        L.pengk_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
        L.pengk_comm_init_env.argtypes = [vp]
        L.pengk_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.pengk_comm_destroy.argtypes = [vp]
        L.pengk_allreduce_tables.argtypes = [vp, C.c_int, vp, vp, vp]
        L.pengk_comm_check_bin_bound.argtypes = [vp]
        L.pengk_allgather.argtypes = [vp, vp, vp, C.c_size_t]
        L.pengk_comm_host_init_env.argtypes = []
        L.pengk_comm_host_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.pengk_comm_host_allgather.argtypes = [vp, vp, C.c_size_t]
        L.pengk_comm_host_allreduce_u64.argtypes = [vp, C.c_size_t]
        L.pengk_comm_host_shutdown.argtypes = []
        L.pengk_scan_layout_words.argtypes = [vp, i64, C.POINTER(u64)]
        L.pengk_scan_layout_build.argtypes = [vp, vp, i64, u64, vp, vp, vp, vp]
        L.pengk_synth_scan_sequences.argtypes = [vp, u64, u64, u64, C.c_uint32, vp, vp, vp, vp]
        L.pengk_sample_background.argtypes = [vp, u64, u64, u64, vp, vp, C.c_int, vp, vp]
        L.pengk_shuffle_sequences.argtypes = [vp, u64, u64, u64, vp, vp, vp, vp, vp, vp]
        L.pengk_motif_scan.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp]
        L.pengk_score_histograms.argtypes = [vp, C.c_int, vp, u64, vp, vp, vp, vp]
        L.pengk_score_summary.argtypes = [vp, vp, u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.pengk_score_tail_pvalues.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
        L.pengk_score_threshold.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_int32)]
        L.pengk_sites_count.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp, vp]
        L.pengk_sites_histograms.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.pengk_sites_qvalues.argtypes = [vp, u64, u64, vp, vp]
        L.pengk_mask_sites.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
        L.pengk_mask_low_complexity.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp]
        L.pengk_pack_scan_sizes.argtypes = [vp, vp, vp, vp, u64, C.c_int, C.c_int, vp, vp, C.POINTER(PackedStruct)]
        L.pengk_pack_scan.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, vp, vp, vp, u64, vp, u64]
        L.pengk_seq_strata.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, vp, vp]
        L.pengk_match_quotas.argtypes = [vp, vp, u64, vp, C.POINTER(u64)]
        L.pengk_select_strata.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]
        L.pengk_motif_enrich.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        L.pengk_hypergeom_log10_sf.argtypes = [u64, u64, u64, u64, C.POINTER(C.c_double)]
        L.pengk_enrich_summary.argtypes = [vp, vp, u64, C.c_int32, u64, u64, C.POINTER(EnrichmentStruct)]
        L.pengk_split_sequences.argtypes = [vp, u64, u64, u64, u64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp, vp, vp,
                                            C.POINTER(u64)]
        L.pengk_holdout_summary.argtypes = [vp, vp, vp, vp, u64, C.c_int32, u64, u64, u64, u64, C.POINTER(HoldoutStruct)]
        L.pengk_qvalue_threshold.argtypes = [vp, u64, C.c_int32, C.c_double, C.POINTER(C.c_int32)]
        L.pengk_sites_slices.argtypes = [vp, vp, u64, C.c_int, vp, u64, vp, vp, C.POINTER(u64)]
        L.pengk_sites_emit.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, C.c_int, vp, vp, u64, u64, vp, u64]
        L.pengk_motif_best_sites.argtypes = [vp, vp, vp, vp, vp, u64, u64, C.c_int, vp, vp, C.c_int, vp, vp]
        L.pengk_centrality_histograms.argtypes = [vp, C.c_int, vp, vp, vp, u64, vp, vp, C.c_uint32, vp, vp]
        L.pengk_centrality_summary.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, C.POINTER(CentralityStruct)]
        L.pengk_binomial_log10_sf.argtypes = [u64, u64, C.c_double, C.POINTER(C.c_double)]
        L.pengk_dyad_count.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, vp, vp]
        L.pengk_dyad_summary.argtypes = [vp, vp, C.c_int, C.c_int, u64, C.c_double, vp, u64, C.POINTER(u64)]
        L.pengk_position_count.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.pengk_position_summary.argtypes = [vp, C.c_int, C.c_int, C.c_int, u64, C.c_double, vp, u64, C.POINTER(u64)]
        L.pengk_position_pairs.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.pengk_position_summary_null.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, u64, C.c_double, vp, u64, C.POINTER(u64)]
        L.pengk_site_profiles.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, vp, C.c_int, vp]
        L.pengk_profile_refine.argtypes = [vp, C.c_int, C.c_int, vp, C.c_double, vp, vp, vp, C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(u64)]
        L.pengk_site_pair_profiles.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, vp, C.c_int, vp]
        L.pengk_dinuc_model.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(u64)]
        L.pengk_motif_scan_dinuc.argtypes = [vp, vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, C.c_int, vp]
        L.pengk_spacing_histograms.argtypes = [vp, C.c_int, vp, vp, vp, u64, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.pengk_spacing_summary.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, u64, u64, u64, C.c_int,
                                            C.POINTER(SpacingStruct)]
        L.pengk_compare_quantize.argtypes = [vp, C.c_int, vp]
        L.pengk_compare_nulls.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp]
        L.pengk_compare_motifs.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]
        L.pengk_compare_summary.argtypes = [vp, vp, C.c_int, vp, vp, vp]
        L.pengk_test_compare_tails.argtypes = [vp, C.c_int, vp, vp]
        _lib = L
    return _lib


def _check(rc):
    if rc != PENGK_OK:
        raise PengkError(rc, lib().pengk_last_error().decode())


class Packed:
    """Host result of pengk_pack: numpy copies of the 2-bit stream and the scan items."""

    def __init__(self, codes, offs, W, item_windows=0):
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        st = PackedStruct()
        _check(lib().pengk_pack(codes.ctypes.data, offs.ctypes.data, len(offs) - 1, W, item_windows, C.byref(st)))
        try:
            self.words = np.ctypeslib.as_array(st.words, shape=(st.n_words,)).copy()
            self.items = np.ctypeslib.as_array(st.items, shape=(max(st.n_items, 1),)).copy()[:st.n_items]
            self.n_bases = int(st.n_bases)
            self.n_windows = int(st.n_windows)
            self.max_bin_bound = int(st.max_bin_bound)
            self.bg_counts = np.array(list(st.bg_counts), np.int64)
            self.n_sequences = int(st.n_sequences)
            self.max_len = int(st.max_len)
            self.W = int(st.W)
            self.item_windows = int(st.item_windows)
            self.all_whole = int(st.all_whole)
        finally:
            lib().pengk_packed_free(C.byref(st))


class ScanLayout:
    """Host result of pengk_scan_layout_build: the scan layout of the motif scoring (include/pengk.h)."""

    def __init__(self, codes, offs):
        codes = np.ascontiguousarray(codes, np.uint8)
        offs = np.ascontiguousarray(offs, np.int64)
        n = len(offs) - 1
        nw = C.c_uint64()
        _check(lib().pengk_scan_layout_words(offs.ctypes.data, n, C.byref(nw)))
        self.n_seq = n
        self.words = np.zeros(max(nw.value, 1), np.uint64)
        self.valid = np.zeros(max(nw.value, 1), np.uint32)
        self.offs = np.zeros(max(n, 1), np.int64)
        self.lens = np.zeros(max(n, 1), np.uint32)
        _check(lib().pengk_scan_layout_build(codes.ctypes.data, offs.ctypes.data, n, 0, self.words.ctypes.data,
                                             self.valid.ctypes.data, self.offs.ctypes.data, self.lens.ctypes.data))


def score_summary(pos_hist, neg_hist):
    """(zoops_score, occur) of one motif from its input / background histograms (pengk_score_summary, CPU)."""
    p = np.ascontiguousarray(pos_hist, np.uint64)
    n = np.ascontiguousarray(neg_hist, np.uint64)
    assert p.shape == n.shape
    z, o = C.c_double(), C.c_double()
    _check(lib().pengk_score_summary(p.ctypes.data, n.ctypes.data, len(p), C.byref(z), C.byref(o)))
    return z.value, o.value


def score_tail_pvalues(S, bg):
    """(lo, tail): tail[t - lo] = P(score >= t) of one window strand of S (w x 4 int32) under bg (pengk_score_tail_pvalues, CPU)"""
    S = np.ascontiguousarray(S, np.int32)
    bg = np.ascontiguousarray(bg, np.float32)
    lo, hi = C.c_int32(), C.c_int32()
    _check(lib().pengk_score_tail_pvalues(S.ctypes.data, S.shape[0], bg.ctypes.data, C.byref(lo), C.byref(hi), None))
    tail = np.zeros(hi.value - lo.value + 1, np.float64)
    _check(lib().pengk_score_tail_pvalues(S.ctypes.data, S.shape[0], bg.ctypes.data, C.byref(lo), C.byref(hi), tail.ctypes.data))
    return lo.value, tail


def score_threshold(tail, lo, p):
    """the smallest t with tail[t - lo] <= p, else lo + len(tail) (pengk_score_threshold, CPU)"""
    tail = np.ascontiguousarray(tail, np.float64)
    t = C.c_int32()
    _check(lib().pengk_score_threshold(tail.ctypes.data, lo, lo + len(tail) - 1, p, C.byref(t)))
    return t.value


def sites_qvalues(hist, n_tests, tail_from_thr):
    """q[k] of the sites with score t + k from one motif's site histogram (summed over all ranks), its number of scored
    window strands and tail[t - lo:] of score_tail_pvalues (pengk_sites_qvalues, CPU)"""
    h = np.ascontiguousarray(hist, np.uint64)
    tail = np.ascontiguousarray(tail_from_thr, np.float64)
    assert len(tail) >= len(h)
    q = np.zeros(len(h), np.float64)
    _check(lib().pengk_sites_qvalues(h.ctypes.data, len(h), int(n_tests), tail.ctypes.data, q.ctypes.data))
    return q


def qvalue_threshold(q, t, q_max):
    """the smallest score t + k with q[k] <= q_max, else t + len(q) (pengk_qvalue_threshold, CPU)"""
    q = np.ascontiguousarray(q, np.float64)
    out = C.c_int32()
    _check(lib().pengk_qvalue_threshold(q.ctypes.data, len(q), t, q_max, C.byref(out)))
    return out.value


def centrality_summary(hist_offsets, hist_lengths, max_len, w, n_motifs):
    """one motif's central-enrichment test from its two histograms (pengk_centrality_summary, CPU): a dict with sites,
    max_offset, window, in_window, expected, log10_pvalue, log10_evalue"""
    hd = np.ascontiguousarray(hist_offsets, np.uint64)
    hl = np.ascontiguousarray(hist_lengths, np.uint64)
    assert len(hd) == 2 * max_len + 1 and len(hl) == max_len + 1
    out = CentralityStruct()
    _check(lib().pengk_centrality_summary(hd.ctypes.data, hl.ctypes.data, max_len, w, n_motifs, C.byref(out)))
    return {k: getattr(out, k) for k, _ in CentralityStruct._fields_}


def binomial_log10_sf(n, k, p):
    """log10 P(X >= k) for X ~ Binomial(n, p) (pengk_binomial_log10_sf, CPU)"""
    out = C.c_double()
    _check(lib().pengk_binomial_log10_sf(int(n), int(k), float(p), C.byref(out)))
    return out.value


def dyad_summary(counts, mono, both, min_count=5, max_evalue=0.01, capacity=None):
    """the --dyads report from the summed tables of Context.dyad_count (pengk_dyad_summary, CPU): a list of dicts with
    gap, key, count, positions, p, expected, log10_pvalue, log10_evalue, other_gaps_mean, family, is_head, in report
    order.  capacity: the lines the first call has room for (a test hook: the call is repeated when there are more)."""
    c = np.ascontiguousarray(counts, np.uint64)
    m = np.ascontiguousarray(mono, np.uint64)
    assert c.ndim == 2 and c.shape[1] == 4096 and m.shape == (64,)
    n = C.c_uint64()
    cap = 256 if capacity is None else int(capacity)
    while True:
        out = (DyadStruct * max(cap, 1))()
        _check(lib().pengk_dyad_summary(c.ctypes.data, m.ctypes.data, c.shape[0] - 1, int(both), int(min_count), float(max_evalue),
                                        C.addressof(out), cap, C.byref(n)))
        if n.value <= cap:
            break
        cap = n.value
    return [{k: getattr(out[i], k) for k, _ in DyadStruct._fields_} for i in range(n.value)]


def position_summary(counts, K, both, min_count=5, max_evalue=0.01, capacity=None, pairs=None):
    """the --positional report from the summed table of Context.position_count (pengk_position_summary, CPU): a list of
    dicts with key, bin, count, total, bin_positions, expected, log10_pvalue, log10_evalue, bins_significant, family,
    is_head, in report order.  capacity: the lines the first call has room for (a test hook: the call is repeated when
    there are more).  pairs: the summed n_bins x 16 table of Context.position_pairs -- the composition null
    (pengk_position_summary_null) instead of the flat one."""
    c = np.ascontiguousarray(counts, np.uint64)
    assert c.ndim == 2
    if POSITION_MIN_K <= int(K) <= POSITION_MAX_K:
        assert c.shape[1] == 4 ** int(K)
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, np.uint64)
        assert pairs.shape == (c.shape[0], 16)
    n = C.c_uint64()
    cap = 256 if capacity is None else int(capacity)
    while True:
        out = (PositionWordStruct * max(cap, 1))()
        _check(lib().pengk_position_summary_null(c.ctypes.data, None if pairs is None else pairs.ctypes.data, int(K), c.shape[0], int(both),
                                                 int(min_count), float(max_evalue), C.addressof(out), cap, C.byref(n)))
        if n.value <= cap:
            break
        cap = n.value
    return [{k: getattr(out[i], k) for k, _ in PositionWordStruct._fields_} for i in range(n.value)]


def hypergeom_log10_sf(N, K, n, k):
    """log10 P(X >= k) for X ~ Hypergeometric(N, K marked, n drawn) (pengk_hypergeom_log10_sf, CPU)"""
    out = C.c_double()
    _check(lib().pengk_hypergeom_log10_sf(int(N), int(K), int(n), int(k), C.byref(out)))
    return out.value


def order_table_size(K):
    """entries of the tables of orders 0 .. K, back to back: (4^(K+2) - 4) / 3"""
    return (4 ** (K + 2) - 4) // 3


def bg_model_order(counts, K, alpha, interpolate=True):
    """float32 V of orders 0 .. K from their uint64 counters (pengk_bg_model_order, host only); alpha: K + 1 floats"""
    n = np.ascontiguousarray(counts, np.uint64)
    a = np.ascontiguousarray(alpha, np.float32)
    assert not 0 <= K <= 5 or (len(n) >= order_table_size(K) and len(a) >= K + 1)
    V = np.zeros(order_table_size(max(0, min(int(K), 5))), np.float32)
    _check(lib().pengk_bg_model_order(n.ctypes.data, int(K), a.ctypes.data, int(bool(interpolate)), V.ctypes.data))
    return V


def match_quotas(h_in, h_ctrl, ratio=1):
    """(quota, shortfall): how many control sequences of every stratum to keep for `ratio` per input sequence, from the
    two stratum histograms of Context.seq_strata (256 uint64 each), and what the control could not supply
    (pengk_match_quotas, CPU)"""
    a = np.ascontiguousarray(h_in, np.uint64)
    b = np.ascontiguousarray(h_ctrl, np.uint64)
    assert a.shape == b.shape == (256,)
    q = np.zeros(256, np.uint64)
    short = C.c_uint64()
    _check(lib().pengk_match_quotas(a.ctypes.data, b.ctypes.data, int(ratio), q.ctypes.data, C.byref(short)))
    return q, int(short.value)


def enrich_summary(pos_hist, neg_hist, thr, n_pos, n_neg):
    """one database motif's enrichment test from its input / negative histograms of Context.motif_enrich (bin k = score
    thr + k) and the scored sequences of either set (pengk_enrich_summary, CPU): a dict with the fields of pengk_enrichment"""
    p = np.ascontiguousarray(pos_hist, np.uint64)
    n = np.ascontiguousarray(neg_hist, np.uint64)
    assert p.shape == n.shape
    out = EnrichmentStruct()
    _check(lib().pengk_enrich_summary(p.ctypes.data if len(p) else None, n.ctypes.data if len(n) else None, len(p), int(thr),
                                      int(n_pos), int(n_neg), C.byref(out)))
    return {k: getattr(out, k) for k, _ in EnrichmentStruct._fields_}


def holdout_summary(train_pos, train_neg, hold_pos, hold_neg, thr, n_train_pos, n_train_neg, n_hold_pos, n_hold_neg):
    """one found motif's test on the hold-out share from its four histograms of Context.motif_enrich (bin k = score thr + k)
    and the scored sequences of the four sets (pengk_holdout_summary, CPU): a dict with the fields of pengk_holdout"""
    h = [np.ascontiguousarray(x, np.uint64) for x in (train_pos, train_neg, hold_pos, hold_neg)]
    assert h[0].shape == h[1].shape == h[2].shape == h[3].shape
    out = HoldoutStruct()
    _check(lib().pengk_holdout_summary(*[x.ctypes.data if len(x) else None for x in h], len(h[0]), int(thr), int(n_train_pos),
                                       int(n_train_neg), int(n_hold_pos), int(n_hold_neg), C.byref(out)))
    return {k: getattr(out, k) for k, _ in HoldoutStruct._fields_}


def spacing_summary(hist_gaps, hist_lengths, max_gap, max_len, w_a, w_b, n_classes, n, n_a, n_b, n_pairs):
    """one motif pair's co-occurrence and gap test from its two histograms (pengk_spacing_summary, CPU): a dict with the
    fields of pengk_spacing"""
    hg = np.ascontiguousarray(hist_gaps, np.uint64)
    hl = np.ascontiguousarray(hist_lengths, np.uint64)
    assert len(hg) == 4 * (max_gap + 1) + 2 and len(hl) == max_len + 1
    out = SpacingStruct()
    _check(lib().pengk_spacing_summary(hg.ctypes.data, hl.ctypes.data, max_gap, max_len, w_a, w_b, n_classes, int(n), int(n_a),
                                       int(n_b), n_pairs, C.byref(out)))
    return {k: getattr(out, k) for k, _ in SpacingStruct._fields_}


def clamp_flank(w, flank):
    """the flank a motif of width w gets: w + 2F <= MAX_MOTIF_LEN (pengk_site_profiles, pengk_profile_refine)"""
    return min(int(flank), (MAX_MOTIF_LEN - int(w)) // 2)


def profile_refine(counts, w, flank, bg, min_ic):
    """one motif's new matrix from its site-profile counts (pengk_profile_refine, CPU); counts: at least (w + 2F) x 5
    uint64 rows.  A dict: q (w + 2F x 4 double), ic, first, last (the kept columns [first, last)), pwm (the kept columns
    as float32) and sites"""
    F = clamp_flank(w, flank)
    n = w + 2 * F
    k = np.ascontiguousarray(np.asarray(counts, np.uint64).reshape(-1, 5)[:n])
    assert len(k) == n
    b = np.ascontiguousarray(bg, np.float32)
    q, ic = np.zeros((n, 4), np.float64), np.zeros(n, np.float64)
    pwm = np.zeros((MAX_MOTIF_LEN, 4), np.float32)
    first, last, sites = C.c_int32(), C.c_int32(), C.c_uint64()
    _check(lib().pengk_profile_refine(k.ctypes.data, w, int(flank), b.ctypes.data, float(min_ic), q.ctypes.data, ic.ctypes.data,
                                      pwm.ctypes.data, C.byref(first), C.byref(last), C.byref(sites)))
    return {"q": q, "ic": ic, "first": first.value, "last": last.value, "pwm": pwm[:last.value - first.value].copy(),
            "sites": sites.value}


def dinuc_model(counts1, counts2, w, flank, bg0, bg1, alpha):
    """one motif's first-order model from its single and pair counts (pengk_dinuc_model, CPU); counts1: at least W x 5,
    counts2: at least W x 17 uint64 rows, W = w + 2F.  A dict: q0 (W x 4 double), q1 (W x 16), mi (W), S0 (4 int32), D1 and
    D0 (W x 16 int32, row 0 zero), sites and flank (the clamped F)"""
    F = clamp_flank(w, flank)
    n = w + 2 * F
    k1 = np.ascontiguousarray(np.asarray(counts1, np.uint64).reshape(-1, 5)[:n])
    k2 = np.ascontiguousarray(np.asarray(counts2, np.uint64).reshape(-1, 17)[:n])
    assert len(k1) == n and len(k2) == n
    g0 = np.ascontiguousarray(bg0, np.float32)
    g1 = np.ascontiguousarray(bg1, np.float32).reshape(-1)
    assert len(g0) == 4 and len(g1) == 16
    q0, q1, mi = np.zeros((n, 4), np.float64), np.zeros((n, 16), np.float64), np.zeros(n, np.float64)
    S0, D1, D0 = np.zeros(4, np.int32), np.zeros((n, 16), np.int32), np.zeros((n, 16), np.int32)
    sites = C.c_uint64()
    _check(lib().pengk_dinuc_model(k1.ctypes.data, k2.ctypes.data, w, int(flank), g0.ctypes.data, g1.ctypes.data, float(alpha),
                                   q0.ctypes.data, q1.ctypes.data, mi.ctypes.data, S0.ctypes.data, D1.ctypes.data,
                                   D0.ctypes.data, C.byref(sites)))
    return {"q0": q0, "q1": q1, "mi": mi, "S0": S0, "D1": D1, "D0": D0, "sites": sites.value, "flank": F}


def compare_quantize(rows):
    """the quantised columns (w x 4 int16 in [0, 4096]) of a motif's rows (w x 4, any positive scale;
    pengk_compare_quantize, CPU)"""
    r = np.ascontiguousarray(rows, np.float64).reshape(-1, 4)
    X = np.zeros((len(r), 4), np.int16)
    _check(lib().pengk_compare_quantize(r.ctypes.data, len(r), X.ctypes.data))
    return X


def compare_tails_before(n):
    """the doubles of tail(i0, 1) .. tail(i0, n - 1): sum over n' < n of 256 n' + 1"""
    return 128 * (n - 1) * n + (n - 1)


def compare_summary(p_offset, n_offsets):
    """(p_match, evalue, qvalue) of one query's targets from their p_offset and n_offsets (pengk_compare_summary, CPU)"""
    p = np.ascontiguousarray(p_offset, np.float64)
    n = np.ascontiguousarray(n_offsets, np.int32)
    assert p.shape == n.shape
    pm, ev, q = (np.zeros(len(p), np.float64) for _ in range(3))
    _check(lib().pengk_compare_summary(p.ctypes.data, n.ctypes.data, len(p), pm.ctypes.data, ev.ctypes.data, q.ctypes.data))
    return pm, ev, q


def _pad_columns(motifs, lens=None):
    """a list of (w x 4) integer motifs as (n x MAX_MOTIF_LEN x 4 int16, widths); lens: widths to pass instead of the
    arrays' own (the argument checks)"""
    n = len(motifs)
    X = np.zeros((max(n, 1), MAX_MOTIF_LEN, 4), np.int16)
    ln = np.zeros(max(n, 1), np.int32)
    for m in range(n):
        x = np.asarray(motifs[m]).reshape(-1, 4)
        ln[m] = len(x)
        X[m, :min(len(x), MAX_MOTIF_LEN)] = x[:MAX_MOTIF_LEN]
    if lens is not None:
        ln[:n] = lens
    return X, ln


def _pad_motifs(S, lens):
    n = len(lens)
    Sp = np.zeros((max(n, 1), MAX_MOTIF_LEN, 4), np.int32)
    for m in range(n):
        Sp[m, :lens[m]] = np.asarray(S[m], np.int32)[:lens[m]]
    return Sp, np.ascontiguousarray(lens, np.int32)


class DeviceArray:
    """Device buffer owned through pengk_malloc."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(np.atleast_1d(shape).tolist())
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(lib().pengk_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_host(cls, ctx, a):
        a = np.ascontiguousarray(a)
        d = cls(ctx, a.shape, a.dtype)
        if d.nbytes:
            _check(lib().pengk_memcpy_h2d(ctx.h, d.ptr, a.ctypes.data, d.nbytes))
        return d

    def to_host(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            _check(lib().pengk_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr and self.ctx.h:
            lib().pengk_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    """device pointer of a DeviceArray, a torch tensor or a raw int."""
    if isinstance(x, DeviceArray):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class Context:
    def __init__(self, device=0):
        h = C.c_void_p()
        self.h = None
        _check(lib().pengk_create(device, C.byref(h)))
        self.h = h.value
        self._keep = []
        self.W = None

    def close(self):
        if self.h:
            for k in self._keep:
                if isinstance(k, DeviceArray):
                    k.free()
            self._keep = []
            lib().pengk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().pengk_synchronize(self.h))

    def stream(self):
        """the hipStream_t the context enqueues on, as an int (pengk_stream; 0 = the null stream)"""
        return int(lib().pengk_stream(self.h) or 0)

    def set_stream(self, s):
        """re-target the context to a caller-owned stream (pengk_set_stream; waits for the work pending on the old one):
        a torch.cuda.Stream, a hipStream_t as an int, or None / 0 for the null stream.  The caller keeps the stream alive."""
        if s is not None and hasattr(s, "cuda_stream"):
            s = s.cuda_stream
        _check(lib().pengk_set_stream(self.h, C.c_void_p(int(s) if s else 0)))

    def set_option(self, name, value):
        _check(lib().pengk_set_option(self.h, name.encode(), int(value)))

    def test_em_generation(self, generation):
        """Test hook: the serial EM by an earlier generation of the library (0 fold, 1 scan; 2 / 3 the current scheme)."""
        _check(lib().pengk_test_em_generation(self.h, int(generation)))

    def info(self, name):
        v = C.c_int64()
        _check(lib().pengk_get_info(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def to_device(self, a):
        return DeviceArray.from_host(self, a)

    # ---- timers -----------------------------------------------------------------------------
    def timer(self):
        t = C.c_void_p()
        _check(lib().pengk_timer_create(self.h, C.byref(t)))
        return t.value

    def record(self, t):
        _check(lib().pengk_timer_record(self.h, t))

    def elapsed_ms(self, a, b):
        ms = C.c_float()
        _check(lib().pengk_timer_elapsed_ms(self.h, a, b, C.byref(ms)))
        return float(ms.value)

    # ---- sequences ----------------------------------------------------------------------------
    def set_sequences(self, words, items, n_words, n_items, W, item_windows, max_bin_bound, all_whole):
        _check(lib().pengk_set_sequences(self.h, _ptr(words), n_words, _ptr(items), n_items, W, item_windows,
                                         max_bin_bound, all_whole))
        self._keep = [words, items]
        self.W = W

    def upload(self, packed):
        words = self.to_device(packed.words)
        items = self.to_device(packed.items if len(packed.items) else np.zeros(1, np.uint64))
        self.set_sequences(words, items, len(packed.words), len(packed.items), packed.W, packed.item_windows,
                           packed.max_bin_bound, packed.all_whole)
        self.set_option("n_windows_hint", packed.n_windows)
        return words, items

    def synth(self, seed, seq0, n_seq, L, W, item_windows=0, words=None, items=None):
        nw, ni = C.c_uint64(), C.c_uint64()
        _check(lib().pengk_synth_sizes(n_seq, L, W, item_windows, C.byref(nw), C.byref(ni)))
        if words is None:
            words = self.empty(nw.value, np.uint64)
        if items is None:
            items = self.empty(max(ni.value, 1), np.uint64)
        _check(lib().pengk_synth_sequences(self.h, seed, seq0, n_seq, L, W, item_windows, _ptr(words), _ptr(items)))
        self._keep = [words, items]
        self.W = W
        return words, items, int(nw.value), int(ni.value)

    # ---- kernels ------------------------------------------------------------------------------
    def count(self, both, counts=None, ltot=None):
        if counts is None:
            counts = self.empty(4 ** self.W, np.uint32)
        if ltot is None:
            ltot = self.empty(1, np.uint64)
        _check(lib().pengk_count(self.h, int(both), _ptr(counts), _ptr(ltot)))
        return counts, ltot

    def count_bg(self, both, counts=None, ltot=None, bg=None):
        counts = counts if counts is not None else self.empty(4 ** self.W, np.uint32)
        ltot = ltot if ltot is not None else self.empty(1, np.uint64)
        bg = bg if bg is not None else self.empty(84, np.uint64)
        _check(lib().pengk_count_bg(self.h, int(both), _ptr(counts), _ptr(ltot), _ptr(bg)))
        return counts, ltot, bg

    def mirror(self, W, counts):
        _check(lib().pengk_mirror_counts(self.h, W, _ptr(counts)))

    def bg_count(self, out=None):
        if out is None:
            out = self.empty(84, np.uint64)
        _check(lib().pengk_bg_count(self.h, _ptr(out)))
        return out

    def bg_model(self, bg_counts, K=2, alpha=(1.0, 1.0, 1.0), out=None):
        if out is None:
            out = self.empty(84, np.float32)
        a = np.asarray(alpha, np.float32)
        _check(lib().pengk_bg_model(self.h, _ptr(bg_counts), K, a.ctypes.data, _ptr(out)))
        return out

    def pattern_stats(self, W, both, k, max_k, V, ltot, counts, bgprob=None, expected=None, logp=None, z=None):
        n = 4 ** W
        bgprob = bgprob if bgprob is not None else self.empty((max_k + 1, n), np.float32)
        expected = expected if expected is not None else self.empty(n, np.float32)
        logp = logp if logp is not None else self.empty(n, np.float32)
        z = z if z is not None else self.empty(n, np.float32)
        _check(lib().pengk_pattern_stats(self.h, W, int(both), k, max_k, _ptr(V), _ptr(ltot), _ptr(counts), _ptr(bgprob),
                                         _ptr(expected), _ptr(logp), _ptr(z)))
        return bgprob, expected, logp, z

    def pattern_stats_control(self, W, both, k, max_k, V, ltot, counts, ctrl_counts, ctrl_ltot, pseudocount=1.0, bgprob=None,
                              expected=None, logp=None, z=None):
        """the sweep held to a control set's counts as a second null (pengk_pattern_stats_control)"""
        n = 4 ** W
        bgprob = bgprob if bgprob is not None else self.empty((max_k + 1, n), np.float32)
        expected = expected if expected is not None else self.empty(n, np.float32)
        logp = logp if logp is not None else self.empty(n, np.float32)
        z = z if z is not None else self.empty(n, np.float32)
        _check(lib().pengk_pattern_stats_control(self.h, W, int(both), k, max_k, _ptr(V), _ptr(ltot), _ptr(counts), _ptr(ctrl_counts),
                                                 _ptr(ctrl_ltot), float(pseudocount), _ptr(bgprob), _ptr(expected), _ptr(logp), _ptr(z)))
        return bgprob, expected, logp, z

    def pattern_stats_strata(self, W, both, k, max_k, V, windows, ltot, counts, ctrl_counts=None, ctrl_ltot=None, pseudocount=0.0,
                             bgprob=None, expected=None, logp=None, z=None, n_strata=None):
        """the sweep under the mixture of the strata's models (pengk_pattern_stats_strata).  V: device float32
        [n_strata x 84]; windows: the n_strata host weights; ctrl_counts / ctrl_ltot / pseudocount: the control of
        pattern_stats_control, or none.  n_strata: another count than len(windows) (argument tests)."""
        w = np.ascontiguousarray(windows, np.uint64)
        n = 4 ** W
        bgprob = bgprob if bgprob is not None else self.empty((max_k + 1, n), np.float32)
        expected = expected if expected is not None else self.empty(n, np.float32)
        logp = logp if logp is not None else self.empty(n, np.float32)
        z = z if z is not None else self.empty(n, np.float32)
        _check(lib().pengk_pattern_stats_strata(self.h, W, int(both), k, max_k, _ptr(V), len(w) if n_strata is None else n_strata,
                                                w.ctypes.data, _ptr(ltot), _ptr(counts),
                                                None if ctrl_counts is None else _ptr(ctrl_counts),
                                                None if ctrl_ltot is None else _ptr(ctrl_ltot), float(pseudocount), _ptr(bgprob),
                                                _ptr(expected), _ptr(logp), _ptr(z)))
        return bgprob, expected, logp, z

    def strata_bg_count(self, scan, stratum, n_strata, W, all_valid=False, bg=None, windows=None, n_seq=None, want_windows=True):
        """(bg, windows), both on the device: the n_strata x 84 background counters and the n_strata window counts of `scan`
        under the strata `stratum` (device uint16 per sequence; pengk_strata_bg_count).  all_valid: d_valid = NULL.  bg /
        windows: device uint64 arrays to ADD to instead of fresh zeroed ones.  want_windows = False: d_windows = NULL.
        n_seq: another count than scan[4] (argument tests)."""
        rows = max(1, min(int(n_strata), 16))
        if bg is None:
            bg = self.to_device(np.zeros((rows, 84), np.uint64))
        if windows is None and want_windows:
            windows = self.to_device(np.zeros(rows, np.uint64))
        _check(lib().pengk_strata_bg_count(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                           scan[4] if n_seq is None else n_seq, _ptr(stratum), int(n_strata), int(W), _ptr(bg),
                                           _ptr(windows) if want_windows else None))
        return bg, windows

    def bg_count_order(self, scan, K, all_valid=False, bg=None, n_seq=None):
        """the (4^(K+2) - 4) / 3 background counters of orders 0 .. K of `scan`, on the device (pengk_bg_count_order).
        all_valid: d_valid = NULL.  bg: a device uint64 array to ADD to instead of a fresh zeroed one.  n_seq: another
        count than scan[4] (argument tests)."""
        if bg is None:
            bg = self.to_device(np.zeros(order_table_size(max(0, min(int(K), 5))), np.uint64))
        _check(lib().pengk_bg_count_order(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                          scan[4] if n_seq is None else n_seq, int(K), _ptr(bg)))
        return bg

    def pattern_stats_order(self, W, both, k, max_k, V, K, VK, ltot, counts, ctrl_counts=None, ctrl_ltot=None, pseudocount=0.0,
                            bgprob=None, expected=None, logp=None, z=None):
        """the sweep with an order-K model in its highest slot (pengk_pattern_stats_order).  V: device float32[84]; VK:
        device float32, orders 0 .. K back to back; ctrl_counts / ctrl_ltot / pseudocount: the control of
        pattern_stats_control, or none."""
        n = 4 ** W
        bgprob = bgprob if bgprob is not None else self.empty((max_k + 1, n), np.float32)
        expected = expected if expected is not None else self.empty(n, np.float32)
        logp = logp if logp is not None else self.empty(n, np.float32)
        z = z if z is not None else self.empty(n, np.float32)
        _check(lib().pengk_pattern_stats_order(self.h, W, int(both), k, max_k, _ptr(V), int(K), _ptr(VK), _ptr(ltot), _ptr(counts),
                                               None if ctrl_counts is None else _ptr(ctrl_counts),
                                               None if ctrl_ltot is None else _ptr(ctrl_ltot), float(pseudocount), _ptr(bgprob),
                                               _ptr(expected), _ptr(logp), _ptr(z)))
        return bgprob, expected, logp, z

    def iupac_aggregate(self, W, both, ids, counts, bgp, expected):
        ids = np.ascontiguousarray(ids, np.uint64)
        out = np.zeros(len(ids), IUPAC_STATS)
        assert IUPAC_STATS.itemsize == 24
        _check(lib().pengk_iupac_aggregate(self.h, W, int(both), ids.ctypes.data, len(ids), _ptr(counts), _ptr(bgp),
                                           _ptr(expected), out.ctypes.data))
        return out

    def em(self, W, pwms, counts, bg, saturation=1e4, threshold=0.08, max_iterations=10):
        p = np.ascontiguousarray(pwms, np.float32).copy().reshape(-1, W, 4)
        n = p.shape[0]
        iters = np.zeros(n, np.int32)
        change = np.zeros(n, np.float32)
        _check(lib().pengk_em(self.h, W, n, p.ctypes.data, saturation, threshold, max_iterations, _ptr(counts), _ptr(bg),
                              iters.ctypes.data, change.ctypes.data))
        return p, iters, change

    def sequential_sum(self, terms):
        """left-to-right float32 sums of the rows of a 2-D array (pengk_sequential_sum_f32)"""
        t = np.ascontiguousarray(terms, np.float32)
        t = t.reshape(1, -1) if t.ndim == 1 else t
        d_t = DeviceArray.from_host(self, t.reshape(-1)) if t.size else None
        d_o = DeviceArray.from_host(self, np.zeros(max(t.shape[0], 1), np.float32))
        _check(lib().pengk_sequential_sum_f32(self.h, _ptr(d_t) if d_t is not None else None, t.shape[0], t.shape[1], _ptr(d_o)))
        return d_o.to_host()[:t.shape[0]]

    # ---- motif scoring (scripts/shoot_peng.py's second step) -------------------------------------------------
    def upload_scan(self, layout):
        """device copy of a ScanLayout: (words, valid, offs, lens, n_seq)"""
        return (self.to_device(layout.words), self.to_device(layout.valid), self.to_device(layout.offs),
                self.to_device(layout.lens), layout.n_seq)

    def synth_scan(self, seed, seq0, n_seq, L):
        """pengk_synth_sequences' input in the scan layout: (words, valid, offs, lens, n_seq)"""
        nw = n_seq * ((L + 31) // 32)
        words, valid = self.empty(max(nw, 1), np.uint64), self.empty(max(nw, 1), np.uint32)
        offs, lens = self.empty(max(n_seq, 1), np.int64), self.empty(max(n_seq, 1), np.uint32)
        _check(lib().pengk_synth_scan_sequences(self.h, seed, seq0, n_seq, L, _ptr(words), _ptr(valid), _ptr(offs), _ptr(lens)))
        return words, valid, offs, lens, n_seq

    def sample_background(self, scan, seed, seq0, K, thresholds, words=None):
        """negatives in the words layout of `scan` (device); thresholds: uint32 triples of the contexts of orders 0..K"""
        th = np.ascontiguousarray(thresholds, np.uint32).reshape(-1)
        assert len(th) == 3 * (1, 5, 21)[K]
        if words is None:
            words = self.empty(scan[0].shape, np.uint64)
        _check(lib().pengk_sample_background(self.h, seed, seq0, scan[4], _ptr(scan[2]), _ptr(scan[3]), K, th.ctypes.data,
                                             _ptr(words)))
        return words

    def shuffle_sequences(self, scan, seed, seq0, all_valid=False, words=None, valid=None):
        """dinucleotide-preserving shuffles of the sequences of `scan` in its layout (device): (words, valid).
        all_valid: the input's validity words are not read (d_valid = NULL) and validity words are written only into a
        `valid` buffer given by the caller (else None is returned for them)"""
        if words is None:
            words = self.empty(scan[0].shape, np.uint64)
        if valid is None and not all_valid:
            valid = self.empty(scan[1].shape, np.uint32)
        _check(lib().pengk_shuffle_sequences(self.h, seed, seq0, scan[4], _ptr(scan[0]), None if all_valid else _ptr(scan[1]),
                                             _ptr(scan[2]), _ptr(scan[3]), _ptr(words), None if valid is None else _ptr(valid)))
        return words, valid

    def motif_scan(self, scan, S, lens, both, words=None, all_valid=False, best=None):
        """best[m, i] of every motif on every sequence of `scan`; S: n x w x 4 int32 (padded to MAX_MOTIF_LEN here)"""
        n = len(lens)
        Sp = np.zeros((max(n, 1), MAX_MOTIF_LEN, 4), np.int32)
        for m in range(n):
            Sp[m, :lens[m]] = np.asarray(S[m], np.int32)[:lens[m]]
        ln = np.ascontiguousarray(lens, np.int32)
        if best is None:
            best = self.empty((max(n, 1), max(scan[4], 1)), np.int32)
        _check(lib().pengk_motif_scan(self.h, _ptr(words if words is not None else scan[0]), None if all_valid else _ptr(scan[1]),
                                      _ptr(scan[2]), _ptr(scan[3]), scan[4], n, Sp.ctypes.data, ln.ctypes.data, int(both),
                                      _ptr(best)))
        return best

    def score_histograms(self, best, n_seq, lo, hi, hist=None):
        """add the histograms of best (n_motifs x n_seq, device) to hist (device uint64; allocated zeroed if None);
        returns (hist, offsets)"""
        lo = np.ascontiguousarray(lo, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        nb = hi.astype(np.int64) - lo + 2
        offs = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
        if hist is None:
            hist = self.to_device(np.zeros(int(offs[-1]), np.uint64))
        _check(lib().pengk_score_histograms(self.h, len(lo), _ptr(best), n_seq, lo.ctypes.data, hi.ctypes.data,
                                            offs.ctypes.data, _ptr(hist)))
        return hist, offs

    # ---- motif sites (--sites) ------------------------------------------------------------------------------
    def sites_count(self, scan, S, lens, both, thr, counts=None):
        """counts[m, i] (device uint64): sites of motif m on sequence i of `scan` at thresholds thr"""
        n = len(lens)
        Sp, ln = _pad_motifs(S, lens)
        th = np.ascontiguousarray(thr, np.int32)
        if counts is None:
            counts = self.empty((max(n, 1), max(scan[4], 1)), np.uint64)
        _check(lib().pengk_sites_count(self.h, _ptr(scan[0]), _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], n,
                                       Sp.ctypes.data, ln.ctypes.data, int(both), th.ctypes.data, _ptr(counts)))
        return counts

    # ---- erasing sites and packing on the device (--erase) --------------------------------------------------
    def mask_sites(self, scan, S, lens, both, thr, all_valid=False, out_valid=None, sites=None, erased=None):
        """(out_valid, sites, erased), all on the device: the validity words of `scan` with the sites of the motifs at
        thresholds thr cleared (pengk_mask_sites), the site window strands per motif and the bits cleared.  all_valid:
        d_valid = NULL.  sites / erased: device uint64 arrays to ADD to instead of fresh zeroed ones."""
        n = len(lens)
        Sp, ln = _pad_motifs(S, lens)
        th = np.ascontiguousarray(thr, np.int32)
        if out_valid is None:
            out_valid = self.empty(scan[0].shape, np.uint32)
        if sites is None:
            sites = self.to_device(np.zeros(max(n, 1), np.uint64))
        if erased is None:
            erased = self.to_device(np.zeros(1, np.uint64))
        _check(lib().pengk_mask_sites(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                      scan[4], n, Sp.ctypes.data, ln.ctypes.data, int(both), th.ctypes.data, _ptr(out_valid),
                                      _ptr(sites), _ptr(erased)))
        return out_valid, sites, erased

    # ---- masking low-complexity stretches (--mask-low-complexity) ---------------------------------------------
    def mask_low_complexity(self, scan, threshold=20, all_valid=False, out_valid=None, masked=None, n_seq=None):
        """(out_valid, masked), both on the device: the validity words of `scan` with the cover of its perfect intervals
        cleared (pengk_mask_low_complexity) and the two counts -- bits cleared, sequences that lost one.  all_valid:
        d_valid = NULL.  masked: a device array of 2 uint64 to ADD to instead of a fresh zeroed one.  n_seq: another count
        than scan[4] (argument tests)."""
        if out_valid is None:
            out_valid = self.empty(scan[0].shape, np.uint32)
        if masked is None:
            masked = self.to_device(np.zeros(2, np.uint64))
        _check(lib().pengk_mask_low_complexity(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]),
                                               _ptr(scan[3]), scan[4] if n_seq is None else n_seq, int(threshold),
                                               _ptr(out_valid), _ptr(masked)))
        return out_valid, masked

    # ---- spaced dyads (--dyads) -------------------------------------------------------------------------------
    def dyad_count(self, scan, max_gap, both, all_valid=False, counts=None, mono=None, n_seq=None):
        """(counts, mono), both on the device: the (max_gap + 1) x 4096 dyad table and the 64 triplet counts of `scan`
        (pengk_dyad_count).  all_valid: d_valid = NULL.  counts / mono: device uint64 arrays to ADD to instead of fresh
        zeroed ones.  n_seq: another count than scan[4] (argument tests)."""
        if counts is None:
            counts = self.to_device(np.zeros((max(0, min(int(max_gap), DYAD_MAX_GAP)) + 1, 4096), np.uint64))
        if mono is None:
            mono = self.to_device(np.zeros(64, np.uint64))
        _check(lib().pengk_dyad_count(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                      scan[4] if n_seq is None else n_seq, int(max_gap), int(both), _ptr(counts), _ptr(mono)))
        return counts, mono

    # ---- positional words (--positional) ----------------------------------------------------------------------
    def position_count(self, scan, K, anchor, bin_size, n_bins, both, all_valid=False, counts=None, n_seq=None):
        """the n_bins x 4^K table of clump heads per position bin of `scan`, on the device (pengk_position_count).
        anchor: 0 start, 1 end, 2 centre.  all_valid: d_valid = NULL.  counts: a device uint64 array to ADD to instead of
        a fresh zeroed one.  n_seq: another count than scan[4] (argument tests)."""
        if counts is None:
            rows = max(1, min(int(n_bins), POSITION_MAX_BINS))
            counts = self.to_device(np.zeros((rows, 4 ** max(POSITION_MIN_K, min(int(K), POSITION_MAX_K))), np.uint64))
        _check(lib().pengk_position_count(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                          scan[4] if n_seq is None else n_seq, int(K), int(anchor), int(bin_size), int(n_bins),
                                          int(both), _ptr(counts)))
        return counts

    def position_pairs(self, scan, K, anchor, bin_size, n_bins, both, all_valid=False, pairs=None, n_seq=None):
        """the n_bins x 16 table of the first pairs of the words standing in each position bin of `scan`, on the device
        (pengk_position_pairs): the arguments of position_count; pairs: a device uint64 array to ADD to."""
        if pairs is None:
            pairs = self.to_device(np.zeros((max(1, min(int(n_bins), POSITION_MAX_BINS)), 16), np.uint64))
        _check(lib().pengk_position_pairs(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                          scan[4] if n_seq is None else n_seq, int(K), int(anchor), int(bin_size), int(n_bins),
                                          int(both), _ptr(pairs)))
        return pairs

    def pack_scan(self, scan, W, item_windows=0, valid=None, all_valid=False, attach=False):
        """the sequences of `scan` (under the validity words `valid` instead of its own, when given) in the count layout,
        packed on the device: (words, items, figures) -- two device uint64 arrays and the PackedStruct of
        pengk_pack_scan_sizes.  attach: pengk_set_sequences on the result, as Context.upload does for a host pack."""
        v = None if all_valid else _ptr(valid if valid is not None else scan[1])
        n = scan[4]
        base, item = self.empty(max(n, 1), np.uint64), self.empty(max(n, 1), np.uint64)
        st = PackedStruct()
        _check(lib().pengk_pack_scan_sizes(self.h, v, _ptr(scan[2]), _ptr(scan[3]), n, W, item_windows, _ptr(base), _ptr(item),
                                           C.byref(st)))
        words, items = self.empty(st.n_words, np.uint64), self.empty(max(st.n_items, 1), np.uint64)
        _check(lib().pengk_pack_scan(self.h, _ptr(scan[0]), v, _ptr(scan[2]), _ptr(scan[3]), n, W, item_windows, _ptr(base),
                                     _ptr(item), _ptr(words), st.n_words, _ptr(items), st.n_items))
        self.synchronize()  # (the offset arrays die with this call)
        if attach:
            self.set_sequences(words, items, st.n_words, st.n_items, st.W, st.item_windows, st.max_bin_bound, st.all_whole)
            self.set_option("n_windows_hint", st.n_windows)
        return words, items, st

    # ---- a control set matched to the input (--score-negatives control) -------------------------------------
    def seq_strata(self, scan, gc_bins=10, use_length=True, all_valid=False, stratum=None, hist=None, n_seq=None):
        """(stratum, hist), both on the device: the stratum (length bin * gc_bins + GC bin, 0xFFFF without a valid base) of
        every sequence of `scan` and the 256 stratum counts (pengk_seq_strata).  all_valid: d_valid = NULL.  hist: a device
        array of 256 uint64 to ADD to instead of a fresh zeroed one.  n_seq: another count than scan[4] (argument tests)."""
        if stratum is None:
            stratum = self.empty(max(scan[4], 1), np.uint16)
        if hist is None:
            hist = self.to_device(np.zeros(256, np.uint64))
        _check(lib().pengk_seq_strata(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]),
                                      scan[4] if n_seq is None else n_seq, int(gc_bins), int(use_length), _ptr(stratum), _ptr(hist)))
        return stratum, hist

    def select_strata(self, stratum, n_seq, count, quota, rank0, offs, lens):
        """(sel_offs, sel_lens, sel_index, n_sel): the kept sequences of this call's n_seq (their strata in `stratum`, device
        uint16) as compacted device arrays -- with the words of the layout that offs / lens belong to, a scan layout of
        n_sel sequences -- and their count (pengk_select_strata).  count / quota / rank0: 256 uint64 each, host."""
        c = np.ascontiguousarray(count, np.uint64)
        q = np.ascontiguousarray(quota, np.uint64)
        r0 = np.ascontiguousarray(rank0, np.uint64)
        assert c.shape == q.shape == r0.shape == (256,)
        so, sl = self.empty(max(n_seq, 1), np.int64), self.empty(max(n_seq, 1), np.uint32)
        si = self.empty(max(n_seq, 1), np.uint32)
        n_sel = C.c_uint64()
        _check(lib().pengk_select_strata(self.h, _ptr(stratum), n_seq, c.ctypes.data, q.ctypes.data, r0.ctypes.data, _ptr(offs),
                                         _ptr(lens), _ptr(so), _ptr(sl), _ptr(si), C.byref(n_sel)))
        return so, sl, si, int(n_sel.value)

    # ---- a hold-out share (--holdout) ------------------------------------------------------------------------
    def split_sequences(self, seed, seq0, n_seq, threshold, offs, lens, index=None, want_class=False):
        """((offs0, lens0, index0, n0), (offs1, lens1, index1, n1), cls): the training and the hold-out share of this call's
        n_seq sequences as compacted device arrays -- with the words of the layout that offs / lens belong to, two scan
        layouts -- and, want_class, the class of every sequence as a device uint8 array, else None
        (pengk_split_sequences).  index: a device uint32 array of local indices to hash instead of 0 .. n_seq - 1."""
        m = max(n_seq, 1)
        out = [(self.empty(m, np.int64), self.empty(m, np.uint32), self.empty(m, np.uint32)) for _ in range(2)]
        cls = self.empty(m, np.uint8) if want_class else None
        n0, n1 = C.c_uint64(), C.c_uint64()
        _check(lib().pengk_split_sequences(self.h, int(seed), int(seq0), int(n_seq), int(threshold),
                                           None if index is None else _ptr(index), _ptr(offs), _ptr(lens),
                                           None if cls is None else _ptr(cls), _ptr(out[0][0]), _ptr(out[0][1]), _ptr(out[0][2]),
                                           C.byref(n0), _ptr(out[1][0]), _ptr(out[1][1]), _ptr(out[1][2]), C.byref(n1)))
        return out[0] + (int(n0.value),), out[1] + (int(n1.value),), cls

    def sites_histograms(self, scan, S, lens, both, thr, hi, counts=None, hist=None, tests=None, offs=None):
        """(hists, tests): hists[m] (uint64, max(0, hi[m] - thr[m] + 1) bins) the sites of motif m by score - thr[m], tests[m]
        its scored window strands (pengk_sites_histograms; downloaded).  counts: a device n_motifs x n_seq uint64 array
        to fill as sites_count does.  hist / tests: device uint64 arrays to ADD to instead of fresh zeroed ones (motif m's
        bins from hist[offs[m]] on, default back to back); what is returned is then their content after the call."""
        n = len(lens)
        Sp, ln = _pad_motifs(S, lens)
        th = np.ascontiguousarray(thr, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        nb = np.maximum(hi.astype(np.int64) - th.astype(np.int64) + 1, 0)
        if offs is None:
            offs = np.concatenate([[0], np.cumsum(nb)])[:max(n, 1)]
        offs = np.ascontiguousarray(offs, np.uint64)
        if hist is None:
            hist = self.to_device(np.zeros(max(int(nb.sum()), 1), np.uint64))
        if tests is None:
            tests = self.to_device(np.zeros(max(n, 1), np.uint64))
        _check(lib().pengk_sites_histograms(self.h, _ptr(scan[0]), _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], n,
                                            Sp.ctypes.data, ln.ctypes.data, int(both), th.ctypes.data, hi.ctypes.data,
                                            offs.ctypes.data, _ptr(hist), _ptr(tests),
                                            _ptr(counts) if counts is not None else None))
        h = hist.to_host()
        return [h[int(offs[m]):int(offs[m]) + int(nb[m])].copy() for m in range(n)], tests.to_host()[:n]

    def motif_enrich(self, scan, S, lens, both, thr, hi, words=None, valid=None, all_valid=False, hist=None, scored=None,
                     offs=None, n_seq=None):
        """(hists, scored): hists[m] (uint64, max(0, hi[m] - thr[m] + 1) bins) the sequences of `scan` by their best score
        of motif m minus thr[m], scored[m] the sequences with a window of valid bases (pengk_motif_enrich; downloaded).
        words / valid: other words in the layout of `scan` (negatives); all_valid: d_valid = NULL.  hist / scored: device
        uint64 arrays to ADD to instead of fresh zeroed ones (motif m's bins from hist[offs[m]] on, default back to
        back); what is returned is then their content after the call.  n_seq: another count than scan[4] (argument
        tests)."""
        n = len(lens)
        Sp, ln = _pad_motifs(S, lens)
        th = np.ascontiguousarray(thr, np.int32)
        hi = np.ascontiguousarray(hi, np.int32)
        nb = np.maximum(hi.astype(np.int64) - th.astype(np.int64) + 1, 0)
        if offs is None:
            offs = np.concatenate([[0], np.cumsum(nb)])[:max(n, 1)]
        offs = np.ascontiguousarray(offs, np.uint64)
        if hist is None:
            hist = self.to_device(np.zeros(max(int(nb.sum()), 1), np.uint64))
        if scored is None:
            scored = self.to_device(np.zeros(max(n, 1), np.uint64))
        w = words if words is not None else scan[0]
        v = None if all_valid else _ptr(valid if valid is not None else scan[1])
        _check(lib().pengk_motif_enrich(self.h, _ptr(w), v, _ptr(scan[2]), _ptr(scan[3]), scan[4] if n_seq is None else n_seq, n,
                                        Sp.ctypes.data, ln.ctypes.data, int(both), th.ctypes.data, hi.ctypes.data,
                                        offs.ctypes.data, _ptr(hist), _ptr(scored)))
        h = hist.to_host()
        return [h[int(offs[m]):int(offs[m]) + int(nb[m])].copy() for m in range(n)], scored.to_host()[:n]

    def sites_slices(self, counts, n_seq, n_motifs):
        """(bounds, records, motif_totals) of pengk_sites_slices"""
        tot = np.zeros(max(n_motifs, 1), np.uint64)
        cap = 64
        while True:
            bounds, recs, ns = np.zeros(cap + 1, np.uint64), np.zeros(cap, np.uint64), C.c_uint64()
            _check(lib().pengk_sites_slices(self.h, _ptr(counts), n_seq, n_motifs, tot.ctypes.data, cap, bounds.ctypes.data,
                                            recs.ctypes.data, C.byref(ns)))
            if ns.value <= cap:
                k = ns.value
                return bounds[:k + 1] if k else np.zeros(1, np.uint64), recs[:k], tot[:n_motifs]
            cap = ns.value

    def sites_emit(self, scan, S, lens, both, thr, counts, i0, i1, out, cap):
        Sp, ln = _pad_motifs(S, lens)
        th = np.ascontiguousarray(thr, np.int32)
        _check(lib().pengk_sites_emit(self.h, _ptr(scan[0]), _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], len(lens),
                                      Sp.ctypes.data, ln.ctypes.data, int(both), th.ctypes.data, _ptr(counts), i0, i1,
                                      _ptr(out) if out is not None else None, cap))

    def sites_records(self, scan, S, lens, both, thr, counts, i0, i1, n_records, buf=None):
        """the n_records pengk_site records of sequences [i0, i1) as pengk_sites_emit wrote them (a SITE array: motif,
        then sequence within the slice, then position, + before -; not regrouped); buf: a device buffer to reuse"""
        if buf is None or buf.nbytes < max(n_records, 1) * SITE.itemsize:
            buf = self.empty(max(n_records, 1) * SITE.itemsize, np.uint8)
        self.sites_emit(scan, S, lens, both, thr, counts, i0, i1, buf, n_records)
        return buf.to_host()[:n_records * SITE.itemsize].view(SITE).copy()

    def motif_sites(self, scan, S, lens, both, thr):
        """every site, in the --sites order (motif, global sequence, position, + before -): a SITE array whose seq field
        is the global sequence index (uint64 here), plus the count pass's per-motif totals"""
        n_seq, n = scan[4], len(lens)
        counts = self.sites_count(scan, S, lens, both, thr)
        bounds, recs, tot = self.sites_slices(counts, n_seq, n)
        cap = int(recs.max()) if len(recs) else 0
        buf = self.empty(max(cap, 1) * SITE.itemsize, np.uint8)
        parts = []
        for k in range(len(recs)):
            i0, i1 = int(bounds[k]), int(bounds[k + 1])
            self.sites_emit(scan, S, lens, both, thr, counts, i0, i1, buf, cap)
            r = buf.to_host()[:int(recs[k]) * SITE.itemsize].view(SITE)
            parts.append((i0, r))
        out = np.zeros(int(sum(len(r) for _, r in parts)),
                       [("motif", np.int64), ("seq", np.uint64), ("pos", np.uint32), ("strand", np.uint8), ("score", np.int32)])
        # slices are sequence ranges; within one, motif-major: gather motif by motif over the slices
        j = 0
        for m in range(n):
            for i0, r in parts:
                sel = r[(r["motif_strand"] >> 1) == m]
                k = len(sel)
                out["motif"][j:j + k] = m
                out["seq"][j:j + k] = sel["seq"].astype(np.uint64) + np.uint64(i0)
                out["pos"][j:j + k] = sel["pos"]
                out["strand"][j:j + k] = sel["motif_strand"] & 1
                out["score"][j:j + k] = sel["score"]
                j += k
        return out, tot

    # ---- central enrichment (--centrality) ------------------------------------------------------------------
    def motif_best_sites(self, scan, S, lens, both, seq0=0, best=None, site=None):
        """(best, site): the best score and 2p + s of every motif on every sequence of `scan` (device int32 / uint64,
        n_motifs x n_seq); seq0 = the global index of the scan's first sequence (it seeds the tie-break)"""
        n = len(lens)
        Sp, ln = _pad_motifs(S, lens)
        if best is None:
            best = self.empty((max(n, 1), max(scan[4], 1)), np.int32)
        if site is None:
            site = self.empty((max(n, 1), max(scan[4], 1)), np.uint64)
        _check(lib().pengk_motif_best_sites(self.h, _ptr(scan[0]), _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], seq0, n,
                                            Sp.ctypes.data, ln.ctypes.data, int(both), _ptr(best), _ptr(site)))
        return best, site

    def centrality_histograms(self, best, site, lens_dev, n_seq, widths, thr, max_len, hd=None, hl=None):
        """(hd, hl) device uint64, n_motifs x (2 max_len + 1) offset bins and n_motifs x (max_len + 1) length bins, ADDED
        to (allocated zeroed if None)"""
        n = len(widths)
        w = np.ascontiguousarray(widths, np.int32)
        th = np.ascontiguousarray(thr, np.int32)
        if hd is None:
            hd = self.to_device(np.zeros((max(n, 1), 2 * max_len + 1), np.uint64))
        if hl is None:
            hl = self.to_device(np.zeros((max(n, 1), max_len + 1), np.uint64))
        _check(lib().pengk_centrality_histograms(self.h, n, _ptr(best), _ptr(site), _ptr(lens_dev), n_seq, w.ctypes.data,
                                                 th.ctypes.data, max_len, _ptr(hd), _ptr(hl)))
        return hd, hl

    # ---- motif pair spacing (--spacing) ----------------------------------------------------------------------------
    def spacing_histograms(self, best, site, lens_dev, n_seq, widths, thr, max_gap, min_len, max_len, hg=None, hl=None, hm=None):
        """(hg, hl, hm) device uint64: pairs x (4 (max_gap + 1) + 2) gap bins, pairs x (max_len + 1) length bins (pair
        b (b - 1) / 2 + a, a < b) and the n_motifs site counts, ADDED to (allocated zeroed if None)"""
        n = len(widths)
        pairs = n * (n - 1) // 2
        w = np.ascontiguousarray(widths, np.int32)
        th = np.ascontiguousarray(thr, np.int32)
        if hg is None:
            hg = self.to_device(np.zeros((max(pairs, 1), 4 * (max_gap + 1) + 2), np.uint64))
        if hl is None:
            hl = self.to_device(np.zeros((max(pairs, 1), max_len + 1), np.uint64))
        if hm is None:
            hm = self.to_device(np.zeros(max(n, 1), np.uint64))
        _check(lib().pengk_spacing_histograms(self.h, n, _ptr(best), _ptr(site), _ptr(lens_dev), n_seq, w.ctypes.data,
                                              th.ctypes.data, max_gap, min_len, max_len, _ptr(hg), _ptr(hl), _ptr(hm)))
        return hg, hl, hm

    # ---- motif refinement (--refine) ---------------------------------------------------------------------------
    def site_profiles(self, scan, best, site, widths, thr, flank, counts=None):
        """device uint64 n_motifs x MAX_MOTIF_LEN x 5: the base counts of every column in [-F, w + F) of the best sites
        (best, site from motif_best_sites on the same scan) at or above thr, ADDED to counts (allocated zeroed if None)"""
        n = len(widths)
        w = np.ascontiguousarray(widths, np.int32)
        th = np.ascontiguousarray(thr, np.int32)
        if counts is None:
            counts = self.to_device(np.zeros((max(n, 1), MAX_MOTIF_LEN, 5), np.uint64))
        _check(lib().pengk_site_profiles(self.h, _ptr(scan[0]), _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], n, _ptr(best),
                                         _ptr(site), w.ctypes.data, th.ctypes.data, int(flank), _ptr(counts)))
        return counts

    # ---- first-order models (--dinuc) ---------------------------------------------------------------------------
    def site_pair_profiles(self, scan, best, site, widths, thr, flank, counts=None, all_valid=False):
        """device uint64 n_motifs x MAX_MOTIF_LEN x 17: the adjacent-pair counts (bin 4a + b, a the letter before; bin 16:
        not two bases) of every column in (-F, w + F) of the best sites at or above thr, ADDED to counts (allocated
        zeroed if None); all_valid: the validity words are not read (d_valid = NULL)"""
        n = len(widths)
        w = np.ascontiguousarray(widths, np.int32)
        th = np.ascontiguousarray(thr, np.int32)
        if counts is None:
            counts = self.to_device(np.zeros((max(n, 1), MAX_MOTIF_LEN, 17), np.uint64))
        _check(lib().pengk_site_pair_profiles(self.h, _ptr(scan[0]), None if all_valid else _ptr(scan[1]), _ptr(scan[2]),
                                              _ptr(scan[3]), scan[4], n, _ptr(best), _ptr(site), w.ctypes.data, th.ctypes.data,
                                              int(flank), _ptr(counts)))
        return counts

    def motif_scan_dinuc(self, scan, S0, D, lens, both, words=None, all_valid=False, best=None):
        """best[m, i] of every first-order model on every sequence of `scan`; S0: n x 4, D: n x w x 16 int32 (row 0
        unused; padded to MAX_MOTIF_LEN here)"""
        n = len(lens)
        S0p = np.zeros((max(n, 1), 4), np.int32)
        Dp = np.zeros((max(n, 1), MAX_MOTIF_LEN, 16), np.int32)
        for m in range(n):
            S0p[m] = np.asarray(S0[m], np.int32)
            Dp[m, :lens[m]] = np.asarray(D[m], np.int32).reshape(-1, 16)[:lens[m]]
        ln = np.ascontiguousarray(lens, np.int32)
        if best is None:
            best = self.empty((max(n, 1), max(scan[4], 1)), np.int32)
        _check(lib().pengk_motif_scan_dinuc(self.h, _ptr(words if words is not None else scan[0]),
                                            None if all_valid else _ptr(scan[1]), _ptr(scan[2]), _ptr(scan[3]), scan[4], n,
                                            S0p.ctypes.data, Dp.ctypes.data, ln.ctypes.data, int(both), _ptr(best)))
        return best

    # ---- motif comparison (--compare) --------------------------------------------------------------------------
    def compare_nulls(self, queries, targets, both, qlens=None, tlens=None):
        """the null histograms (n_q x MAX_MOTIF_LEN x 257 uint64) of quantised queries against a database of quantised
        targets (lists of w x 4 integer arrays; pengk_compare_nulls)"""
        QX, ql = _pad_columns(queries, qlens)
        TX, tl = _pad_columns(targets, tlens)
        hist = np.zeros((max(len(queries), 1), MAX_MOTIF_LEN, COMPARE_BINS), np.uint64)
        _check(lib().pengk_compare_nulls(self.h, len(queries), QX.ctypes.data, ql.ctypes.data, len(targets), TX.ctypes.data,
                                         tl.ctypes.data, int(both), hist.ctypes.data))
        return hist

    def compare_motifs(self, queries, targets, both, min_overlap=5, qlens=None, tlens=None):
        """(align, p): the best alignment of every (query, target) -- align (n_q x n_t x 5 int32: offset, orientation,
        overlap, score, n_offsets) and its p_offset (n_q x n_t double; pengk_compare_motifs)"""
        QX, ql = _pad_columns(queries, qlens)
        TX, tl = _pad_columns(targets, tlens)
        align = np.zeros((max(len(queries), 1), max(len(targets), 1), 5), np.int32)
        p = np.zeros((max(len(queries), 1), max(len(targets), 1)), np.float64)
        _check(lib().pengk_compare_motifs(self.h, len(queries), QX.ctypes.data, ql.ctypes.data, len(targets), TX.ctypes.data,
                                          tl.ctypes.data, int(both), int(min_overlap), align.ctypes.data, p.ctypes.data))
        return align, p

    def compare_tails(self, hist, w=None):
        """the tail table of one query whose null histograms are hist (w x 257 counts), flat and in the device's order:
        i0 ascending, then n = 1 .. w - i0, each with 256 n + 1 doubles (pengk_test_compare_tails)"""
        h = np.ascontiguousarray(hist, np.uint64).reshape(-1, COMPARE_BINS)
        w = len(h) if w is None else int(w)
        tails = np.zeros(sum(compare_tails_before(w - i0 + 1) for i0 in range(min(max(w, 0), MAX_MOTIF_LEN))) or 1, np.float64)
        _check(lib().pengk_test_compare_tails(self.h, w, h.ctypes.data, tails.ctypes.data))
        return tails

    def em_device(self, W, n_pwm, d_pwms, counts, bg, d_state, d_change, saturation=1e4, threshold=0.08, max_iterations=10):
        _check(lib().pengk_em_device(self.h, W, n_pwm, _ptr(d_pwms), saturation, threshold, max_iterations, _ptr(counts),
                                     _ptr(bg), _ptr(d_state), _ptr(d_change)))

"""ctypes binding of include/raxtax_hip.h.  Fails loudly when libraxtax_hip.so is missing:
there is no Python or CPU fallback for the device path."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
import os as _os

LIB_PATH = Path(_os.environ.get("RTX_LIB_PATH") or PKG / "libraxtax_hip.so")   # RTX_LIB_PATH: an experimental build (tools/)

RTX_MAX_DEPTH = 32
RTX_NUM_KMERS = 65536
RTX_OK = 0
RTX_ERR_INVALID, RTX_ERR_HIP, RTX_ERR_NO_DEVICE, RTX_ERR_OOM = -1, -2, -3, -4
RTX_ERR_PARSE, RTX_ERR_DEPTH, RTX_ERR_STATE, RTX_ERR_TOO_LONG = -5, -6, -7, -8
RTX_SKIP_EXACT_MATCHES = 1
RTX_RAW_CONFIDENCE = 2
RTX_TEXT_TSV = 4
RTX_Q_OK, RTX_Q_NO_KMERS, RTX_Q_ALL_KMERS = 0, 1, 2
RTX_OPT_DEREP = 27                 # rtx_index_set_option: raxtax() classifies each distinct read of a chunk once
RTX_DEFAULT_DEREP_HASH_MASK = 3    # rtx_set_default_option: the hash of rtx_derep_run ANDed with a mask (tests)
RTX_DEFAULT_TALLY_HASH_MASK = 4    # rtx_set_default_option: the hash of rtx_tally_add ANDed with a mask (tests)
RTX_DEFAULT_OTU_HASH_MASK = 5      # rtx_set_default_option: the hashes of rtx_otu_cluster ANDed with a mask (tests)
RTX_DEFAULT_CHIMERA_SLICE = 6      # rtx_set_default_option: a cap on the reads / entries of a slice of rtx_chimera_run / rtx_denovo_check (tests)
RTX_DEFAULT_UNOISE_SLICE = 8       # rtx_set_default_option: a cap on the rows and on the centroids of one launch of rtx_otu_unoise (tests)
RTX_UNOISE_MAX_DIFFS = 16          # rtx_otu_unoise: the most differences a read may have to its parent
RTX_UNOISE_ZOTU, RTX_UNOISE_ABSORBED, RTX_UNOISE_LEFT, RTX_UNOISE_LONG = 0, 1, 2, 3   # rtx_unoise_view_t.status
RTX_OTU_MAX_LEN = 4096
RTX_LIN_UNCLASSIFIABLE, RTX_LIN_UNCLASSIFIED, RTX_LIN_CLASSIFIED = 0, 1, 2   # rtx_lineage_records.kind
STAGES = ("kmer_extract", "hit_count", "prob_table", "taxon_prefix", "lineage_walk", "tile_bounds", "tile_prune", "exact_match", "order", "pair_union")

RTX_TRIM_5P, RTX_TRIM_3P = 0, 1      # rtx_trim_pattern.end
RTX_TRIM_MAX_PATTERNS, RTX_TRIM_MAX_PATTERN, RTX_TRIM_MAX_WINDOW, RTX_TRIM_NO_PATTERN = 8, 64, 256, 0xFF

RTX_DEMUX_MAX_TAGS, RTX_DEMUX_MAX_TAG, RTX_DEMUX_MAX_OFFSET, RTX_DEMUX_MAX_MISMATCHES = 1024, 32, 15, 8
RTX_DEMUX_NO_TAG, RTX_DEMUX_NONE = 0xFFFF, 0xFFFFFFFF
RTX_PROFILE_MAX_SAMPLE_COUNTERS = 1 << 28
RTX_DEMUX_NAMES = ("ok", "no_tag5", "no_tag3", "ambiguous", "unknown_pair")   # a verdict: RTX_DEMUX_OK .. RTX_DEMUX_UNKNOWN_PAIR

RTX_QUAL_MAX_READ, RTX_QUAL_TABLE = 1 << 20, 94
RTX_QC_NAMES = ("bad_quality", "short_for_trunc_len", "too_short", "too_long", "too_many_n", "max_ee", "max_ee_rate")   # bit b of a verdict: RTX_QC_*

RTX_SCREEN_K, RTX_SCREEN_NONE, RTX_SCREEN_MAX_READ, RTX_SCREEN_MAX_BASES, RTX_SCREEN_CONTAMINANT = 16, 0xFFFFFFFF, 1 << 20, 1 << 26, 1

RTX_MERGE_MAX_READ, RTX_MERGE_MISMATCH_COST = 1024, 5
RTX_MG_NAMES = ("bad_quality", "too_long", "too_short", "no_overlap")   # bit b of a verdict: RTX_MG_* (a verdict holds one reason)

RTX_CHIMERA_MAX_QUERY, RTX_CHIMERA_MAX_SEGMENTS, RTX_CHIMERA_DEFAULT_SEGMENTS, RTX_CHIMERA_DEFAULT_MINDELTA = 4096, 32, 16, 24
RTX_CHIM_OK, RTX_CHIM_NO_KMER, RTX_CHIM_TOO_LONG = 0, 1, 2
RTX_DENOVO_NO_PARENT = 3           # rtx_chimera_rec.status of an entry without a parent prefix (rtx_denovo_check)
RTX_DENOVO_DEFAULT_ABSKEW = 2
RTX_DENOVO_DEFAULT_MAX_PARENTS = 262144
RTX_CHIM_FIELDS = ("status", "n_valid", "single", "parent", "seg", "pos", "left", "parent_a", "right", "parent_b", "delta", "flag")   # rtx_chimera_rec: twelve uint32

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)
f32p = C.POINTER(C.c_float)


class NodesView(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("node_begin", u32p), ("node_end", u32p), ("node_first_child", u32p),
                ("node_n_children", u32p), ("node_parent", u32p), ("node_type", u8p)]


class ResultView(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("n_rows", C.c_uint64), ("t", u32p), ("status", u8p),
                ("global_signal", f64p), ("row_begin", u64p), ("row_count", u32p), ("row_lineage", u32p), ("row_node", u32p),
                ("row_depth", u32p), ("row_conf", f64p), ("row_local_signal", f64p),
                ("row_conf_stride", C.c_uint32), ("row_depth_u8", u8p), ("row_conf_hundredths", u8p)]   # ABI 5 (0 / NULL in a hand-made view)


class TextView(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("out", C.c_void_p), ("out_off", u64p), ("tsv", C.c_void_p), ("tsv_off", u64p)]


class ProfileView(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("cutoff_hundredths", C.c_uint32), ("flags", C.c_uint32), ("clade", u64p), ("direct", u64p),
                ("conf_sum", u64p), ("totals", C.c_uint64 * 4)]


class SampleProfileView(C.Structure):   # rtx_sample_profile_view
    _fields_ = [("n_nodes", C.c_uint32), ("n_samples", C.c_uint32), ("cutoff_hundredths", C.c_uint32), ("flags", C.c_uint32), ("direct", u64p), ("totals", u64p)]


class TrimPattern(C.Structure):
    _fields_ = [("codes", u8p), ("len", C.c_uint32), ("end", C.c_uint32), ("max_errors", C.c_uint32), ("window", C.c_uint32)]


class DemuxTag(C.Structure):   # rtx_demux_tag
    _fields_ = [("codes", u8p), ("len", C.c_uint32), ("end", C.c_uint32)]


class DemuxPair(C.Structure):   # rtx_demux_pair
    _fields_ = [("tag5", C.c_uint32), ("tag3", C.c_uint32), ("sample", C.c_uint32)]


class DemuxParams(C.Structure):   # rtx_demux_params
    _fields_ = [("max_mismatches", C.c_uint32), ("max_offset", C.c_uint32)]


class QualParams(C.Structure):   # rtx_qual_params
    _fields_ = [("ascii_base", C.c_uint32), ("trunc_len", C.c_uint32), ("trunc_qual", C.c_int32), ("trunc_ee", C.c_double), ("min_len", C.c_uint32),
                ("max_len", C.c_uint32), ("max_ns", C.c_int32), ("max_ee", C.c_double), ("max_ee_rate", C.c_double)]


class ScreenParams(C.Structure):   # rtx_screen_params
    _fields_ = [("min_hits", C.c_uint32), ("min_pct", C.c_uint32)]


class TallyParams(C.Structure):   # rtx_tally_params
    _fields_ = [("n_samples", C.c_uint32), ("max_entries", C.c_uint64), ("max_bytes", C.c_uint64), ("initial_entries", C.c_uint64), ("initial_bytes", C.c_uint64)]


class LineageRecords(C.Structure):   # rtx_lineage_records
    _fields_ = [("kind", u8p), ("L", u8p), ("node", u32p), ("hund", u8p), ("hund_stride", C.c_uint32)]


class OtuTaxonomyParams(C.Structure):   # rtx_otu_taxonomy_params
    _fields_ = [("agree_pct", C.c_uint32), ("flags", C.c_uint32)]


class OtuTaxonomyView(C.Structure):   # rtx_otu_taxonomy_view_t
    _fields_ = [("n_rows", C.c_uint64), ("n_otus", C.c_uint64), ("n_nodes", C.c_uint32), ("agree_pct", C.c_uint32), ("stride", C.c_uint32), ("sizes", u64p), ("members", u64p),
                ("classified", u64p), ("depth", u32p), ("node", u32p), ("seed_rel", u8p), ("clade", u64p), ("conf", u64p), ("packed_waves", C.c_uint64), ("big_otus", C.c_uint64)]


class TallyView(C.Structure):   # rtx_tally_view
    _fields_ = [("n_entries", C.c_uint64), ("n_columns", C.c_uint32), ("bases", C.POINTER(C.c_uint8)), ("base_off", C.POINTER(C.c_uint64)), ("counts", C.POINTER(C.c_uint64)),
                ("sizes", C.POINTER(C.c_uint64)), ("first", C.POINTER(C.c_uint64)), ("totals", C.c_uint64 * 3)]


class OtuParams(C.Structure):   # rtx_otu_params
    _fields_ = [("differences", C.c_uint32), ("flags", C.c_uint32), ("initial_links", C.c_uint64)]


class OtuView(C.Structure):   # rtx_otu_view_t
    _fields_ = [("n_rows", C.c_uint64), ("n_otus", C.c_uint64), ("n_columns", C.c_uint32), ("otu", u32p), ("seed", u32p), ("members", u64p), ("sizes", u64p), ("counts", u64p),
                ("n_links", C.c_uint64), ("link_a", u32p), ("link_b", u32p), ("rounds", C.c_uint32), ("link_passes", C.c_uint32), ("long_rows", C.c_uint64)]


class GraftParams(C.Structure):   # rtx_graft_params
    _fields_ = [("boundary", C.c_uint64), ("bloom_log2", C.c_uint32), ("flags", C.c_uint32), ("max_bloom_bytes", C.c_uint64), ("initial_candidates", C.c_uint64)]


class UnoiseParams(C.Structure):   # rtx_unoise_params
    _fields_ = [("minsize", C.c_uint64), ("alpha", C.c_uint32), ("max_diffs", C.c_uint32), ("flags", C.c_uint32)]


class UnoiseView(C.Structure):   # rtx_unoise_view_t
    _fields_ = [("n_rows", C.c_uint64), ("status", C.POINTER(C.c_uint8)), ("parent", u32p), ("dist", u32p), ("lim", u32p), ("n_zotu", C.c_uint64), ("n_absorbed", C.c_uint64),
                ("n_left", C.c_uint64), ("n_long", C.c_uint64), ("minsize", C.c_uint64), ("alpha", C.c_uint32), ("max_diffs", C.c_uint32), ("tiers", C.c_uint32),
                ("launches", C.c_uint32), ("pairs", C.c_uint64), ("pairs_length", C.c_uint64), ("pairs_finished", C.c_uint64), ("seconds", C.c_double * 4)]


class GraftView(C.Structure):   # rtx_graft_view_t
    _fields_ = [("n_rows", C.c_uint64), ("n_old_otus", C.c_uint64), ("n_otus", C.c_uint64), ("n_grafts", C.c_uint64), ("boundary", C.c_uint64), ("parent", u32p), ("old_to_new", u32p),
                ("light", u32p), ("child", u32p), ("par", u32p), ("heavy", u32p), ("into", u32p), ("size", u64p), ("heavy_otus", C.c_uint64), ("light_otus", C.c_uint64),
                ("heavy_rows", C.c_uint64), ("light_rows", C.c_uint64), ("variants", C.c_uint64), ("candidates", C.c_uint64), ("confirmed", C.c_uint64), ("bloom_log2", C.c_uint32),
                ("test_passes", C.c_uint32), ("seconds", C.c_double * 5)]


class DenovoParams(C.Structure):   # rtx_denovo_params
    _fields_ = [("segments", C.c_uint32), ("mindelta", C.c_uint32), ("abskew", C.c_uint32), ("max_parents", C.c_uint32), ("flags", C.c_uint32)]


class MergeParams(C.Structure):   # rtx_merge_params
    _fields_ = [("ascii_base", C.c_uint32), ("min_overlap", C.c_uint32), ("max_diffs", C.c_uint32), ("max_diff_pct", C.c_uint32), ("q_cap", C.c_uint32)]


class ChimeraParams(C.Structure):   # rtx_chimera_params
    _fields_ = [("segments", C.c_uint32), ("mindelta", C.c_uint32)]


class ChimeraRec(C.Structure):   # rtx_chimera_rec
    _fields_ = [(f, C.c_uint32) for f in RTX_CHIM_FIELDS]


class DenovoView(C.Structure):   # rtx_denovo_view_t
    _fields_ = [("n_entries", C.c_uint64), ("row", u32p), ("otu", u32p), ("weight", u64p), ("lim", u32p), ("rec", C.POINTER(ChimeraRec)), ("n_checked", C.c_uint64),
                ("n_flagged", C.c_uint64), ("rounds", C.c_uint32), ("scans", C.c_uint64)]


class RtxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libraxtax_hip error {code}: {msg}")
        self.code = code


# every symbol include/raxtax_hip.h declares (tests/test_abi_symbols.py checks the export list)
_SIGNATURES = {
    "rtx_abi_version": (C.c_int, []),
    "rtx_last_error": (C.c_char_p, []),
    "rtx_device_count": (C.c_int, []),
    "rtx_tree_build": (C.c_int, [C.c_uint64, C.c_char_p, u64p, u8p, u64p, C.POINTER(C.c_void_p)]),
    "rtx_tree_build_ex": (C.c_int, [C.c_uint64, C.c_char_p, u64p, u8p, u64p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_tree_parse_reference_fasta": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "rtx_tree_parse_reference_fasta_ex": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_tree_build_kmer_map": (C.c_int, [C.c_void_p]),
    "rtx_tree_save_bin": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rtx_tree_load_bin": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "rtx_tree_destroy": (None, [C.c_void_p]),
    "rtx_tree_num_tips": (C.c_uint64, [C.c_void_p]),
    "rtx_tree_lineage": (C.c_char_p, [C.c_void_p, C.c_uint64]),
    "rtx_tree_original_index": (C.c_uint64, [C.c_void_p, C.c_uint64]),
    "rtx_tree_kmer_csr": (C.c_int, [C.c_void_p, C.POINTER(u64p), C.POINTER(u32p)]),
    "rtx_tree_exact_matches": (C.c_uint64, [C.c_void_p, u8p, C.c_uint64, C.POINTER(u32p)]),
    "rtx_tree_exact_matches_batch": (C.c_uint64, [C.c_void_p, C.c_uint64, u8p, u64p, u64p, u32p, C.c_uint64]),
    "rtx_tree_nodes": (C.c_int, [C.c_void_p, C.POINTER(NodesView)]),
    "rtx_fasta_block_end": (C.c_uint64, [C.c_char_p, C.c_uint64]),
    "rtx_queries_parse_fasta_block": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32,
                                      C.POINTER(C.c_void_p)]),
    "rtx_queries_parse_fasta": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64,
                                          C.POINTER(C.c_void_p)]),
    "rtx_queries_destroy": (None, [C.c_void_p]),
    "rtx_queries_len": (C.c_uint64, [C.c_void_p]),
    "rtx_queries_label": (C.c_char_p, [C.c_void_p, C.c_uint64]),
    "rtx_queries_data": (C.c_int, [C.c_void_p, C.POINTER(u8p), C.POINTER(u64p)]),
    "rtx_index_create": (C.c_int, [C.c_int, C.c_uint64, u64p, u32p, C.c_uint32, u32p, u32p, u32p, u32p, u8p,
                                   C.POINTER(C.c_void_p)]),
    "rtx_index_create_shard": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.c_uint32, u64p, u32p, C.c_uint32,
                                        u32p, u32p, u32p, u32p, u8p, C.POINTER(C.c_void_p)]),
    "rtx_shard_begin": (C.c_int, [C.c_void_p, u32p, u32p]),
    "rtx_shard_count": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rtx_shard_bounds": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rtx_shard_prunes": (C.c_int, [C.c_void_p]),
    "rtx_shard_prob": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rtx_shard_walk": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "rtx_shard_info": (C.c_int, [C.c_void_p, u64p, u64p, u32p, u32p, u32p]),
    "rtx_device_buffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), u64p]),
    "rtx_shard_buffer": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), u64p]),
    "rtx_shard_rehist": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rtx_index_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rtx_index_create_from_sequences": (C.c_int, [C.c_int, C.c_uint64, u8p, u64p, C.c_uint32, u32p, u32p, u32p, u32p, u8p,
                                                 C.POINTER(C.c_void_p)]),
    "rtx_index_create_from_tree": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rtx_index_destroy": (None, [C.c_void_p]),
    "rtx_index_num_refs": (C.c_uint64, [C.c_void_p]),
    "rtx_index_device_bytes": (C.c_uint64, [C.c_void_p]),
    "rtx_index_workspace_bytes": (C.c_uint64, [C.c_void_p]),
    "rtx_index_workspace_parts": (C.c_int, [C.c_void_p, u64p]),
    "rtx_index_set_batch": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rtx_set_default_option": (C.c_int, [C.c_int, C.c_uint64]),
    "rtx_index_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64]),
    "rtx_index_self_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]),
    "rtx_index_prune_verdict": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "rtx_index_run_ahead_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rtx_classify_batch": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u64p, C.c_uint32,
                                     C.POINTER(ResultView)]),
    "rtx_index_has_exact_lookup": (C.c_int, [C.c_void_p]),
    "rtx_batch_exact_matches": (C.c_int, [C.c_void_p, C.POINTER(u64p), C.POINTER(u32p)]),
    "rtx_batch_upload": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u64p]),
    "rtx_batch_run": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rtx_batch_sync": (C.c_int, [C.c_void_p]),
    "rtx_batch_download": (C.c_int, [C.c_void_p, C.POINTER(ResultView)]),
    "rtx_batch_download_then_run": (C.c_int, [C.c_void_p, C.POINTER(ResultView), C.c_uint32]),
    "rtx_index_text_setup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rtx_batch_prefetch_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p)]),
    "rtx_batch_text": (C.c_int, [C.c_void_p, C.POINTER(TextView)]),
    "rtx_batch_stage_times": (C.c_int, [C.c_void_p, f32p, u32p]),
    "rtx_batch_work": (C.c_int, [C.c_void_p, u64p, u64p, u64p]),
    "rtx_batch_prob_work": (C.c_int, [C.c_void_p, u64p, u64p]),
    "rtx_batch_work_split": (C.c_int, [C.c_void_p, u64p, u64p]),
    "rtx_debug_kmers": (C.c_int, [C.c_void_p, C.c_uint64, u16p, u32p]),
    "rtx_debug_hit_counts": (C.c_int, [C.c_void_p, C.c_uint64, u16p]),
    "rtx_debug_prob_table": (C.c_int, [C.c_void_p, C.c_uint64, f64p, f64p]),
    "rtx_debug_pruned_prob_table": (C.c_int, [C.c_void_p, C.c_uint64, f64p, f64p, u32p]),
    "rtx_debug_probs": (C.c_int, [C.c_void_p, C.c_uint64, f64p]),
    "rtx_debug_order": (C.c_int, [C.c_void_p, u32p]),
    "rtx_debug_tile_bounds": (C.c_int, [C.c_void_p, C.c_uint64, u16p]),
    "rtx_debug_prune_stats": (C.c_int, [C.c_void_p, u64p]),
    "rtx_debug_run_counts": (C.c_int, [C.c_void_p, C.c_uint64, u16p, u8p, u32p, u32p, u32p]),
    "rtx_debug_run_mode": (C.c_int, [C.c_void_p, C.c_uint64, u32p]),
    "rtx_batch_last_sub_batch": (C.c_int, [C.c_void_p, u64p, u32p]),
    "rtx_batch_classes": (C.c_int, [C.c_void_p, u32p, u64p]),
    "rtx_debug_prune_detail": (C.c_int, [C.c_void_p, C.c_uint64, u32p]),
    "rtx_debug_evaluate": (C.c_int, [C.c_void_p, f64p, C.POINTER(ResultView)]),
    "rtx_debug_evaluate_mode": (C.c_int, [C.c_void_p, f64p, C.c_uint32, C.POINTER(ResultView), u32p]),
    "rtx_debug_ln_factorial": (C.c_int, [C.c_uint32, f64p]),
    "rtx_debug_prob_hist": (C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint64, C.c_uint32, u16p, u16p, f64p, f64p, f64p, u8p, u32p]),
    "rtx_result_pack": (C.c_int64, [C.POINTER(ResultView), u8p, C.c_uint64]),
    "rtx_records_format": (C.c_int64, [C.c_void_p, u8p, C.c_uint64, C.POINTER(C.c_char_p), u32p, C.c_uint32, C.c_char_p, C.c_uint64, u64p, C.c_uint32]),
    "rtx_format_query": (C.c_int64, [C.c_void_p, C.POINTER(ResultView), C.c_uint64, C.c_char_p, u8p, C.c_uint64,
                                     u32p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64,
                                     C.POINTER(C.c_int64)]),
    "rtx_raxtax": (C.c_int, None),  # argtypes set in api.py (callback type)
    "rtx_raxtax_multi": (C.c_int, None),
    "rtx_raxtax_multi_ex": (C.c_int, None),
    "rtx_batch_strands": (C.c_int, [C.c_void_p, C.POINTER(u8p), C.POINTER(u32p)]),
    "rtx_revcomp": (C.c_int, [u8p, C.c_uint64, u8p]),
    "rtx_raxtax_multi_ex2": (C.c_int, None),
    "rtx_batch_nearest": (C.c_int, [C.c_void_p, C.POINTER(u32p), C.POINTER(u32p)]),
    "rtx_batch_nearest_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "rtx_raxtax_multi_ex3": (C.c_int, None),
    "rtx_batch_identity": (C.c_int, [C.c_void_p, C.POINTER(u32p), C.POINTER(u32p)]),
    "rtx_batch_identity_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "rtx_semiglobal_distance": (C.c_int, [u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint32)]),
    "rtx_index_profile_begin": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rtx_index_profile_read": (C.c_int, [C.c_void_p, C.POINTER(ProfileView)]),
    "rtx_index_profile_reset": (C.c_int, [C.c_void_p]),
    "rtx_index_profile_end": (C.c_int, [C.c_void_p]),
    "rtx_index_profile_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "rtx_profile_merge": (C.c_int, [C.POINTER(C.POINTER(ProfileView)), C.c_uint32, u64p, u64p, u64p, u64p]),
    "rtx_profile_format": (C.c_int64, [C.c_void_p, u64p, u64p, u64p, u64p, C.c_uint32, C.c_char_p, C.c_uint64]),
    "rtx_batch_prefetch_weights": (C.c_int, [C.c_void_p, C.c_uint64, u32p]),
    "rtx_index_profile_begin_samples": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rtx_batch_prefetch_samples": (C.c_int, [C.c_void_p, C.c_uint64, u32p]),
    "rtx_index_profile_read_samples": (C.c_int, [C.c_void_p, C.POINTER(SampleProfileView)]),
    "rtx_sample_profile_merge": (C.c_int, [C.POINTER(C.POINTER(SampleProfileView)), C.c_uint32, u64p, u64p]),
    "rtx_sample_table_format": (C.c_int64, [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), u64p, u64p, C.c_uint32, C.c_char_p, C.c_uint64]),
    "rtx_derep_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "rtx_derep_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, C.POINTER(C.c_uint64)]),
    "rtx_derep_destroy": (None, [C.c_void_p]),
    "rtx_derep_plan": (C.c_int, [C.c_uint64, u32p, u32p, u32p, u32p, C.POINTER(C.c_uint64)]),
    "rtx_raxtax_last_derep": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "rtx_trim_create": (C.c_int, [C.c_int, C.POINTER(TrimPattern), C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_trim_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u32p, u32p]),
    "rtx_trim_destroy": (None, [C.c_void_p]),
    "rtx_trim_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_primer_search": (C.c_int, [u8p, C.c_uint32, u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]),
    "rtx_trim_apply": (C.c_int, [C.c_uint64, u8p, u64p, u32p, u32p, u8p, u64p]),
    "rtx_index_set_primers": (C.c_int, [C.c_void_p, C.POINTER(TrimPattern), C.c_uint32]),
    "rtx_index_primers": (C.c_int, [C.c_void_p, u32p]),
    "rtx_raxtax_last_trim": (C.c_int, [u64p, u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_raxtax_multi_ex4": (C.c_int, None),
    "rtx_demux_create": (C.c_int, [C.c_int, C.POINTER(DemuxTag), C.c_uint32, C.POINTER(DemuxPair), C.c_uint32, C.POINTER(DemuxParams), C.POINTER(C.c_void_p)]),
    "rtx_demux_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u32p, u32p, u32p, u32p]),
    "rtx_demux_destroy": (None, [C.c_void_p]),
    "rtx_demux_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_index_set_tags": (C.c_int, [C.c_void_p, C.POINTER(DemuxTag), C.c_uint32, C.POINTER(DemuxPair), C.c_uint32, C.POINTER(DemuxParams)]),
    "rtx_index_tags": (C.c_int, [C.c_void_p, u32p]),
    "rtx_raxtax_multi_ex7": (C.c_int, None),
    "rtx_raxtax_last_demux": (C.c_int, [u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_demux_read": (C.c_int, [C.POINTER(DemuxParams), C.POINTER(DemuxTag), C.c_uint32, C.POINTER(DemuxPair), C.c_uint32, u8p, C.c_uint64, u32p, u32p, u32p, u32p, u32p]),
    "rtx_queries_parse_fastq": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_fastq_block_end": (C.c_uint64, [C.c_char_p, C.c_uint64]),
    "rtx_queries_parse_fastq_block": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_queries_quals": (C.c_int, [C.c_void_p, C.POINTER(u8p)]),
    "rtx_qual_error_table": (C.c_int, [u64p]),
    "rtx_qual_create": (C.c_int, [C.c_int, C.POINTER(QualParams), C.POINTER(C.c_void_p)]),
    "rtx_qual_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u8p, u64p, u32p, u32p, u32p, u64p, u32p]),
    "rtx_qual_destroy": (None, [C.c_void_p]),
    "rtx_qual_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_qual_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_qual_read": (C.c_int, [C.POINTER(QualParams), u8p, u8p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u64p, u32p]),
    "rtx_index_set_quality": (C.c_int, [C.c_void_p, C.POINTER(QualParams)]),
    "rtx_index_quality": (C.c_int, [C.c_void_p, C.POINTER(QualParams), C.POINTER(C.c_int)]),
    "rtx_raxtax_last_qual": (C.c_int, [u64p, u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_raxtax_multi_ex5": (C.c_int, None),
    "rtx_tally_create": (C.c_int, [C.c_int, C.POINTER(TallyParams), C.POINTER(C.c_void_p)]),
    "rtx_tally_add": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u32p]),
    "rtx_tally_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rtx_tally_info": (C.c_int, [C.c_void_p, u64p, u64p, u64p, u64p, u64p]),
    "rtx_tally_destroy": (None, [C.c_void_p]),
    "rtx_tally_table_create": (C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_tally_table_add": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u32p]),
    "rtx_tally_table_merge": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]),
    "rtx_tally_table_view": (C.c_int, [C.c_void_p, C.POINTER(TallyView)]),
    "rtx_tally_table_destroy": (None, [C.c_void_p]),
    "rtx_tally_format_fasta": (C.c_int64, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_tally_format_table": (C.c_int64, [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_otu_cluster": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(OtuParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_cluster_host": (C.c_int, [C.c_void_p, C.POINTER(OtuParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_view": (C.c_int, [C.c_void_p, C.POINTER(OtuView)]),
    "rtx_otu_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_otu_destroy": (None, [C.c_void_p]),
    "rtx_otu_format_fasta": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_otu_format_table": (C.c_int64, [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_otu_format_map": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "rtx_otu_graft": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(GraftParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_graft_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(GraftParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_graft_view": (C.c_int, [C.c_void_p, C.POINTER(GraftView)]),
    "rtx_otu_format_grafts": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "rtx_otu_unoise": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(UnoiseParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_unoise_host": (C.c_int, [C.c_void_p, C.POINTER(UnoiseParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_unoise_view": (C.c_int, [C.c_void_p, C.POINTER(UnoiseView)]),
    "rtx_otu_format_unoise": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "rtx_otu_taxonomy": (C.c_int, [C.c_int, C.c_uint64, u32p, u64p, C.c_uint64, u32p, C.POINTER(LineageRecords), C.POINTER(NodesView), C.POINTER(OtuTaxonomyParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_taxonomy_host": (C.c_int, [C.c_uint64, u32p, u64p, C.c_uint64, u32p, C.POINTER(LineageRecords), C.POINTER(NodesView), C.POINTER(OtuTaxonomyParams), C.POINTER(C.c_void_p)]),
    "rtx_otu_taxonomy_view": (C.c_int, [C.c_void_p, C.POINTER(OtuTaxonomyView)]),
    "rtx_otu_taxonomy_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_otu_taxonomy_destroy": (None, [C.c_void_p]),
    "rtx_otu_taxonomy_format": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_result_best_lineages": (C.c_int, [C.c_void_p, C.POINTER(ResultView), u32p, u64p, C.c_uint32, C.c_uint32, u8p, u8p, u32p, u8p, C.c_uint32]),
    "rtx_denovo_check": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(DenovoParams), C.POINTER(C.c_void_p)]),
    "rtx_denovo_check_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(DenovoParams), C.POINTER(C.c_void_p)]),
    "rtx_denovo_view": (C.c_int, [C.c_void_p, C.POINTER(DenovoView)]),
    "rtx_denovo_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_denovo_destroy": (None, [C.c_void_p]),
    "rtx_denovo_format_records": (C.c_int64, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "rtx_denovo_format_fasta": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_denovo_format_table": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_uint64]),
    "rtx_index_set_tally": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rtx_index_tally": (C.c_void_p, [C.c_void_p]),
    "rtx_raxtax_last_tally": (C.c_int, [u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_screen_set_build": (C.c_int, [C.c_uint64, u8p, u64p, C.POINTER(C.c_void_p)]),
    "rtx_screen_set_free": (None, [C.c_void_p]),
    "rtx_screen_set_info": (C.c_int, [C.c_void_p, u64p, u64p, u64p, u64p, u64p]),
    "rtx_screen_set_table": (C.c_int, [C.c_void_p, C.POINTER(u32p), u32p]),
    "rtx_screen_create": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(ScreenParams), C.POINTER(C.c_void_p)]),
    "rtx_screen_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u32p, u32p, u32p, u32p, u32p, u32p]),
    "rtx_screen_destroy": (None, [C.c_void_p]),
    "rtx_screen_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_screen_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_screen_read": (C.c_int, [C.c_void_p, C.POINTER(ScreenParams), u8p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p]),
    "rtx_index_set_screen": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ScreenParams)]),
    "rtx_index_screen": (C.c_int, [C.c_void_p, C.POINTER(ScreenParams), C.POINTER(C.c_int), u64p]),
    "rtx_raxtax_multi_ex8": (C.c_int, None),
    "rtx_raxtax_last_screen": (C.c_int, [u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_merge_create": (C.c_int, [C.c_int, C.POINTER(MergeParams), C.POINTER(C.c_void_p)]),
    "rtx_merge_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u8p, u64p, u8p, u8p, u64p, u32p, u32p, u32p, u32p, u64p, u8p, u8p, C.c_uint64]),
    "rtx_merge_destroy": (None, [C.c_void_p]),
    "rtx_merge_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_merge_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "rtx_merge_pair": (C.c_int, [C.POINTER(MergeParams), u8p, u8p, C.c_uint32, u8p, u8p, C.c_uint32, u32p, u32p, u32p, u32p, u8p, u8p]),
    "rtx_merge_queries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_void_p)]),
    "rtx_queries_merge_report": (C.c_int, [C.c_void_p, C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(u32p)]),
    "rtx_fastq_block_end_n": (C.c_uint64, [C.c_char_p, C.c_uint64, C.c_uint64, u64p]),
    "rtx_chimera_create": (C.c_int, [C.c_void_p, C.POINTER(ChimeraParams), C.POINTER(C.c_void_p)]),
    "rtx_chimera_run": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, C.c_void_p]),
    "rtx_chimera_destroy": (None, [C.c_void_p]),
    "rtx_chimera_kernel_time": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rtx_chimera_read": (C.c_int, [C.POINTER(ChimeraParams), u8p, C.c_uint64, u8p, u64p, C.c_uint64, C.c_void_p]),
    "rtx_index_set_chimera": (C.c_int, [C.c_void_p, C.POINTER(ChimeraParams)]),
    "rtx_index_chimera": (C.c_int, [C.c_void_p, C.POINTER(ChimeraParams), C.POINTER(C.c_int)]),
    "rtx_raxtax_multi_ex6": (C.c_int, None),
    "rtx_raxtax_last_chimera": (C.c_int, [u64p, u64p, u64p, C.POINTER(C.c_double)]),
    "rtx_sender_discard": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    "rtx_batch_prefetch": (C.c_int, [C.c_void_p, C.c_uint64, u8p, u64p, u32p, u64p]),
    "rtx_batch_activate": (C.c_int, [C.c_void_p]),
    "rtx_pack_bases": (C.c_int, [u8p, C.c_uint64, u8p]),
    "rtx_batch_sub_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rtx_raxtax_last_timing": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rtx_set_host_share": (C.c_int, [C.c_uint32]),
    "rtx_host_threads": (C.c_uint32, []),
}

_lib = None


def load() -> C.CDLL:
    """Loads libraxtax_hip.so (built by raxtax_amd._build.build_lib / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m raxtax_amd._build` (hipcc, gfx950). "
            "raxtax_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process do not both see the GPU.
    # Importing torch first makes libraxtax_hip.so resolve to the runtime that is already loaded, so the
    # library and torch.distributed (RCCL) share one (bench.py, raxtax_amd/sharded.py).  Optional.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement of the library
        pass
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        if args is not None:
            fn.argtypes = args
    _lib = lib
    return lib


def check(code: int):
    if code < 0:
        raise RtxError(code, load().rtx_last_error().decode(errors="replace"))
    return code


def ptr(a: np.ndarray, typ):
    return a.ctypes.data_as(typ)

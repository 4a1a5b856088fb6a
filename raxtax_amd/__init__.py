"""raxtax_amd -- MI355X (gfx950) implementation of raxtax's per-query k-mer classification
hot path behind a C ABI (include/raxtax_hip.h).  See DESIGN.md."""
import os as _os

# hardware queues of the HIP runtime (read when it initialises; csrc/host_threads.cpp says why the library wants more than the default four):
# asked for here too, in case the process initialises HIP (torch.cuda ...) between this import and the loading of the library
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from .api import (EvaluationResult, Index, Result, Tree, parse_query_fasta_str, parse_reference_fasta_str,  # noqa: F401
                  raxtax, raxtax_last_timing, NO_REF, NO_DIST, semiglobal_distance, Profile, profile_merge, profile_text, SampleProfile, sample_profile_merge, sample_table_text, Derep, derep_plan, raxtax_last_derep,
                  Tally, TallyTable, tally_reads, tally_merge, tally_fasta, tally_table_text, raxtax_last_tally, Otus, otu_cluster, otu_cluster_host, otu_fasta, otu_table_text, otu_map_text, otu_graft, otu_graft_host, otu_grafts_text, UnoiseParams, otu_unoise, otu_unoise_host, unoise_text, DenovoParams, Denovo, denovo_check, denovo_check_host, denovo_records_text, denovo_fasta, denovo_table_text, Lineages, best_lineages, OtuTaxonomy, otu_taxonomy, otu_taxonomy_host,
                  Trim, TrimPrimer, primer_patterns, primer_search, trim_apply, trim_hit, encode_iupac, raxtax_last_trim, TRIM_5P, TRIM_3P, TRIM_NO_PATTERN,
                  Demux, DemuxTag, DemuxParams, demux_read, demux_hit, demux_verdict_names, sample_sheet, raxtax_last_demux, DEMUX_NO_TAG, DEMUX_NONE,
                  DEMUX_OK, DEMUX_NO_TAG5, DEMUX_NO_TAG3, DEMUX_AMBIGUOUS, DEMUX_UNKNOWN_PAIR,
                  parse_query_fastq_str, Qual, QualParams, qual_read, qual_error_table, qual_verdict_names, raxtax_last_qual, QUAL_MAX_READ,
                  QC_BAD_QUALITY, QC_SHORT_FOR_TRUNC_LEN, QC_TOO_SHORT, QC_TOO_LONG, QC_TOO_MANY_N, QC_MAX_EE, QC_MAX_EE_RATE,
                  Merge, MergeParams, merge_pair, merge_queries, merge_verdict_names, fastq_text, fastq_block_end_n, MERGE_MAX_READ,
                  MG_BAD_QUALITY, MG_TOO_LONG, MG_TOO_SHORT, MG_NO_OVERLAP,
                  Screen, ScreenSet, ScreenParams, screen_read, raxtax_last_screen, SCREEN_K, SCREEN_NONE, SCREEN_MAX_READ, SCREEN_MAX_BASES, SCREEN_CONTAMINANT,
                  Chimera, ChimeraParams, chimera_read, raxtax_last_chimera, CHIMERA_DTYPE, CHIMERA_MAX_QUERY, CHIM_OK, CHIM_NO_KMER, CHIM_TOO_LONG)
from ._lib import (RTX_RAW_CONFIDENCE, RTX_SKIP_EXACT_MATCHES, RtxError)  # noqa: F401

__all__ = ["Tree", "Index", "Result", "EvaluationResult", "raxtax", "raxtax_last_timing", "parse_reference_fasta_str",
           "parse_query_fasta_str", "RtxError", "RTX_SKIP_EXACT_MATCHES", "RTX_RAW_CONFIDENCE", "NO_REF", "NO_DIST", "semiglobal_distance",
           "Profile", "profile_merge", "profile_text", "SampleProfile", "sample_profile_merge", "sample_table_text", "Derep", "derep_plan", "raxtax_last_derep",
           "Tally", "TallyTable", "tally_reads", "tally_merge", "tally_fasta", "tally_table_text", "raxtax_last_tally", "Otus", "otu_cluster", "otu_cluster_host", "otu_fasta", "otu_table_text", "otu_map_text", "otu_graft", "otu_graft_host", "otu_grafts_text", "UnoiseParams", "otu_unoise", "otu_unoise_host", "unoise_text", "DenovoParams", "Denovo", "denovo_check", "denovo_check_host", "denovo_records_text", "denovo_fasta", "denovo_table_text", "Lineages", "best_lineages", "OtuTaxonomy", "otu_taxonomy", "otu_taxonomy_host",
           "Trim", "TrimPrimer", "primer_patterns", "primer_search", "trim_apply", "trim_hit", "encode_iupac", "raxtax_last_trim", "TRIM_5P", "TRIM_3P",
           "TRIM_NO_PATTERN", "Demux", "DemuxTag", "DemuxParams", "demux_read", "demux_hit", "demux_verdict_names", "sample_sheet", "raxtax_last_demux", "DEMUX_NO_TAG",
           "DEMUX_NONE", "DEMUX_OK", "DEMUX_NO_TAG5", "DEMUX_NO_TAG3", "DEMUX_AMBIGUOUS", "DEMUX_UNKNOWN_PAIR", "parse_query_fastq_str", "Qual", "QualParams", "qual_read", "qual_error_table", "qual_verdict_names", "raxtax_last_qual",
           "QUAL_MAX_READ", "QC_BAD_QUALITY", "QC_SHORT_FOR_TRUNC_LEN", "QC_TOO_SHORT", "QC_TOO_LONG", "QC_TOO_MANY_N", "QC_MAX_EE", "QC_MAX_EE_RATE",
           "Merge", "MergeParams", "merge_pair", "merge_queries", "merge_verdict_names", "fastq_text", "fastq_block_end_n", "MERGE_MAX_READ",
           "MG_BAD_QUALITY", "MG_TOO_LONG", "MG_TOO_SHORT", "MG_NO_OVERLAP",
           "Screen", "ScreenSet", "ScreenParams", "screen_read", "raxtax_last_screen", "SCREEN_K", "SCREEN_NONE", "SCREEN_MAX_READ", "SCREEN_MAX_BASES", "SCREEN_CONTAMINANT",
           "Chimera", "ChimeraParams", "chimera_read", "raxtax_last_chimera", "CHIMERA_DTYPE", "CHIMERA_MAX_QUERY", "CHIM_OK", "CHIM_NO_KMER", "CHIM_TOO_LONG"]

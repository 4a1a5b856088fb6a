/*
 * raxtax_hip.h -- C ABI of libraxtax_hip.so, the MI355X (gfx950) drop-in for the
 * per-query k-mer classification hot path of noahares/raxtax v1.5.0.
 *
 * The reference has no FFI or plugin interface: its seam is the Rust function
 *     raxtax(queries, tree, skip_exact_matches, raw_confidence, chunk_size, sender, tsv)
 * (src/raxtax.rs:14-22, called once from src/main.rs:137-145).  The entry points
 * below are what a Rust `extern "C"` block for that seam binds (INTEGRATION.md
 * shows the binding).  Plain pointers and sizes only; every function returns an
 * int status (RTX_OK or a negative RTX_ERR_*); `rtx_last_error()` returns a
 * message for the calling thread.  The caller owns every host buffer it passes
 * in; the library owns all device memory and every buffer it hands out through
 * a view (valid until the next call on the same handle, or its destruction).
 * One handle per GPU; calls on one handle must be serialised by the caller;
 * distinct handles may be driven from distinct host threads.
 *
 * There is NO CPU fallback: every rtx_index_* / rtx_batch_* / rtx_classify_*
 * call fails with RTX_ERR_NO_DEVICE when no gfx950 device is usable.
 *
 * Sequences are passed as the reference stores them: one byte per base, 4-bit
 * one-hot codes A=1 C=2 G=4 T=8, ambiguity codes = unions (src/parser.rs:11-34).
 * Reference ids are indices into the lineage-sorted order of Tree::new
 * (src/tree.rs:53-54), i.e. indices into `tree.lineages`.
 */
#ifndef RAXTAX_HIP_H
#define RAXTAX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 6 /* 2: rtx_result_view.row_begin/row_count replace row_off; 3: exact_off == NULL = look the exact matches up on the device;
                             4: RTX_NUM_STAGES 8 -> 10 (rtx_batch_stage_times writes ten entries), rtx_batch_prefetch / rtx_batch_activate;
                             5: rtx_result_view grows row_conf_stride, row_depth_u8, row_conf_hundredths (the rows are finalised on the device and
                                arrive in their final layout: row_conf is [n_rows][row_conf_stride], no longer [n_rows][RTX_MAX_DEPTH]); the exports
                                and options of round 5 (rtx_index_self_sample, rtx_records_format, options 18-22);
                             6: RTX_OPT_RUN_AHEAD (23), RTX_RETRY_CHUNK from rtx_batch_download_then_run under it, rtx_index_run_ahead_stats
                                (still 6 with RTX_OPT_NEAREST (26), RTX_NO_REF, rtx_batch_nearest and rtx_raxtax_multi_ex2: exports and an option
                                that is off by default, nothing that exists changes shape; and with the taxon profile, rtx_index_profile_* /
                                rtx_profile_merge / rtx_profile_format: exports only; and with RTX_OPT_DEREP (27), rtx_derep_*,
                                rtx_batch_prefetch_weights and rtx_raxtax_last_derep: exports and an option that is off by default; and with
                                RTX_OPT_IDENTITY (28), RTX_NO_DIST, rtx_batch_identity, rtx_semiglobal_distance and rtx_raxtax_multi_ex3: the same;
                                and with primer trimming, rtx_trim_* / rtx_primer_search / rtx_index_set_primers / rtx_raxtax_last_trim /
                                rtx_raxtax_multi_ex4: exports and a setting that is off by default; and with FASTQ and the quality filter,
                                rtx_queries_parse_fastq* / rtx_fastq_block_end / rtx_queries_quals / rtx_qual_* / rtx_index_set_quality /
                                rtx_raxtax_last_qual / rtx_raxtax_multi_ex5: the same; and with paired-end merging, rtx_merge_* /
                                rtx_queries_merge_report / rtx_fastq_block_end_n: exports only; and with the chimera check, rtx_chimera_* /
                                rtx_index_set_chimera / rtx_index_chimera / rtx_raxtax_last_chimera / rtx_raxtax_multi_ex6: exports and a
                                setting that is off by default; and with sample demultiplexing, rtx_demux_* / rtx_index_set_tags /
                                rtx_index_tags / rtx_raxtax_last_demux / rtx_raxtax_multi_ex7 and the per-sample counters
                                rtx_index_profile_begin_samples / _read_samples / rtx_batch_prefetch_samples / rtx_sample_profile_merge /
                                rtx_sample_table_format: the same; and with the contaminant screen, rtx_screen_* / rtx_index_set_screen /
                                rtx_index_screen / rtx_raxtax_last_screen / rtx_raxtax_multi_ex8: the same; and with the de novo chimera check of a
                                run, rtx_denovo_*: exports only; and with the consensus taxonomy of the OTUs, rtx_otu_taxonomy* /
                                rtx_result_best_lineages: exports only; and with denoising, rtx_otu_unoise* / rtx_otu_format_unoise: exports
                                only) */
#define RTX_NUM_KMERS 65536u /* 2 << 15 posting lists, src/tree.rs:52 */
#define RTX_MAX_DEPTH 32u    /* deepest lineage (comma-separated levels) the device walk carries */

/* status codes */
#define RTX_OK 0
#define RTX_ERR_INVALID (-1)    /* bad argument / malformed input arrays            */
#define RTX_ERR_HIP (-2)        /* HIP runtime error (see rtx_last_error)           */
#define RTX_ERR_NO_DEVICE (-3)  /* no usable gfx950 device                          */
#define RTX_ERR_OOM (-4)        /* host or device allocation failed                 */
#define RTX_ERR_PARSE (-5)      /* FASTA / lineage annotation error (parser.rs)     */
#define RTX_ERR_DEPTH (-6)      /* lineage deeper than RTX_MAX_DEPTH: refused by rtx_tree_build* / _parse* / _load_bin, the lineage named in rtx_last_error */
#define RTX_ERR_STATE (-7)      /* call sequence violated (e.g. run before upload)  */
#define RTX_ERR_TOO_LONG (-8)   /* the memoised probability tables were demanded (RTX_OPT_PROB_MODE = 2) for a read they do not cover.  (Until ABI 4 also: a
                                   query longer than 65 542 bases.  The reference asserts on DISTINCT k-mers, raxtax.rs:56, and serves such reads: so does
                                   the library now -- per query, RTX_Q_ALL_KMERS for a read that really holds all 65 536 of them) */
#define RTX_ERR_SENDER (-9)     /* the result sink refused a message (closed channel, raxtax.rs:87)    */
#define RTX_RETRY_CHUNK 1        /* not an error: rtx_batch_download_then_run under RTX_OPT_RUN_AHEAD found the batch being downloaded short of buffer space
                                   AFTER it had enqueued the next one; both have been taken off the handle (buffers grown): run this batch again
                                   (upload, run, download) and stage the next one anew */

/* flags of rtx_classify_batch / rtx_batch_run (src/io.rs:119-121,131-133) */
#define RTX_SKIP_EXACT_MATCHES 1u /* zero the hit counts of exact matches, raxtax.rs:65-68 */
#define RTX_RAW_CONFIDENCE 2u     /* host mirror only: suppress the single-exact-match override, raxtax.rs:73-84 */
#define RTX_TEXT_TSV 4u           /* rtx_index_text_setup only: the `.tsv` lines as well (lineage.rs:31-48) */

/* per-query status in rtx_result_view.status */
#define RTX_Q_OK 0
#define RTX_Q_NO_KMERS 1 /* t == 0, or t == 1 without a full-overlap reference: the reference
                            panics here (prob.rs:21 u64 underflow / prob.rs:162 zip_eq); the
                            library reports the query instead of aborting -- deliberate divergence */

#define RTX_Q_ALL_KMERS 2 /* t == 65 536: the read holds every 8-mer (only reads of 65 543 bases or more can).  The reference
                            asserts that t fits a u16 (raxtax.rs:56) and aborts the run; the library reports this query, returns
                            no rows for it (t = 65 536 in the view) and classifies the rest of the batch */

typedef struct rtx_tree rtx_tree;   /* host mirror of `Tree` (src/tree.rs:36-43)          */
typedef struct rtx_index rtx_index; /* device-resident index + per-GPU batch workspace    */

/* ------------------------------------------------------------------------- */
/* diagnostics                                                                */
/* ------------------------------------------------------------------------- */
int rtx_abi_version(void);
const char *rtx_last_error(void);
int rtx_device_count(void); /* number of visible HIP devices, 0 if none / no driver */

/* ------------------------------------------------------------------------- */
/* Host mirror of the index build (plumbing around the hot path)             */
/* ------------------------------------------------------------------------- */
/* Tree::new(lineages, sequences), src/tree.rs:46-140.  Lineage i is the byte
 * range lineage_bytes[lineage_off[i] .. lineage_off[i+1]) (no terminator);
 * sequence i is seq_bytes[seq_off[i] .. seq_off[i+1]). */
int rtx_tree_build(uint64_t n, const char *lineage_bytes, const uint64_t *lineage_off,
                   const uint8_t *seq_bytes, const uint64_t *seq_off, rtx_tree **out);
/* The same with options.  RTX_TREE_SKIP_KMER_MAP: sort, taxonomy and exact-sequence map only; the k-mer
 * index is then built on the GPU from the sequences by rtx_index_create_from_tree. */
#define RTX_TREE_SKIP_KMER_MAP 1u
int rtx_tree_build_ex(uint64_t n, const char *lineage_bytes, const uint64_t *lineage_off,
                      const uint8_t *seq_bytes, const uint64_t *seq_off, uint32_t flags, rtx_tree **out);
/* parse_reference_fasta_str, src/parser.rs:46-105 */
int rtx_tree_parse_reference_fasta(const char *text, uint64_t len, rtx_tree **out);
/* The same with RTX_TREE_* flags: RTX_TREE_SKIP_KMER_MAP leaves Tree.k_mer_map unbuilt (rtx_index_create_from_tree
 * then builds the bitmaps on the GPU from the sequences); rtx_tree_build_kmer_map builds it later, e.g. on a
 * background thread for the `.bin` cache while queries are already being classified.  Both parsers cut the text
 * at header lines and parse the pieces on several threads. */
int rtx_tree_parse_reference_fasta_ex(const char *text, uint64_t len, uint32_t flags, rtx_tree **out);
int rtx_tree_build_kmer_map(rtx_tree *tree);
/* Tree::save_to_file / Tree::load_from_file (src/tree.rs:147-164): the reference's `.bin` database,
 * bincode 1.3.3 default options.  Files written here are readable by upstream raxtax and vice versa. */
int rtx_tree_save_bin(const rtx_tree *tree, const char *path);
int rtx_tree_load_bin(const char *path, rtx_tree **out);
void rtx_tree_destroy(rtx_tree *tree);
uint64_t rtx_tree_num_tips(const rtx_tree *tree);                  /* Tree.num_tips      */
const char *rtx_tree_lineage(const rtx_tree *tree, uint64_t i);    /* Tree.lineages[i]   */
uint64_t rtx_tree_original_index(const rtx_tree *tree, uint64_t i);/* sorted -> input idx */
/* Tree.k_mer_map as CSR: offsets[65537], postings sorted-unique per list (tree.rs:134-137) */
int rtx_tree_kmer_csr(const rtx_tree *tree, const uint64_t **offsets, const uint32_t **postings);
/* Tree.sequences.get(seq), src/raxtax.rs:42.  Returns the number of ids. */
uint64_t rtx_tree_exact_matches(const rtx_tree *tree, const uint8_t *seq, uint64_t len,
                                const uint32_t **ids);
/* The same lookup for a batch: fills exact_off[n_queries+1] and up to ids_cap ids; returns the
 * total number of ids (call again with a larger buffer if it exceeds ids_cap). */
uint64_t rtx_tree_exact_matches_batch(const rtx_tree *tree, uint64_t n_queries, const uint8_t *bases,
                                      const uint64_t *base_off, uint64_t *exact_off, uint32_t *exact_ids,
                                      uint64_t ids_cap);
/* Flattened taxonomy: nodes in breadth-first order (root = node 0, the children of a node
 * are consecutive), childless Sequence nodes (tree.rs:102-107) dropped -- they never
 * influence Lineage::evaluate.  node_begin/end = Node.confidence_range (tree.rs:190). */
typedef struct {
    uint32_t n_nodes;
    const uint32_t *node_begin;
    const uint32_t *node_end;
    const uint32_t *node_first_child;
    const uint32_t *node_n_children;
    const uint32_t *node_parent; /* 0xFFFFFFFF for the root */
    const uint8_t *node_type;    /* 0 Inner, 1 Taxon, 2 Sequence (tree.rs:181-186) */
} rtx_nodes_view;
int rtx_tree_nodes(const rtx_tree *tree, rtx_nodes_view *out);

/* parse_query_fasta_str, src/parser.rs:117-154.  Returns a handle holding labels and
 * encoded sequences; `skip` labels (already-processed queries, parser.rs:150-153) are dropped. */
typedef struct rtx_queries rtx_queries;
int rtx_queries_parse_fasta(const char *text, uint64_t len, const char *const *skip, uint64_t n_skip,
                            rtx_queries **out);
/* The same for one block of a file that is read piecewise (FASTA ingest of very large query files: the reference
 * reads the whole file, parser.rs:112-115).  Blocks must be cut in front of a header line: rtx_fasta_block_end returns
 * the offset of the last '>' that directly follows a newline (0 if there is none) -- parse text[0, end) with
 * RTX_FASTA_MORE_FOLLOWS and carry text[end, len) over to the next block; every block but the first also gets
 * RTX_FASTA_NOT_FIRST.  The records of all blocks together are exactly those of the whole-file parse. */
#define RTX_FASTA_MORE_FOLLOWS 1u /* not the last block: a trailing header without bases is dropped (the next header replaces it) */
#define RTX_FASTA_NOT_FIRST 2u    /* not the first block: it starts with a header by construction */
uint64_t rtx_fasta_block_end(const char *text, uint64_t len);
int rtx_queries_parse_fasta_block(const char *text, uint64_t len, const char *const *skip, uint64_t n_skip, uint32_t flags,
                                  rtx_queries **out);
void rtx_queries_destroy(rtx_queries *q);
uint64_t rtx_queries_len(const rtx_queries *q);
const char *rtx_queries_label(const rtx_queries *q, uint64_t i);
/* all sequences concatenated + n+1 offsets (the layout rtx_classify_batch takes) */
int rtx_queries_data(const rtx_queries *q, const uint8_t **bases, const uint64_t **base_off);
/* FASTQ (what a sequencer emits) in the four-line record form only: `@header`, the sequence, `+` followed by anything, the quality string of
 * the sequence's length; `\r\n` line ends are tolerated, the last record may lack its final newline, blank lines may only follow the last
 * record.  The label is derived from the header line and the bases are encoded as rtx_queries_parse_fasta does it (lower case and IUPAC
 * included), `skip` labels are dropped likewise; a record without bases is kept (the empty read).  ascii_base (33 or 64) is only checked
 * against: every quality byte must lie in 33 .. 126.  RTX_ERR_PARSE, with the number of the record (from 1, within the text given) in
 * rtx_last_error: a first line that does not start with '@', a third line that does not start with '+', a quality string of another length
 * than the sequence, a quality byte outside 33 .. 126, a character that is no base, and a record that is cut short.
 * A quality line may itself start with '@', so a block of a file that is read piecewise cannot be cut at "\n@": rtx_fastq_block_end returns
 * the offset behind the last complete group of four lines counted from the start of the text (0 if there is none) -- every block starts at
 * a record; parse text[0, end) and carry text[end, len) over, flags as for FASTA (a record cut short is an error in every block).  The
 * records of all blocks together are exactly those of the whole-file parse.
 * rtx_queries_quals: the quality bytes as they stand in the file (ASCII, the base not taken off), concatenated and indexed by the base_off
 * of rtx_queries_data; NULL for the handle of a FASTA parse. */
int rtx_queries_parse_fastq(const char *text, uint64_t len, const char *const *skip, uint64_t n_skip, uint32_t ascii_base, rtx_queries **out);
uint64_t rtx_fastq_block_end(const char *text, uint64_t len);
int rtx_queries_parse_fastq_block(const char *text, uint64_t len, const char *const *skip, uint64_t n_skip, uint32_t ascii_base, uint32_t flags,
                                  rtx_queries **out);
int rtx_queries_quals(const rtx_queries *q, const uint8_t **quals);

/* ------------------------------------------------------------------------- */
/* Device index (replaces the read-only `&Tree` argument of raxtax())        */
/* ------------------------------------------------------------------------- */
/* Uploads Tree.k_mer_map (CSR, lists sorted-unique) and the flattened taxonomy
 * (as rtx_nodes_view) to GPU `device`; the library re-encodes the postings into
 * its own HBM layout (per-k-mer reference bitmaps).  n_refs = Tree.num_tips. */
int rtx_index_create(int device, uint64_t n_refs, const uint64_t *offsets /*65537*/,
                     const uint32_t *postings, uint32_t n_nodes, const uint32_t *node_begin,
                     const uint32_t *node_end, const uint32_t *node_first_child,
                     const uint32_t *node_n_children, const uint8_t *node_type, rtx_index **out);
/* One shard of a reference-sharded database (BASELINE.json configs[4]): the handle holds the bitmaps of
 * references [ref_lo, ref_hi) only; offsets/postings and the taxonomy are those of the WHOLE database
 * (global ids).  shard_cuts lists the boundaries of all shards (every rank passes the same list) so that
 * the taxonomy boundary numbering is identical on every rank.  Such a handle is driven with
 * rtx_shard_begin / _count / _prob / _walk (below) instead of rtx_batch_run. */
int rtx_index_create_shard(int device, uint64_t n_refs_total, uint64_t ref_lo, uint64_t ref_hi,
                           const uint64_t *shard_cuts, uint32_t n_cuts, const uint64_t *offsets,
                           const uint32_t *postings, uint32_t n_nodes, const uint32_t *node_begin,
                           const uint32_t *node_end, const uint32_t *node_first_child,
                           const uint32_t *node_n_children, const uint8_t *node_type, rtx_index **out);
/* Index build on the GPU (the k-mer part of Tree::new, src/tree.rs:114-123,134-137): the encoded
 * reference sequences in lineage-sorted order (sequence i = reference id i) instead of posting lists. */
int rtx_index_create_from_sequences(int device, uint64_t n_refs, const uint8_t *seq_bytes, const uint64_t *seq_off,
                                    uint32_t n_nodes, const uint32_t *node_begin, const uint32_t *node_end,
                                    const uint32_t *node_first_child, const uint32_t *node_n_children,
                                    const uint8_t *node_type, rtx_index **out);
/* Convenience: the same from a host tree (GPU build if the tree has no k-mer map). */
int rtx_index_create_from_tree(int device, const rtx_tree *tree, rtx_index **out);
void rtx_index_destroy(rtx_index *index);
uint64_t rtx_index_num_refs(const rtx_index *index);
uint64_t rtx_index_device_bytes(const rtx_index *index); /* HBM held by the index itself */
uint64_t rtx_index_workspace_bytes(const rtx_index *index); /* ... and by everything else of the handle as of the last upload: probability tables, the scratch
                                                               sets of a sub-batch, inputs, result arena and final result arrays (ABI 5) */
/* ... in parts (bytes): [0] probability tables, [1] counts, [2] record segments, [3] boundary prefix sums, [4] per-tile masks and sparse-slot lists,
 * [5] the rest of the scratch sets, [6] inputs and processing order, [7] result arena and final arrays; [8] = scratch sets in use */
int rtx_index_workspace_parts(const rtx_index *index, uint64_t out[9]);
/* queries processed per kernel wave (sub-batch); 0 = choose from free HBM */
int rtx_index_set_batch(rtx_index *index, uint32_t sub_batch);
/* Tuning / test knobs.  RTX_OPT_PROB_MODE: 0 = auto (memoised cmf tables when every query has
 * t <= 1023 and they fit in HBM, else the per-query recurrence kernel), 1 = recurrence only,
 * 2 = tables only (error if unavailable).  Both produce the same probabilities to ~1e-13. */
#define RTX_OPT_SUB_BATCH 1
#define RTX_OPT_PROB_MODE 2
#define RTX_OPT_STAGE_TIMING 6 /* 0 (default): HIP events around hit_count only; 1: around every kernel
                                 (rtx_batch_stage_times then reports all stages; adds ~1 ms per 100k queries) */
#define RTX_OPT_DEBUG_TAPS 14 /* 0 (default); 1: prune_kernel keeps its view of every query of a sub-batch for rtx_debug_prune_detail (tests) */
#define RTX_OPT_DEVICE_EXACT 15 /* 1 (default): a batch uploaded WITHOUT exact-match ids (exact_off == NULL) has them looked up on the device
                                 * (a hash table of the distinct reference sequences, every candidate verified byte by byte; rtx_exact.hip)
                                 * as part of rtx_batch_run -- Tree.sequences.get, raxtax.rs:42 -- when the handle was built from the
                                 * sequences (rtx_index_create_from_tree / _from_sequences); rtx_batch_exact_matches returns the ids.
                                 * 0: such a batch has no exact matches (the behaviour of ABI version 2) */
#define RTX_OPT_CLUSTER 7 /* 1 (default): the queries of a batch are processed in an order that puts related
                             queries next to each other (min-hash sketches, rtx_cluster.hip) so that bitmap rows
                             are reused; 0: input order.  Results are identical and always in input order. */
#define RTX_OPT_PACKED_COUNTS 8 /* 1 (default): with t <= 1023 the hit counts travel from hit_count to taxon_prefix
                                 * packed, 10 bits per reference (low byte + 2 high bits); 0: as u16 (A/B measurements) */
#define RTX_OPT_HIT_PAIR 11 /* 1 (default): with t <= 1023 and RTX_OPT_CLUSTER on, hit_count runs two neighbouring queries per wave (two
                             * sets of bit planes in registers) and loads the bitmap rows they share once (rtx_hit_pair.hip);
                             * identical results; 0: one query per wave (the kernel of longer queries; A/B measurements) */
#define RTX_OPT_TILE_SKIP 10 /* 1 (default): hit_count records the largest count of every tile of 8192 references and
                              * taxon_prefix (lineage.rs:61-66) reads only the tiles that hold a reference whose probability
                              * reaches 1e-30 -- the others add less than n_refs * 1e-30 to any prefix sum, far below what a
                              * confidence (rounded to 1e-2) can show; 0: every reference is summed (A/B measurements) */
#define RTX_OPT_LOCATOR 12 /* 1 (default): when the handle was built from the reference sequences (rtx_index_create_from_sequences /
                            * _from_tree) the processing order of RTX_OPT_CLUSTER is led by the query's position in the
                            * lineage-ordered database (a vote of its 12-mers in a table built from the references), the
                            * min-hashes only break ties; 0: min-hash order alone.  Scheduling only: results are identical */
#define RTX_OPT_TILE_PRUNE 13 /* 1 (default): hit_count counts only the tiles of 8192 references that can hold a reference with any
                               * probability -- decided from upper bounds (the queries counted against a union bitmap over blocks
                               * of 64 references) and a per-query threshold u: the references with a count up to u hold less
                               * than 1e-10 of probability together and are treated as references without a hit (rtx_prune.hip;
                               * every probability and confidence sum stays within 1e-9 of the full count -- measured 1e-11 --,
                               * the result of a query does not depend on the rest of the batch).  Takes effect with t <= 1023,
                               * RTX_OPT_HIT_PAIR = 1, RTX_OPT_TILE_SKIP = 1, the whole database on the handle and 4 tiles or more;
                               * the debug taps recount the tapped sub-batch in full.  0: every tile is counted */
#define RTX_OPT_FINE_BOUNDS 17 /* 1 (default): second stage of the bounds of the tile pruning on databases of 16 tiles or more: the pairs of
                                * queries that the bounds over blocks of 64 references leave 4 or more live tiles are counted against a
                                * second union bitmap over blocks of 8 references (1/8 of the index), which takes the tiles without a block
                                * above the query's threshold off their lists before the counting pass.  Results do not change (a bound is a
                                * bound); 0: first stage only (A/B measurements) */
#define RTX_OPT_RECORDS 18 /* 4 (default; 0 .. 16): the RECORDS path of the tile pruning.  A query that the pruning gives a threshold and at most
                            * this many live tiles only ever needs its references with a count ABOVE the threshold (every other one is a
                            * reference without a hit): the epilogue of hit_count then writes (reference, count) records of those alone instead
                            * of the counts of 8192 references per tile, and one wave per query turns them into the prefix sums of
                            * lineage.rs:61-77 at the few taxonomy boundaries they touch and walks the lineage (rtx_records.hip) in the place
                            * of taxon_prefix's sweeps.  Same thresholds, same probabilities; 0: every query takes the dense epilogue.
                            * Shapes the workspace like the options below. */
#define RTX_OPT_OVERLAP 19 /* 1 (default): the back half of sub-batch k (prob_lookup, taxon_prefix + walk, records tail: chains of dependent round
                            * trips) runs on a second HIP stream beside the front half of sub-batch k + 1 (bounds, counting: VALU and L1
                            * rate); two scratch sets alternate -- taken only if the second one fits free HBM without shrinking the sub-batch.
                            * 2: three stages (bounds | threshold + counting | back half; measured: no faster than two).  0: one stream.
                            * Same results.  Whole-database handles whose batch is on the pruned path (where every tile is counted the second
                            * stream costs more than it hides), one handle per device (handles that rtx_raxtax_multi drives side by side on
                            * ONE device keep to one stream and one scratch set: two sets are ~120 GB at 500 000 references); shapes the workspace. */
#define RTX_OPT_MIN_SUB_BATCHES 20 /* 4 (default; 1 .. 64): a batch on the pruned path is cut into at least this many sub-batches (of 16 384 queries or
                                    * more), so that the host finalises the records of one while the next ones run and only the last one is left
                                    * when the device is done.  rtx_raxtax sets 2 for the time of a call: its chunks follow one another through
                                    * rtx_batch_download_then_run, which hides the last sub-batch of a chunk behind the next chunk.  Shapes the workspace. */
#define RTX_OPT_TWO_LEVEL_BOUNDS 21 /* 1 (default): the bounds pass of the tile pruning on a whole-database handle runs in two levels
                                     * (rtx_bounds2.hip): union bounds over blocks of 256 references for every tile -- four rows of that
                                     * bitmap per load instruction --, and over blocks of 64 only for the groups of four tiles whose
                                     * coarse bound comes close to the query's largest (sixteen rows per load instruction).  Every tile
                                     * keeps a valid upper bound either way: results differ from the one-level pass only through which
                                     * tiles are proven dead before counting (a function of the query alone).  0: the one-level pass
                                     * over blocks of 64 (reference shards always use it).  Values above 1 set the rule that picks the
                                     * refined groups (experiments): c_t | c_m << 16 | lo << 32 | hi << 48, in 1/256 of t. */
#define RTX_OPT_PRUNE_SELF_SAMPLE 22 /* 1 (default): the handle honours the verdict of rtx_index_self_sample (taken when the handle is created
                                      * from the reference sequences or from a tree): on a database whose own references keep 85 % or more
                                      * of its tiles live -- every tile holds relatives of every query: real barcodes of one order -- tile
                                      * pruning stays off whatever RTX_OPT_TILE_PRUNE says (bounds and thresholds would cost more than they
                                      * save).  0: RTX_OPT_TILE_PRUNE alone decides.  Shapes the workspace like RTX_OPT_TILE_PRUNE */
#define RTX_OPT_RUN_AHEAD 23         /* 0 (default).  1: rtx_batch_download_then_run enqueues the staged batch BEFORE the last sub-batch of the batch
                                      * being downloaded has finished: the front half of the next batch's first sub-batch runs beside the back
                                      * half of this batch's last one (RTX_OPT_OVERLAP's two streams never drain between the chunks of a file).
                                      * The result state of a batch then exists twice on the device.  The call may return RTX_RETRY_CHUNK (see
                                      * there); a run under this option leaves the handle's stream NOT covering its back halves until the next
                                      * call that needs it (rtx_batch_sync, a download, the next run, switching the option off).  rtx_raxtax sets
                                      * it for the duration of a call with more than one chunk.  Results are those of the plain sequence.  (2: a test aid -- every
                                      * second run-ahead is abandoned as if the batch had overflowed.) */
#define RTX_OPT_DEVICE_TEXT 24       /* 0 (default).  1: rtx_raxtax / rtx_raxtax_multi take the `.out` / `.tsv` text of their chunks from the device
                                      * (rtx_batch_text: the call sets the text up for its tree and flags and stages the labels with every chunk);
                                      * the format stage keeps only the lineage check of raxtax.rs:43-53.  The messages are the same either way. */
#define RTX_OPT_STRAND 25            /* 0 (default): every query is classified in the orientation it is given, as the reference does.  1: BOTH STRANDS -- when a
                                      * batch becomes the current one the handle appends the reverse complement of every query on the device (the sequence
                                      * reversed, the four bits of every one-hot code reversed: A <-> T, C <-> G, ambiguity codes to their complements, a byte
                                      * above 15 stays), classifies both and keeps, per query, the orientation with the larger PEAK -- the largest hit count
                                      * over the references, after RTX_SKIP_EXACT_MATCHES has zeroed the exact matches of that orientation; an orientation
                                      * whose status is not RTX_Q_OK has peak 0.  The reverse complement wins only with a strictly larger peak.  Everything
                                      * a download returns for a query (t, status, global signal, rows, exact matches) is what the chosen orientation gives
                                      * as an input of its own; rtx_batch_strands tells which one it was.  Needs the exact-match lookup of the device
                                      * (rtx_index_has_exact_lookup; a batch with ids passed in is refused: RTX_ERR_INVALID, a handle without the lookup:
                                      * RTX_ERR_STATE), not available on a reference shard (RTX_ERR_INVALID) and without device text (rtx_batch_text:
                                      * RTX_ERR_STATE; rtx_raxtax formats on the host whatever RTX_OPT_DEVICE_TEXT says).  Costs at least twice the step
                                      * time.  Shapes the workspace like the options below. */
#define RTX_OPT_NEAREST 26           /* 0 (default): nothing is launched or allocated, every output is what it is without the option.  1: every run also finds,
                                      * per query, the NEAREST reference -- the lowest reference id (the order of the tree's lineages) whose hit count is the
                                      * query's peak (rtx_batch_strands; the counts as the probability stage sees them, after RTX_SKIP_EXACT_MATCHES) -- and
                                      * the number of references that share that count (ties): rtx_batch_nearest.  A query whose status is not RTX_Q_OK or
                                      * whose peak is 0 has RTX_NO_REF and 0 ties.  Under RTX_OPT_STRAND the values are those of the chosen orientation.
                                      * Exact on the pruned path as well.  Not available on a reference shard (RTX_ERR_INVALID); staged rtx_shard_* runs and
                                      * rtx_debug_evaluate fill nothing.  Setting it drops the uploaded batch like the options below. */
#define RTX_NO_REF 0xFFFFFFFFu       /* no reference (rtx_batch_nearest, rtx_query_hit_fn) */
#define RTX_OPT_IDENTITY 28          /* 0 (default): nothing is launched or allocated.  1: every run also aligns each query, in the orientation that was classified,
                                      * to its nearest reference (RTX_OPT_NEAREST, which must be on: RTX_ERR_STATE otherwise, and switching it off while
                                      * this option is on is refused with RTX_ERR_STATE) and reports the semi-global edit distance of
                                      * rtx_semiglobal_distance: rtx_batch_identity.  A query without a nearest reference (RTX_NO_REF) or longer than
                                      * RTX_IDENTITY_MAX_QUERY bases has RTX_NO_DIST.  Needs a handle that holds the reference sequences (built from a
                                      * tree or from sequences: RTX_ERR_STATE otherwise); not available on a reference shard (RTX_ERR_INVALID); staged
                                      * rtx_shard_* runs and rtx_debug_evaluate fill nothing.  Setting it drops the uploaded batch like RTX_OPT_NEAREST. */
#define RTX_NO_DIST 0xFFFFFFFFu      /* no distance (rtx_batch_identity, rtx_query_align_fn) */
#define RTX_IDENTITY_MAX_QUERY 4096u /* longest query that is aligned: 64 lanes of 64 bases (rtx_identity.hip) */
#define RTX_OPT_DEREP 27             /* 0 (default): no new code runs, nothing is allocated, every output is what it is without the option.  1: DEREPLICATION --
                                      * rtx_raxtax / rtx_raxtax_multi* classify each distinct read of a chunk once: a device stage in front of the handle
                                      * (rtx_derep_run, on a stream of its own, a chunk ahead of the handle) finds the byte-identical copies, the handle
                                      * receives the distinct reads alone, and every query of the caller gets the result of its representative -- its own
                                      * message, label and callbacks, in input order, byte for byte those of a run without the option (the result of a
                                      * query never depends on the rest of its batch).  Per chunk: a copy in another chunk is classified again.  The text
                                      * is formatted on the host whatever RTX_OPT_DEVICE_TEXT says (a device line carries one label); an open profile
                                      * counts a distinct read with its number of copies (rtx_batch_prefetch_weights).  The handles of a call must agree
                                      * on it (RTX_ERR_INVALID).  Only the mirror honours it, as RTX_OPT_DEVICE_TEXT: rtx_batch_* and rtx_classify_batch
                                      * ignore it, it shapes no workspace and drops no uploaded batch. */
/* RTX_OPT_SUB_BATCH, _PACKED_COUNTS, _HIT_PAIR, _TILE_PRUNE and _PROB_MODE shape the workspace that rtx_batch_upload sizes:
 * setting one of them drops the uploaded batch (rtx_batch_run then fails with RTX_ERR_STATE until the batch is uploaded again). */
int rtx_index_set_option(rtx_index *index, int option, uint64_t value);

/* Does tile pruning pay on this database?  Classifies every (n_refs / n_sample)-th reference (n_sample = 0: 1024) as a query with its
 * exact copies left out (RTX_SKIP_EXACT_MATCHES) and tile pruning on, and keeps the share of (query, tile) combinations that stayed live:
 * from 0.85 on the handle leaves tile pruning off (see RTX_OPT_PRUNE_SELF_SAMPLE).  A property of the database: the results of a query
 * never depend on the rest of its batch.  rtx_index_create_from_sequences / _from_tree call it themselves; a handle built from postings
 * (rtx_index_create) has no sequences and keeps pruning on until the caller passes them here.  seq_bytes / seq_off as in
 * rtx_index_create_from_sequences (the references in the order of the handle).  *live_fraction (may be NULL): the share, or -1 where there
 * was nothing to decide (a reference shard, fewer than 4 tiles, no union bitmap).  Any uploaded batch is dropped.
 * The reference has no counterpart: it counts every reference for every query (raxtax.rs:58-64). */
int rtx_index_self_sample(rtx_index *index, const uint8_t *seq_bytes, const uint64_t *seq_off, uint64_t n_refs, uint32_t n_sample, double *live_fraction);
/* *pruning: 1 if tile pruning is on for this handle (RTX_OPT_TILE_PRUNE and the verdict above); *live_fraction: the share the sample kept live, -1 without a sample */
int rtx_index_prune_verdict(const rtx_index *index, int *pruning, double *live_fraction);
/* RTX_OPT_RUN_AHEAD: batches this handle enqueued ahead of the end of the batch before them, and run-aheads it abandoned (RTX_RETRY_CHUNK), since its creation */
int rtx_index_run_ahead_stats(const rtx_index *index, uint64_t *enqueued_ahead, uint64_t *abandoned);
/* Process-wide default for handles created afterwards.  RTX_DEFAULT_SEGMENT_CLASSES (default 1): at index creation
 * every (row, tile) segment of the bitmaps is classified; empty segments are never read and segments with at most
 * 16 references are added from 32-byte slots through byte counters instead of 1-KiB row reads (rtx_segments.hip).
 * 0: every segment is read densely.  Results are identical for either value (A/B measurements). */
#define RTX_DEFAULT_SEGMENT_CLASSES 1
/* RTX_DEFAULT_EXACT_HASH_MASK (default: all ones; 0 restores it): the hash of the device exact-match table is ANDed with this mask.
 * Tests pass a mask of a few bits so that most sequences collide in slot and tag and every probe ends in the byte compare. */
#define RTX_DEFAULT_EXACT_HASH_MASK 2
/* RTX_DEFAULT_DEREP_HASH_MASK (default: all ones; 0 restores it): the hash of rtx_derep_run is ANDed with this mask, read at every run.
 * Tests pass a mask of two bits so that every probe of its table ends in the byte compare. */
#define RTX_DEFAULT_DEREP_HASH_MASK 3
int rtx_set_default_option(int option, uint64_t value);

/* ------------------------------------------------------------------------- */
/* Classification: the body of raxtax(), src/raxtax.rs:39-84, minus string    */
/* formatting (host mirror); the exact-match lookup of raxtax.rs:42 on the     */
/* device, or the caller passes the ids.                                       */
/* ------------------------------------------------------------------------- */
/* One result row = one EvaluationResult (src/lineage.rs:8-14) before the
 * single-exact-match override of raxtax.rs:73-84 (applied by the caller /
 * host mirror, since it needs `raw_confidence` and the lineage strings). */
typedef struct {
    uint32_t n_queries;
    uint64_t n_rows;               /* the length of the row arrays (under RTX_OPT_STRAND they also hold the rows of the orientations that lost: no query refers to them) */
    const uint32_t *t;             /* [n_queries] distinct valid 8-mers (k_mers.len(), raxtax.rs:55) */
    const uint8_t *status;         /* [n_queries] RTX_Q_*                                            */
    const double *global_signal;   /* [n_queries] lineage.rs:86-90                                   */
    const uint64_t *row_begin;     /* [n_queries] rows of query q = row_begin[q] .. row_begin[q] + row_count[q]; */
    const uint32_t *row_count;     /* [n_queries] the rows are stored in processing order, not in query order    */
    const uint32_t *row_lineage;   /* [n_rows] index into tree.lineages (lineage.rs:105)             */
    const uint32_t *row_node;      /* [n_rows] node id (rtx_nodes_view numbering)                    */
    const uint32_t *row_depth;     /* [n_rows] number of confidence values                           */
    const double *row_conf;        /* [n_rows][row_conf_stride] confidence_values, rounded to 2 decimals; entries from row_depth on are 0 */
    const double *row_local_signal;/* [n_rows] lineage.rs:95-102                                     */
    /* ABI 5.  The rows leave the device finalised (rtx_finalise.hip: sorted as lineage.rs:91-93 asks, local signal computed, final
     * layout), the host copies them and nothing else.  row_conf_stride = the deepest lineage of the tree (0 in a view a caller fills
     * by hand = RTX_MAX_DEPTH, the layout of ABI <= 4).  The two byte arrays carry what rtx_result_pack ships (NULL in a hand-made
     * view: the pack converts). */
    uint32_t row_conf_stride;
    const uint8_t *row_depth_u8;        /* [n_rows] row_depth as a byte                                   */
    const uint8_t *row_conf_hundredths; /* [n_rows][row_conf_stride] round(confidence * 100), lineage.rs:128-129 */
} rtx_result_view;

/* Whole path for one batch of queries: H2D, kernels, D2H, host finalisation (sort
 * lineage.rs:91-93 + local signal).  The handle alternates between two host result sets: a view stays
 * valid until the second-next download on the handle, so a caller can format batch c while batch c+1
 * is classified (the host mirror rtx_raxtax does).  exact_ids/exact_off: the ids Tree.sequences.get()
 * returned per query (raxtax.rs:42), or NULL / NULL: the library looks them up on the device (handles built from the reference
 * sequences, RTX_OPT_DEVICE_EXACT; rtx_batch_exact_matches returns them) -- on a handle without that table, or with the option off,
 * NULL means that no query has an exact match. */
/* The upload in two halves, so that the NEXT batch can cross PCIe while the current one is classified (rtx_raxtax does this with its
 * chunks; raxtax.rs:35-36: the reference's workers pick up their next chunk without waiting for anybody either):
 *   rtx_batch_prefetch  validates and stages a batch beside the current one: bases packed two per byte (4-bit codes, parser.rs:11-34)
 *                       into page-locked memory, asynchronous H2D on a stream of its own.  Returns when the host buffers may be reused.
 *   rtx_batch_activate  makes the staged batch the current one (the handle's stream waits for the transfer, the host does not): call
 *                       it once the batch before it has been downloaded, then rtx_batch_run.
 * rtx_batch_upload = prefetch + activate. */
int rtx_batch_prefetch(rtx_index *index, uint64_t n_queries, const uint8_t *bases, const uint64_t *base_off,
                       const uint32_t *exact_ids, const uint64_t *exact_off);
int rtx_batch_activate(rtx_index *index);
/* The packing rtx_batch_prefetch applies, on its own (no device involved): packed[i] = bases[2 i] | bases[2 i + 1] << 4 for n_bases
 * codes (an odd last one alone in its byte; packed holds (n_bases + 1) / 2 bytes).  Returns 1, or 0 if a byte above 15 was seen --
 * no code of parser.rs:11-34; rtx_batch_prefetch sends such a batch as it is. */
int rtx_pack_bases(const uint8_t *bases, uint64_t n_bases, uint8_t *packed);
int rtx_classify_batch(rtx_index *index, uint64_t n_queries, const uint8_t *bases,
                       const uint64_t *base_off, const uint32_t *exact_ids,
                       const uint64_t *exact_off, uint32_t flags, rtx_result_view *out);
/* 1 if the handle can look exact matches up itself (built from the reference sequences, RTX_OPT_DEVICE_EXACT on) */
int rtx_index_has_exact_lookup(const rtx_index *index);
/* The exact matches of the last download as the device found them (the batch was uploaded with exact_off == NULL): CSR over the
 * queries, ids ascending as Tree.sequences holds them (tree.rs:109-112).  Valid as long as the view of that download. */
int rtx_batch_exact_matches(rtx_index *index, const uint64_t **exact_off /*n_queries + 1*/, const uint32_t **exact_ids);

/* Strand and peak of every query of the last download, [n_queries], valid as long as that download's view.  strand: 0 = plus (as given),
 * 1 = minus (the reverse complement was classified; RTX_OPT_STRAND) -- all 0 with the option off.  peak: the largest hit count over the
 * references for the classified orientation (see RTX_OPT_STRAND), filled with the option off as well: peak / t tells how near the nearest
 * reference is.  Either pointer may be NULL.  (A staged run of rtx_shard_* takes no peaks: all 0.) */
int rtx_batch_strands(rtx_index *index, const uint8_t **strand, const uint32_t **peak);
/* The reverse complement as the device builds it, on the host: out[i] = complement(in[n - 1 - i]) (in and out must not overlap).  The formatter
 * uses it for the `.tsv` sequence column of a minus-strand query, which prints the classified orientation. */
int rtx_revcomp(const uint8_t *in, uint64_t n, uint8_t *out);
/* Nearest reference and ties of every query of the last download (RTX_OPT_NEAREST), [n_queries], valid as long as that download's view (each of
 * the two host result sets keeps its own, also under RTX_OPT_RUN_AHEAD).  Either pointer may be NULL.  RTX_ERR_STATE if the run of that
 * download had the option off. */
int rtx_batch_nearest(rtx_index *index, const uint32_t **nearest, const uint32_t **ties);
/* Milliseconds the kernel behind it took over the sub-batches of the last run, and its launches (RTX_OPT_STAGE_TIMING on; else 0 and 0).  Not one
 * of the stages of rtx_batch_stage_times: RTX_NUM_STAGES is part of the ABI.  After rtx_batch_sync. */
int rtx_batch_nearest_time(rtx_index *index, float *ms, uint32_t *launches);
/* Alignment identity of every query of the last download (RTX_OPT_IDENTITY), [n_queries], under the lifetime rules of rtx_batch_nearest.
 * dist: the semi-global edit distance (rtx_semiglobal_distance) of the query, in the orientation that was classified (rtx_batch_strands), to
 * the reference rtx_batch_nearest names, or RTX_NO_DIST; qlen: the query's length in bases.  The identity in hundredths of a percent is
 * ((qlen - dist) * 10000 + qlen / 2) / qlen.  Either pointer may be NULL.  RTX_ERR_STATE if the run of that download had the option off. */
int rtx_batch_identity(rtx_index *index, const uint32_t **dist, const uint32_t **qlen);
/* Milliseconds the alignment kernels took in the last run, and their launches (RTX_OPT_STAGE_TIMING on; else 0 and 0), like
 * rtx_batch_nearest_time: not one of the stages of rtx_batch_stage_times.  After rtx_batch_sync. */
int rtx_batch_identity_time(rtx_index *index, float *ms, uint32_t *launches);
/* The distance of RTX_OPT_IDENTITY on the host, no device involved: the minimum, over all substrings s of r (the empty one included), of the
 * Levenshtein distance between q and s -- substitution, insertion and deletion cost 1 each, the whole query is aligned, the reference's
 * overhang at either end is free.  Bytes as everywhere (one per base, parser.rs:11-34): two match when both are codes (1 .. 15) and share a
 * bit; a byte that is 0 or above 15 matches nothing.  0 <= *dist <= qlen; any lengths. */
int rtx_semiglobal_distance(const uint8_t *q, uint64_t qlen, const uint8_t *r, uint64_t rlen, uint32_t *dist);

/* ---- taxon profile of a run, accumulated on the device (rtx_profile.hip) --------------------------------------------------------------
 * What is in the sample: per node of the taxonomy (rtx_nodes_view numbering) the queries under it, the queries assigned to it and the sum
 * of their confidences, from the BEST LINEAGE of every query -- the one `.out` prints first: the first row of the query, or, where it has
 * exactly one exact match and neither RTX_SKIP_EXACT_MATCHES nor RTX_RAW_CONFIDENCE is in the profile's flags, the Taxon node of that
 * reference with 100 on every level (raxtax.rs:73-84).  Its path a_0 .. a_{depth-1} runs from the child of the root to its node; L = the
 * number of leading levels whose confidence in hundredths reaches the cutoff.  L == 0: the query is `unclassified`; else clade[a_d] += 1 and
 * conf_sum[a_d] += hundredths[d] for d < L, direct[a_{L-1}] += 1, and the query is `classified`.  A query whose status is not RTX_Q_OK or
 * that has no row is `unclassifiable`.  totals = {queries, classified, unclassified, unclassifiable}.  Node 0, the root, stays 0;
 * clade[n] == direct[n] + the clade of n's children, and the sum of direct is totals[1].  Integers throughout: the result is exact and
 * does not depend on the order of the queries.
 * Off unless begun: no allocation, no launch, every other output what it is without it.  While a profile is open every batch is added ONCE,
 * when its download accepts it (rtx_batch_download / _download_then_run / rtx_classify_batch, rtx_raxtax*): a run that is repeated for buffer
 * space, a batch that ends in RTX_RETRY_CHUNK and a second download of one run add nothing; neither do rtx_debug_evaluate and staged
 * rtx_shard_* runs.  Under RTX_OPT_STRAND a query counts with the orientation that was chosen.
 *   rtx_index_profile_begin  cutoff_hundredths 1 .. 100, flags RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE (either one: no override); allocates
 *                            and zeroes the counters.  RTX_ERR_INVALID: cutoff out of range, unknown flags, a reference shard; RTX_ERR_STATE:
 *                            a profile is open already.
 *   rtx_index_profile_read   the counters of everything downloaded so far, copied to host arrays that stay valid until the next read, reset
 *                            or end.  RTX_ERR_STATE (also reset, end, time): no profile is open.
 *   rtx_index_profile_reset  zeroes the counters, the profile stays open.
 *   rtx_index_profile_end    switches the accumulation off and frees everything.
 *   rtx_index_profile_time   milliseconds and launches of the kernel since begin or reset, for downloads under RTX_OPT_STAGE_TIMING (else 0, 0).
 *   rtx_profile_merge        sums n profiles (one handle per GPU) into caller arrays of n_nodes entries; RTX_ERR_INVALID when the views differ
 *                            in n_nodes, cutoff or flags.
 *   rtx_profile_format       the report: "# cutoff=0.80<TAB>queries=N<TAB>classified=A<TAB>unclassified=B<TAB>unclassifiable=C", then
 *                            "clade<TAB>direct<TAB>percent<TAB>mean_conf<TAB>depth<TAB>taxon<TAB>lineage", then one line per node with clade > 0 in
 *                            pre-order (node_begin ascending, then depth ascending); percent = (clade * 10000 + N / 2) / N printed with two
 *                            decimals, mean_conf = (conf_sum + clade / 2) / clade hundredths likewise, lineage = the first `depth` levels of
 *                            lineages[node_begin], taxon = the last of them.  Every line ends in '\n', no NUL.  Returns the bytes written,
 *                            with out == NULL the bytes needed; a buffer that is too small: -(bytes needed) - RTX_NEED_BASE.
 * rtx_raxtax and rtx_raxtax_multi* honour open profiles: all handles of a call have one open, with one cutoff, or none has, and its flags
 * are the call's skip_exact_matches / raw_confidence (RTX_ERR_INVALID otherwise). */
typedef struct {
    uint32_t n_nodes;
    uint32_t cutoff_hundredths;
    uint32_t flags;
    const uint64_t *clade, *direct, *conf_sum; /* [n_nodes] */
    uint64_t totals[4];
} rtx_profile_view;
int rtx_index_profile_begin(rtx_index *index, uint32_t cutoff_hundredths, uint32_t flags);
int rtx_index_profile_read(rtx_index *index, rtx_profile_view *out);
int rtx_index_profile_reset(rtx_index *index);
int rtx_index_profile_end(rtx_index *index);
int rtx_index_profile_time(rtx_index *index, float *ms, uint32_t *launches);
int rtx_profile_merge(rtx_profile_view *const *views, uint32_t n, uint64_t *clade, uint64_t *direct, uint64_t *conf_sum, uint64_t totals[4]);
int64_t rtx_profile_format(const rtx_tree *tree, const uint64_t *clade, const uint64_t *direct, const uint64_t *conf_sum,
                           const uint64_t totals[4], uint32_t cutoff_hundredths, char *out, uint64_t cap);

/* One weight per query for the batch that the NEXT rtx_batch_prefetch / rtx_batch_upload stages (call it first): the number of reads the
 * query stands for in the open profile -- every counter takes weight (conf_sum: weight x hundredths) where it takes 1 without; 0: the query
 * does not count.  The path of rtx_batch_prefetch_labels: the same input set, asynchronous, taken or dropped at that prefetch; a count that
 * does not match the batch is dropped (every query then counts once).  Indexed by the caller's query under RTX_OPT_STRAND.  rtx_raxtax*
 * stage the copies of every distinct read this way under RTX_OPT_DEREP. */
int rtx_batch_prefetch_weights(rtx_index *index, uint64_t n_queries, const uint32_t *weights);

/* ---- per-sample counts beside the profile (rtx_profile.hip: profile_samples_kernel) ------------------------------------------------------
 * The taxon x sample table of a pooled run: the profile's `direct` and `totals` once more, split by the sample every query belongs to
 * (rtx_demux_run names it).  A query with a sample s adds its weight (or 1) to direct_by_sample[s][a_{L-1}] when it is classified, and to
 * totals_by_sample[s][0] and the entry of its kind, exactly as it adds to the profile's own counters -- with the same best lineage, cutoff
 * and flags, once per accepted batch.  Integer adds: exact, independent of the order.  The per-sample clade is derived on the host
 * (clade[n] = direct[n] + the clade of n's children: rtx_sample_table_format does).  A sparse table, per-sample conf_sum and
 * dereplication together with samples are out of scope.
 *   rtx_index_profile_begin_samples  opens a profile exactly as rtx_index_profile_begin does -- every rtx_index_profile_* call works on it
 *                            unchanged, end frees everything -- and allocates and zeroes direct_by_sample[n_samples][n_nodes] and
 *                            totals_by_sample[n_samples][4] (uint64).  RTX_ERR_INVALID besides: n_samples == 0, or n_samples x n_nodes
 *                            above RTX_PROFILE_MAX_SAMPLE_COUNTERS (2^28 counters, 2 GiB; rtx_last_error names the limit).
 *   rtx_batch_prefetch_samples  one sample per query for the batch that the NEXT rtx_batch_prefetch / rtx_batch_upload stages: the path and
 *                            the rules of rtx_batch_prefetch_weights (asynchronous, taken or dropped at that prefetch, dropped on a count
 *                            that does not match, indexed by the caller's query under RTX_OPT_STRAND).  RTX_DEMUX_NONE: the query
 *                            counts in no sample; any other value >= n_samples: RTX_ERR_INVALID; RTX_ERR_STATE without such a profile.
 *                            A batch with nothing staged counts in no sample.
 *   rtx_index_profile_read_samples  the per-sample counters of everything downloaded so far, copied to host arrays that stay valid until
 *                            the next such read, reset or end.  RTX_ERR_STATE without such a profile.  rtx_index_profile_reset zeroes
 *                            them with the rest.
 *   rtx_sample_profile_merge sums n such views (one handle per GPU) into caller arrays of n_samples x n_nodes and n_samples x 4 entries;
 *                            RTX_ERR_INVALID when the views differ in n_nodes, n_samples, cutoff or flags.
 *   rtx_sample_table_format  the table: "# cutoff=0.80<TAB>samples=S"; four lines "# queries", "# classified", "# unclassified",
 *                            "# unclassifiable", each followed by S tab-separated values; "depth<TAB>taxon<TAB>lineage" followed by the S
 *                            names; then one line per node whose clade is not zero in some sample, in the pre-order of rtx_profile_format:
 *                            depth, taxon, lineage and the S clade counts.  Every line ends in '\n', no NUL; the return convention of
 *                            rtx_profile_format. */
#define RTX_PROFILE_MAX_SAMPLE_COUNTERS (1ull << 28)
typedef struct {
    uint32_t n_nodes, n_samples;
    uint32_t cutoff_hundredths;
    uint32_t flags;
    const uint64_t *direct; /* [n_samples][n_nodes] */
    const uint64_t *totals; /* [n_samples][4] */
} rtx_sample_profile_view;
int rtx_index_profile_begin_samples(rtx_index *index, uint32_t cutoff_hundredths, uint32_t flags, uint32_t n_samples);
int rtx_batch_prefetch_samples(rtx_index *index, uint64_t n_queries, const uint32_t *sample);
int rtx_index_profile_read_samples(rtx_index *index, rtx_sample_profile_view *out);
int rtx_sample_profile_merge(rtx_sample_profile_view *const *views, uint32_t n, uint64_t *direct, uint64_t *totals);
int64_t rtx_sample_table_format(const rtx_tree *tree, uint32_t n_samples, const char *const *names, const uint64_t *direct, const uint64_t *totals,
                                uint32_t cutoff_hundredths, char *out, uint64_t cap);

/* The same in stages, so that a caller (bench.py) can keep inputs resident in HBM and
 * time the device part alone, or overlap stages of different batches. */
int rtx_batch_upload(rtx_index *index, uint64_t n_queries, const uint8_t *bases,
                     const uint64_t *base_off, const uint32_t *exact_ids,
                     const uint64_t *exact_off);
int rtx_batch_run(rtx_index *index, uint32_t flags); /* enqueue all kernels (async)        */
int rtx_batch_sync(rtx_index *index);                /* wait for the handle's stream        */
int rtx_batch_download(rtx_index *index, rtx_result_view *out);
/* rtx_batch_download of the current batch that, as soon as the last result records have left the device, makes the STAGED batch
 * (rtx_batch_prefetch) the current one and runs it with `flags` (= rtx_batch_activate + rtx_batch_run) -- the host finalises the last
 * sub-batch of this batch while the device already classifies the next (rtx_raxtax's chunks follow one another without the host's
 * finalisation between them).  Nothing staged: plain rtx_batch_download.  Under RTX_OPT_RUN_AHEAD the staged batch is enqueued before the
 * current one has finished, and the call may return RTX_RETRY_CHUNK (> 0). */
int rtx_batch_download_then_run(rtx_index *index, rtx_result_view *out, uint32_t flags);

/* ---- dereplication (rtx_derep.hip; RTX_OPT_DEREP is the host mirror's use of it) --------------------------------------------------------
 * Which queries of a batch are copies of an earlier one -- what `vsearch --derep_fulllength` does in front of a classifier, on the device.
 *   rtx_derep_create  an object of its own on GPU `device`: one stream, its own buffers (they only grow), no rtx_index.  It may run beside
 *                     a handle on the same device; distinct objects may be driven from distinct threads, calls on one are serialised by
 *                     the caller.  RTX_ERR_NO_DEVICE without a gfx950.
 *   rtx_derep_run     rep[q] = the lowest q' <= q whose sequence is identical to that of q: the same length and the same bytes as given
 *                     (ambiguity codes and bytes above 15 compared as they are; a read and its reverse complement are different reads).
 *                     *n_unique = the number of q with rep[q] == q.  Exact -- a hash only picks the candidates, the bytes decide -- and
 *                     the same whatever the scheduling.  bases / base_off as rtx_batch_prefetch takes them.  n == 0: RTX_OK, *n_unique = 0;
 *                     n > 2^31 - 2 or a base_off that is not monotone: RTX_ERR_INVALID.  Synchronous.
 *   rtx_derep_plan    the host side of the map (no device): uniq[u] = the queries with rep[q] == q, ascending (*n_unique of them);
 *                     slot[q] = the position of rep[q] in uniq; size[u] = the queries whose representative is uniq[u].  All three hold n
 *                     entries.  RTX_ERR_INVALID if rep is no such map (rep[q] > q, or rep[rep[q]] != rep[q]).
 *   rtx_raxtax_last_derep  the last rtx_raxtax* call of the process: the queries of its dereplicated chunks, the distinct reads handed to
 *                     the handles and the busy seconds of the stage (map, plan and the copy of the distinct reads); all 0 with the option off. */
typedef struct rtx_derep rtx_derep;
int rtx_derep_create(int device, rtx_derep **out);
int rtx_derep_run(rtx_derep *d, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *rep /*[n]*/, uint64_t *n_unique);
void rtx_derep_destroy(rtx_derep *d);
int rtx_derep_plan(uint64_t n, const uint32_t *rep, uint32_t *uniq /*[n]*/, uint32_t *slot /*[n]*/, uint32_t *size /*[n]*/, uint64_t *n_unique);
int rtx_raxtax_last_derep(uint64_t *queries, uint64_t *distinct, double *busy_seconds);

/* ---- distinct reads of a run (rtx_tally.hip, host_tally.cpp; rtx_index_set_tally is the host mirror's use of it) ----------------------------
 * The distinct sequences of a whole run with their abundances, per sample -- what `vsearch --derep_fulllength --sizeout` and `--otutabout`
 * (or DADA2's sequence table) leave -- accumulated on the device over any number of chunks and calls.  Unlike rtx_derep the object owns
 * its sequences: an open-addressing table of entry + 1 (at most half full), per entry hash, length and offset into an arena of bases (one
 * byte per base, every entry from a multiple of 8 bytes on), a dense uint32 matrix [entries x columns] of counts, 64-bit totals.  All of
 * them start small and grow by doubling up to the caps.  Exact: a hash picks the candidates, the bytes decide, always; a read and its
 * reverse complement are different reads, also under RTX_OPT_STRAND (a read is tallied as given).
 *   rtx_tally_create  an object of its own on GPU `device` (one stream; RTX_ERR_NO_DEVICE without a gfx950), owned by the caller and alive
 *                     as long as the caller wants.  params (NULL: all defaults): n_samples columns (0: one column, and `sample` is not
 *                     needed); max_entries (0: RTX_TALLY_DEFAULT_MAX_ENTRIES; at most 2^31 - 2) and max_bytes (0:
 *                     RTX_TALLY_DEFAULT_MAX_BYTES) cap the entries and the arena; initial_entries / initial_bytes (0:
 *                     RTX_TALLY_DEFAULT_INITIAL_ENTRIES / _BYTES) size the first allocation.  RTX_ERR_INVALID: max_entries above
 *                     2^31 - 2, or a matrix of max_entries x columns cells beyond 2^40.
 *   rtx_tally_add     one chunk: read q adds weight[q] (NULL: 1) to the cell (its sequence, sample[q]) (NULL: column 0).  A read of weight
 *                     0 or of length 0 is not looked at any further (its sample may be anything, RTX_DEMUX_NONE included) and creates no
 *                     entry.  Checked on the host before anything is enqueued, RTX_ERR_INVALID: a sample >= max(1, n_samples) on a read
 *                     that counts; a total counted weight of the object above 2^32 - 1 (no cell can wrap); n > 2^31 - 2; offsets that are
 *                     not monotone; a read of 2^32 bases or more.  Three steps on the object's stream, separate launches, so that no wave waits for another:
 *                     lookup in the table (read-only); the reads it does not know among themselves (the chunk-local table of
 *                     rtx_derep_run) and a scan that numbers the new distinct reads in the order of their read index -- entry ids are the
 *                     order of first appearance, whatever the scheduling; then append and count.  Between the second and the third the
 *                     host learns the scan's totals and grows the buffers.  Caps: a new distinct read is stored if and only if its
 *                     inclusive scan position is within max_entries and max_bytes; the reads of the others are summed into
 *                     overflow_reads and their sequences into no entry (presented again, they overflow again): a run never fails for
 *                     being diverse.  The call returns when the third step is enqueued; bases / base_off as rtx_batch_prefetch takes
 *                     them, free at return.  Calls on one object are serialised by the caller.
 *   rtx_tally_read    waits for the object's stream, downloads and sorts: a new table (below), to be destroyed by the caller.  The object
 *                     goes on counting.
 *   rtx_tally_info    entries and arena bytes in use, their present capacities, counted weight so far (any pointer may be NULL).
 *   RTX_DEFAULT_TALLY_HASH_MASK (rtx_set_default_option; default: all ones; 0 restores it): the hash of rtx_tally_add is ANDed with this
 *                     mask, read at every add (an object whose table was laid out under another mask lays it out again first).  For tests.
 * rtx_tally_table: the table on the host, opaque.  Rows sorted by total size descending, then by their bytes ascending (a prefix before
 * the longer sequence); one count per column; totals {reads: the weight of all reads that counted, entries, overflow_reads}.
 *   rtx_tally_table_create / _add   the same accumulation on the host (a hash map), without caps: the host restatement of rtx_tally_add,
 *                     with its checks.
 *   rtx_tally_table_merge           the sum of n tables (one object per handle): equal sequences are summed; RTX_ERR_INVALID when the column
 *                     counts differ.  A new table.
 *   rtx_tally_table_view            the rows (valid until the table is added to or destroyed): `first` is the rank of a row's entry in the
 *                     order of first appearance (of the object, or of the host accumulation; of a merged table: table after table).
 *   rtx_tally_format_fasta          `>uniq{rank};size={N}\n{sequence}\n` per row, rank from 1 in table order; the letters are those of the
 *                     `.tsv` sequence column (A C G T, anything else '-').  Rows with a total below minsize are left out; the ranks stay
 *                     those of the whole table.  Returns the bytes written, with buf == NULL the bytes needed; a buffer that is too small:
 *                     -(bytes needed) - RTX_NEED_BASE (as rtx_profile_format).
 *   rtx_tally_format_table          `#uniq\t{names, tab-separated}\n`, then `uniq{rank}\t{counts}\n` per row, under the same minsize and
 *                     the same protocol.  names: one per column.
 *   rtx_index_set_tally / rtx_index_tally   the object rtx_raxtax* tally into (NULL: off; the handle itself never reads it).  Its device
 *                     must be the handle's (RTX_ERR_INVALID).  On every handle of a call or on none, no two handles with one object, and
 *                     n_samples equal to the samples of the tag list (rtx_index_set_tags) when tags are set, 0 otherwise: RTX_ERR_INVALID
 *                     from the call otherwise.  The tally is the last stage of the front: it counts exactly the reads that go on to be
 *                     classified -- not one that is unassigned, emptied, discarded, a contaminant or flagged as a chimera -- each with its
 *                     own sample, with and without RTX_OPT_DEREP (copies count as reads).
 *   rtx_raxtax_last_tally  the last rtx_raxtax* call of the process: the queries of its tallied chunks, those that counted, the entries the
 *                     objects gained and the busy seconds of the stage; all 0 with no tally set. */
#define RTX_DEFAULT_TALLY_HASH_MASK 4
#define RTX_TALLY_DEFAULT_MAX_ENTRIES (1ull << 24)
#define RTX_TALLY_DEFAULT_MAX_BYTES (1ull << 33)
#define RTX_TALLY_DEFAULT_INITIAL_ENTRIES (1ull << 16)
#define RTX_TALLY_DEFAULT_INITIAL_BYTES (1ull << 25)
typedef struct rtx_tally rtx_tally;
typedef struct rtx_tally_table rtx_tally_table;
typedef struct rtx_tally_params {
    uint32_t n_samples;
    uint64_t max_entries, max_bytes, initial_entries, initial_bytes;
} rtx_tally_params;
typedef struct rtx_tally_view {
    uint64_t n_entries;
    uint32_t n_columns;
    const uint8_t *bases;      /* the rows' sequences back to back, one code per byte */
    const uint64_t *base_off;  /* [n_entries + 1] */
    const uint64_t *counts;    /* [n_entries x n_columns] */
    const uint64_t *sizes;     /* [n_entries] the sum of a row */
    const uint64_t *first;     /* [n_entries] rank in the order of first appearance, from 0 */
    uint64_t totals[3];        /* reads, entries, overflow_reads */
} rtx_tally_view;
int rtx_tally_create(int device, const rtx_tally_params *params, rtx_tally **out);
int rtx_tally_add(rtx_tally *t, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample /*[n] or NULL*/, const uint32_t *weight /*[n] or NULL: 1*/);
int rtx_tally_read(rtx_tally *t, rtx_tally_table **table);
int rtx_tally_info(const rtx_tally *t, uint64_t *entries, uint64_t *bytes, uint64_t *entry_capacity, uint64_t *byte_capacity, uint64_t *counted);
void rtx_tally_destroy(rtx_tally *t);
int rtx_tally_table_create(uint32_t n_samples, rtx_tally_table **out);
int rtx_tally_table_add(rtx_tally_table *table, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample, const uint32_t *weight);
int rtx_tally_table_merge(rtx_tally_table *const *tables, uint32_t n, rtx_tally_table **out);
int rtx_tally_table_view(rtx_tally_table *table, rtx_tally_view *view);
void rtx_tally_table_destroy(rtx_tally_table *table);
int64_t rtx_tally_format_fasta(rtx_tally_table *table, uint64_t minsize, char *buf, uint64_t cap);
int64_t rtx_tally_format_table(rtx_tally_table *table, const char *const *names, uint64_t minsize, char *buf, uint64_t cap);
int rtx_index_set_tally(rtx_index *index, rtx_tally *tally);
rtx_tally *rtx_index_tally(const rtx_index *index);
int rtx_raxtax_last_tally(uint64_t *queries, uint64_t *counted, uint64_t *entries_added, double *busy_seconds);

/* ---- OTUs of a run (rtx_otu.hip, host_otu.cpp) ---------------------------------------------------------------------------------------------
 * The distinct reads of a run collapsed into OTUs by Swarm's d = 1 rule (Mahe et al.), with breaking -- what `swarm` leaves by default.
 * Exact, integers only, independent of scheduling.  The input is an rtx_tally_table: rows by total size descending, then bytes ascending;
 * the row index is the rank.  Codes are one per byte; 1, 2, 4, 8 are A, C, G, T.
 *   link         rows x and y are linked iff y is x with one code deleted (at any position, whatever the code), or the same with x and y
 *                swapped, or x and y have equal length and differ at exactly one position where at least one of the two holds one of
 *                1, 2, 4, 8: the symmetric closure of "x generates y by deleting one code or by replacing one code with A, C, G or T".
 *                An N (15) against a plain base links; two different ambiguity codes at one position do not.  A row longer than
 *                RTX_OTU_MAX_LEN has no link at all and is counted in long_rows.  The links are pairs (a, b), a < b, sorted by (a, b).
 *   OTU          take the unassigned row of lowest rank as a seed; grow it breadth-first, a member x pulling in every still unassigned
 *                linked y with size[y] <= size[x]; repeat until every row is assigned.  Equivalently (what the device computes): the label
 *                of y is the lowest rank of any row from which y is reached along links whose sizes never increase.  OTUs are numbered
 *                from 0 in the order of their seeds' ranks; an OTU's size per column is the sum over its members.
 *   rtx_otu_cluster       on GPU `device` (RTX_ERR_NO_DEVICE without a gfx950): the rows are uploaded and laid out in a table of their own
 *                ({tag, row + 1} slots, at most half full); the link kernel forms the hash of every single-difference variant of a row from
 *                the row's own prefix and suffix sums of word mixes and probes the table read-only -- a hash picks the candidates, the
 *                bytes decide, always; links are appended through a counter that goes on counting past the buffer (initial_links pairs;
 *                0: a default from the row count), and a pass that does not fit is run once more in a buffer that does (link_passes);
 *                labels are propagated with atomicMin over the links to the fixed point (rounds); a scan numbers the seeds.
 *   rtx_otu_cluster_host  the same result from the definition: every variant looked up in the table's own map, then the greedy growth as
 *                stated.  Equal to the device's result field by field, except rounds and link_passes (1).
 *                params (NULL: defaults): differences 0 or 1 mean 1, anything else RTX_ERR_INVALID; flags must be 0.  More than 2^31 - 2
 *                rows: RTX_ERR_INVALID.  The table is laid out (rtx_tally_table_view) and otherwise unchanged.
 *   rtx_otu_view          valid until the object is destroyed.  rtx_otu_times: seconds of upload (and table layout), link passes, label rounds
 *                and numbering, download and sort of the last device run; all 0 for a host result.
 *   rtx_otu_format_fasta  `>otu{k};size={N};seed=uniq{rank}\n{sequence of the seed}\n` per OTU, k from 1, rank as in rtx_tally_format_fasta
 *                of the same table.  OTUs with a total below minsize are left out, the numbers stay.  Buffer protocol of
 *                rtx_tally_format_fasta.  `table` must be the table the OTUs were made from (RTX_ERR_INVALID when the row counts differ).
 *   rtx_otu_format_table  `#otu\t{names, tab-separated}\n`, then `otu{k}\t{counts}\n` per OTU under the same minsize.  One name per column.
 *   rtx_otu_format_map    `uniq{rank}\totu{k}\n` per row of the table.
 *   RTX_DEFAULT_OTU_HASH_MASK (rtx_set_default_option; default: all ones; 0 restores it): the hashes of rtx_otu_cluster are ANDed with this
 *                mask, read at every call.  For tests: under a mask of two bits every probe ends in the byte compare. */
#define RTX_DEFAULT_OTU_HASH_MASK 5
#define RTX_OTU_MAX_LEN 4096
typedef struct rtx_otu rtx_otu;
typedef struct rtx_otu_params {
    uint32_t differences; /* 0 or 1: 1 */
    uint32_t flags;       /* 0 */
    uint64_t initial_links;
} rtx_otu_params;
typedef struct rtx_otu_view_t {
    uint64_t n_rows, n_otus;
    uint32_t n_columns;
    const uint32_t *otu;      /* [n_rows] the OTU of a row */
    const uint32_t *seed;     /* [n_otus] the rank of the seed */
    const uint64_t *members;  /* [n_otus] rows */
    const uint64_t *sizes;    /* [n_otus] the sum of the counts */
    const uint64_t *counts;   /* [n_otus x n_columns] */
    uint64_t n_links;
    const uint32_t *link_a, *link_b; /* [n_links] a < b, sorted by (a, b) */
    uint32_t rounds;      /* device: label rounds up to and including the first without a change; host: 0 */
    uint32_t link_passes; /* device: runs of the link kernel (2: the first buffer was too small); host: 1 */
    uint64_t long_rows;
} rtx_otu_view_t;
int rtx_otu_cluster(int device, rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out);
int rtx_otu_cluster_host(rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out);
int rtx_otu_view(rtx_otu *otu, rtx_otu_view_t *view);
int rtx_otu_times(const rtx_otu *otu, double seconds[4]);
void rtx_otu_destroy(rtx_otu *otu);
int64_t rtx_otu_format_fasta(rtx_otu *otu, rtx_tally_table *table, uint64_t minsize, char *buf, uint64_t cap);
int64_t rtx_otu_format_table(rtx_otu *otu, const char *const *names, uint64_t minsize, char *buf, uint64_t cap);
int64_t rtx_otu_format_map(rtx_otu *otu, char *buf, uint64_t cap);

/* ---- Fastidious grafting (rtx_graft.hip, host_otu.cpp) ---------------------------------------------------------------------------------------
 * Swarm's second pass (`swarm -f`): small OTUs of a d = 1 clustering are grafted onto a large OTU that holds a row at most two differences
 * away.  Exact, integers only, independent of scheduling.
 *   input        an rtx_tally_table, the rtx_otu made from it, and the boundary B (default 3, at least 1).
 *   ball         for a row x of len codes, 1 <= len <= RTX_OTU_MAX_LEN, B1(x) is the set of byte strings holding: x itself; x with one code
 *                replaced by one of A, C, G, T (1, 2, 4, 8) other than the code that is there; x with one code deleted, only if len >= 2 (no
 *                empty string is formed); x with one of A, C, G, T inserted at any of the len + 1 places, only if len + 1 <=
 *                RTX_OTU_MAX_LEN.  A row longer than RTX_OTU_MAX_LEN has no ball.
 *   near         rows x and y are near iff B1(x) and B1(y) share a string, compared as bytes.  Ambiguity codes are ordinary bytes here: two
 *                rows that differ in two different ambiguity codes at one position are near (either becomes the same plain row).  For rows
 *                over A, C, G, T near is "Levenshtein distance <= 2".  Every d = 1 link is near.
 *   heavy/light  OTU k of the input is heavy iff sizes[k] >= B, light otherwise; a row is what its OTU is.
 *   parent       for a light row x the lowest rank of a heavy row near x; 0xFFFFFFFF if there is none, and for heavy rows.
 *   graft        a light OTU with at least one member that has a parent is grafted: its graft is the pair (parent[x], x) that is smallest
 *                in (parent, child) order over its members, its target otu[parent].  Targets are heavy and heavy OTUs are never grafted: no
 *                chains.  A light OTU that is near light rows only stays as it is.
 *   result       a new rtx_otu over the same table.  The surviving OTUs keep THEIR OWN seeds and are numbered from 0 in the order of those
 *                seeds' ranks (the relative order of their old numbers); otu'[r] is the new number of the target of otu[r], or of otu[r]
 *                itself; members, sizes and counts are the sums.  A grafted row may outrank the seed of its new OTU: the seed is not the
 *                lowest-ranked member any more.  Links, rounds, link_passes and long_rows are copied from the input, so rtx_otu_view, the
 *                three rtx_otu_format_* functions and rtx_denovo_check(table, otu) take the object as any other.  B = 1 grafts nothing.
 *   rtx_otu_graft         on GPU `device` (RTX_ERR_NO_DEVICE without a gfx950).  Every string of the heavy rows' balls is hashed -- in O(1)
 *                each, from the row's prefix sums of word mixes, as the link kernel of rtx_otu_cluster does; a third sum over the words
 *                shifted up by one byte serves the insertions -- and sets k = 4 bits of a Bloom filter of 2^bloom_log2 bits (0: the smallest
 *                power of two with 16 bits per string, under max_bloom_bytes, 0: 8 GiB).  The light rows' balls are tested against it; what
 *                passes is a candidate (row, kind, position, code), appended through a counter that goes on counting past the buffer
 *                (initial_candidates; 0: max(1024, 4 x light rows)); a pass that does not fit is run once more in a buffer that does
 *                (test_passes).  A candidate string v is then built, and every row that has v in ITS ball -- v itself, v with a plain
 *                code replaced by any code that occurs in a heavy row, v with such a code inserted, v with a plain code deleted -- is
 *                looked up in the table of all rows: a hash picks the candidates, the bytes decide, always.  A heavy row found lowers
 *                parent[x] with atomicMin.  The filter decides nothing: a smaller one only makes more candidates.
 *   rtx_otu_graft_host    the definition restated: a map from every string of the heavy rows' balls to the lowest heavy rank, the light rows'
 *                balls looked up in it.  Equal to the device's result field by field, except the filter's counters (variants, candidates,
 *                confirmed, bloom_log2, test_passes: 0) and the times.
 *                RTX_ERR_INVALID: a table whose row count is not the object's, flags != 0, bloom_log2 neither 0 nor within 5 .. 40.
 *                A boundary of 0 is the default.  RTX_DEFAULT_OTU_HASH_MASK applies to this stage too, read at every call.
 *   rtx_otu_graft_view    of a graft result (RTX_ERR_INVALID on any other rtx_otu): parent, old_to_new, the grafts sorted by the old light
 *                OTU, the counters, and the seconds of upload, Bloom, test, verify, resolve and download.  Valid until the object is destroyed.
 *   rtx_otu_format_grafts `#light\tsize\tchild\tparent\theavy\tinto\n`, then `otu{k}\t{size}\tuniq{rank}\tuniq{rank}\totu{k}\totu{k'}\n` per
 *                graft: the old light OTU and its size, child and parent row, the old heavy OTU, the new number; all counted from 1.
 *                Buffer protocol of rtx_tally_format_fasta. */
typedef struct rtx_graft_params {
    uint64_t boundary;
    uint32_t bloom_log2;
    uint32_t flags;
    uint64_t max_bloom_bytes;
    uint64_t initial_candidates;
} rtx_graft_params; /* 0 = default everywhere; flags must be 0 */
typedef struct rtx_graft_view_t {
    uint64_t n_rows, n_old_otus, n_otus, n_grafts;
    uint64_t boundary;
    const uint32_t *parent;     /* [n_rows] */
    const uint32_t *old_to_new; /* [n_old_otus] */
    const uint32_t *light, *child, *par, *heavy, *into; /* [n_grafts] old light OTU, child row, parent row, old heavy OTU, new number; from 0 */
    const uint64_t *size;       /* [n_grafts] the size of the old light OTU */
    uint64_t heavy_otus, light_otus, heavy_rows, light_rows;
    uint64_t variants;          /* strings of the heavy rows' balls put into the filter */
    uint64_t candidates;        /* strings of the light rows' balls that passed it */
    uint64_t confirmed;         /* candidates with a heavy row behind them */
    uint32_t bloom_log2, test_passes;
    double seconds[5];
} rtx_graft_view_t;
int rtx_otu_graft(int device, rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out);
int rtx_otu_graft_host(rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out);
int rtx_otu_graft_view(rtx_otu *grafted, rtx_graft_view_t *view);
int64_t rtx_otu_format_grafts(rtx_otu *grafted, char *buf, uint64_t cap);

/* ---- Denoising (UNOISE) (rtx_unoise.hip, host_unoise.cpp) ------------------------------------------------------------------------------------
 * The distinct reads of a run denoised into ZOTUs by the UNOISE rule (Edgar 2016): a read is an error of a more abundant read d differences
 * away when size(child) / size(parent) <= 1 / 2^(alpha d + 1).  Exact, integers only, independent of scheduling.
 *   input        an rtx_tally_table (rows by total size descending, then bytes ascending; the row index is the rank; w[r] is the total of a
 *                row; one code per byte) and minsize (default 8, at least 1), alpha (default 2, an integer in 1 .. 8), max_diffs (0: the
 *                default RTX_UNOISE_MAX_DIFFS = 16, at most 16), flags (0).
 *   distance     d(x, y) is the Levenshtein distance of the two rows as byte strings: global, both ends anchored, unit costs, two codes
 *                match iff the bytes are equal (an ambiguity code matches itself and nothing else).  A row longer than RTX_OTU_MAX_LEN has
 *                no distance to anything.
 *   allowed      for rows p < e, k(e, p) is the largest d in 0 .. max_diffs with (w[p] >> (alpha d + 1)) >= w[e]; a shift of 64 or more
 *                gives 0.  k = 0: not a candidate.  Weights never increase along the table, so lim(e) = #{p : (w[p] >> (alpha + 1)) >= w[e]}
 *                is a prefix of the table, and only p < lim(e) can have k >= 1.
 *   recursion    over e = 0, 1, ...: p is a live parent iff its status is ZOTU.  e is ABSORBED iff some live p < lim(e) has
 *                d(e, p) <= k(e, p); its parent is the such p with the smallest (d, p), dist that d.  Otherwise e is a ZOTU if
 *                w[e] >= minsize, else LEFT (small, without a parent; never a parent).  A row longer than RTX_OTU_MAX_LEN is LONG: never
 *                compared, never a parent.  The status of e depends only on statuses below lim(e) <= e: exactly one solution.  An absorbed
 *                read is no parent (UNOISE's greedy rule), parents are ZOTUs: no chains.
 *   result       a new rtx_otu over the same table.  Every row that is not absorbed seeds an OTU of its own, numbered from 0 in the order
 *                of the seeds' ranks; otu[r] is its own OTU or its parent's; members, sizes and counts are the sums; n_links, rounds and
 *                link_passes are 0; long_rows as rtx_otu_cluster sets it.  rtx_otu_view, the three rtx_otu_format_* functions,
 *                rtx_denovo_check(table, otu) and rtx_otu_taxonomy take the object as any other.
 *   rtx_otu_unoise        on GPU `device` (RTX_ERR_NO_DEVICE without a gfx950).  The table is cut into tiers [s0, s1), s1 the first row
 *                with (w[s0] >> (alpha + 1)) >= w[s1]: no row of a tier can be the parent of another, so a tier's statuses depend on
 *                earlier tiers only, and there are at most 64 / (alpha + 1) + 1 tiers.  Per tier a pair kernel takes every (row of the
 *                tier, live centroid below lim(row)) -- the row is a wave's pattern, one centroid per lane the text; k from the two
 *                weights; a pair whose lengths differ by more than k is dropped; the others run Hyyro's bit-vector step on a band of 64
 *                rows that slides down the diagonal, which gives the exact d whenever d <= k, and stop at the first column where the cell
 *                on the final diagonal exceeds k -- and folds (d << 32 | p) per row with a 64-bit atomicMin; a decide kernel writes the
 *                statuses; a scan appends the tier's new ZOTUs to the centroid list in rank order.  Rows travel as 4-bit codes, sixteen to
 *                a 64-bit word: a table with a byte above 15 is refused (RTX_ERR_INVALID) by this entry.
 *   rtx_otu_unoise_host   the definition restated literally: e ascending, an explicit list of live parents, a plain two-row dynamic
 *                programme over the bytes.  Equal to the device's result field by field, except the device's counters and the times (0).
 *                RTX_ERR_INVALID: alpha outside 1 .. 8, minsize 0 (in a params that is given), max_diffs above 16, flags != 0, more than
 *                2^31 - 2 rows.  params NULL: the defaults.  The table is laid out (rtx_tally_table_view) and otherwise unchanged.
 *   rtx_otu_unoise_view   of a denoising result (RTX_ERR_INVALID on any other rtx_otu); valid until the object is destroyed.
 *   rtx_otu_format_unoise `#read\tsize\tstatus\tparent\tdiffs\totu\n`, then `uniq{rank}\t{size}\t{zotu|absorbed|left|long}\t{uniq{rank}|*}\t
 *                {d|*}\totu{k}\n` per row, counted from 1.  Buffer protocol of rtx_tally_format_fasta.
 *   RTX_DEFAULT_UNOISE_SLICE (rtx_set_default_option; default and 0: no cap): a cap on the rows of one launch of the pair kernel and on the
 *                centroids of one launch, read at every call.  For tests: the result does not depend on it. */
#define RTX_DEFAULT_UNOISE_SLICE 8 /* (7 stays unknown: the suite of the de novo check pins it as the first id that is refused) */
#define RTX_UNOISE_MAX_DIFFS 16
#define RTX_UNOISE_ZOTU 0
#define RTX_UNOISE_ABSORBED 1
#define RTX_UNOISE_LEFT 2
#define RTX_UNOISE_LONG 3
typedef struct rtx_unoise_params {
    uint64_t minsize;   /* at least 1 (8 when params is NULL) */
    uint32_t alpha;     /* 1 .. 8 (2 when params is NULL) */
    uint32_t max_diffs; /* 0: RTX_UNOISE_MAX_DIFFS; at most 16 */
    uint32_t flags;     /* 0 */
} rtx_unoise_params;
typedef struct rtx_unoise_view_t {
    uint64_t n_rows;
    const uint8_t *status;   /* [n_rows] RTX_UNOISE_* */
    const uint32_t *parent;  /* [n_rows] a row, or RTX_NO_REF */
    const uint32_t *dist;    /* [n_rows] d(row, parent), or RTX_NO_DIST */
    const uint32_t *lim;     /* [n_rows] */
    uint64_t n_zotu, n_absorbed, n_left, n_long;
    uint64_t minsize;        /* the parameters as used */
    uint32_t alpha, max_diffs;
    uint32_t tiers, launches;                       /* device only from here on; 0 for a host result */
    uint64_t pairs, pairs_length, pairs_finished;   /* pairs handed to the kernel, dropped by the length test, that reached the last column */
    double seconds[4];                              /* upload, pair kernels (events around them), bookkeeping, download */
} rtx_unoise_view_t;
int rtx_otu_unoise(int device, rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out);
int rtx_otu_unoise_host(rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out);
int rtx_otu_unoise_view(rtx_otu *denoised, rtx_unoise_view_t *view);
int64_t rtx_otu_format_unoise(rtx_otu *denoised, char *buf, uint64_t cap);

/* ---- Consensus taxonomy of the OTUs (rtx_otutax.hip, host_otutax.cpp) ------------------------------------------------------------------------
 * Which taxon an OTU is: the deepest taxon that an agreed share of the OTU's reads reaches with confidence, with the support at every level.
 * Exact, integers only, independent of scheduling.
 *   record       of a row r: what the taxon profile takes of a query (rtx_index_profile_begin) under a cutoff c -- kind[r], RTX_LIN_*; L[r], the
 *                leading levels of its best lineage whose confidence reaches c; node[r] = a_{L-1}; hund[r][0 .. L), their hundredths.  The
 *                path a_0 .. a_{L-1} follows from node[r] over node_parent, a_0 a child of the root; L == 0 for the kinds that are not
 *                classified (node and hund are then not read).  rtx_result_best_lineages makes the records of a batch from its download.
 *   weight       w_r, the reads a row stands for (rtx_tally_view.sizes), at least 1.
 *   size         S_k = the sum of w_r over ALL rows with otu[r] == k, whatever their kind (rtx_otu_view_t.sizes[k]); members[k] counts them.
 *   clade        clade_k[n] = the sum of w_r over the members of k whose path contains node n; conf_k[n] = the sum of w_r x hund[r][d] over
 *                the same members, d the level of n.
 *   consensus    under an agreement percentage P, 51 <= P <= 100: start at the root; descend to the child n with clade_k[n] x 100 >= P x S_k;
 *                stop where no child qualifies.  P > 50: at most one child qualifies, there are no ties and no tie rule.
 *   result       per OTU: depth[k] (may be 0); node[k], the last node of the walk, 0 (the root) at depth 0; clade[k][d] and conf[k][d] for
 *                d < depth[k] (0 from there to `stride`, the deepest L of the call, at least 1); classified[k] = the sum of w_r over the
 *                members of kind RTX_LIN_CLASSIFIED; seed_rel[k], how the path of row seed[k] relates to the consensus path: 0 equal, 1 the
 *                consensus is a proper prefix of the seed's path, 2 the seed's path is a proper prefix of the consensus, 3 they diverge.
 *                Nothing is said about the level where the walk stops: without a majority there is no well-defined runner-up.
 *   refused      RTX_ERR_INVALID, on the host, before anything is uploaded: a null array; P outside 51 .. 100; flags != 0; 2^32 - 1 rows or
 *                more; an OTU number >= n_otus; an OTU without a row (its S_k would be 0); a seed >= n_rows; a weight of 0; 100 x the sum of all weights >= 2^64; a kind above 2; L != 0
 *                on a row that is not classified, or L == 0 on one that is; L above RTX_MAX_DEPTH or hund_stride; a node id >= n_nodes; an L
 *                that is not the depth of its node (above it there is no such path, below it the node is not a_{L-1}); a hundredths value
 *                above 100; a node_parent that is not below its node (the nodes come breadth first, the root is node 0).  Of the
 *                rtx_nodes_view only n_nodes and node_parent are read.
 *   rtx_otu_taxonomy       on GPU `device` (RTX_ERR_NO_DEVICE without a gfx950).  A kernel writes every row's path; the host lays the members
 *                out per OTU (rank order) and packs consecutive OTUs of at most 64 members into one wave while their members total at most
 *                64 (packed_waves); every larger OTU takes a workgroup of its own (big_otus).  Level by level the members still on the
 *                consensus path name their node; a one-counter majority summary picks the candidate, the candidate's clade and conf are
 *                summed exactly in 64 bits, and the test above decides.  No atomics: one lane writes an OTU's result.
 *   rtx_otu_taxonomy_host  the definition restated: per OTU a map node -> (clade, conf) over all members' paths, then the descent.  Equal to
 *                the device's result field by field, except packed_waves and big_otus (0) and the times.
 *   rtx_otu_taxonomy_view  valid until the object is destroyed.  rtx_otu_taxonomy_times: seconds of checks, plan and upload, the path kernel,
 *                the consensus kernels, the download; all 0 for a host result.
 *   rtx_otu_taxonomy_format  "#otu<TAB>size<TAB>members<TAB>classified<TAB>depth<TAB>taxon<TAB>lineage<TAB>support<TAB>mean_conf<TAB>seed", then one line
 *                per OTU whose size reaches minsize, `otu{k}` counted from 1 as rtx_otu_format_fasta counts: lineage = the first `depth`
 *                levels of lineages[node_begin[node]], taxon = the last of them (as rtx_profile_format prints them); support = per level
 *                (clade x 10000 + S / 2) / S with two decimals, comma-separated; mean_conf = per level (conf + clade / 2) / clade hundredths
 *                likewise; seed = one of `= < > x` for seed_rel 0 .. 3; a depth of 0 prints `-` in the four taxonomy columns.  Every line
 *                ends in '\n'.  `tree` must be the tree of the nodes (RTX_ERR_INVALID when the node counts differ).  Buffer protocol of
 *                rtx_profile_format.
 *   rtx_result_best_lineages  the records of the n_queries of a download, by the per-query step of the taxon profile itself: cutoff 1 .. 100,
 *                flags RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE (either one: no override), exact_ids / exact_off the exact matches of the
 *                batch (rtx_batch_exact_matches) or NULL / NULL: no query has one.  kind, L, node: [n_queries]; hund: [n_queries][hund_stride],
 *                zero from L on; hund_stride at least the deepest lineage of the tree.  A view without the byte arrays (hand-made) has its
 *                confidences converted as rtx_result_pack converts them.  No device involved. */
#define RTX_LIN_UNCLASSIFIABLE 0u
#define RTX_LIN_UNCLASSIFIED 1u
#define RTX_LIN_CLASSIFIED 2u
typedef struct rtx_otutax rtx_otutax;
typedef struct rtx_lineage_records {
    const uint8_t *kind;  /* [n_rows] RTX_LIN_* */
    const uint8_t *L;     /* [n_rows] */
    const uint32_t *node; /* [n_rows] a_{L-1} */
    const uint8_t *hund;  /* [n_rows][hund_stride] */
    uint32_t hund_stride;
} rtx_lineage_records;
typedef struct rtx_otu_taxonomy_params {
    uint32_t agree_pct; /* 51 .. 100; 0: 51 */
    uint32_t flags;     /* 0 */
} rtx_otu_taxonomy_params;
typedef struct rtx_otu_taxonomy_view_t {
    uint64_t n_rows, n_otus;
    uint32_t n_nodes, agree_pct;
    uint32_t stride;            /* levels per OTU in clade and conf */
    const uint64_t *sizes;      /* [n_otus] S_k */
    const uint64_t *members;    /* [n_otus] rows */
    const uint64_t *classified; /* [n_otus] */
    const uint32_t *depth;      /* [n_otus] */
    const uint32_t *node;       /* [n_otus] */
    const uint8_t *seed_rel;    /* [n_otus] 0 .. 3 */
    const uint64_t *clade;      /* [n_otus x stride] */
    const uint64_t *conf;       /* [n_otus x stride] */
    uint64_t packed_waves, big_otus; /* the device's plan; host: 0 */
} rtx_otu_taxonomy_view_t;
int rtx_otu_taxonomy(int device, uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed,
                     const rtx_lineage_records *records, const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out);
int rtx_otu_taxonomy_host(uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed,
                          const rtx_lineage_records *records, const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out);
int rtx_otu_taxonomy_view(rtx_otutax *tax, rtx_otu_taxonomy_view_t *view);
int rtx_otu_taxonomy_times(const rtx_otutax *tax, double seconds[4]);
void rtx_otu_taxonomy_destroy(rtx_otutax *tax);
int64_t rtx_otu_taxonomy_format(rtx_otutax *tax, const rtx_tree *tree, uint64_t minsize, char *buf, uint64_t cap);
int rtx_result_best_lineages(const rtx_tree *tree, const rtx_result_view *res, const uint32_t *exact_ids, const uint64_t *exact_off, uint32_t cutoff_hundredths,
                             uint32_t flags, uint8_t *kind, uint8_t *L, uint32_t *node, uint8_t *hund, uint32_t hund_stride);

/* ---- primer trimming (rtx_trim.hip; rtx_index_set_primers is the host mirror's use of it) ---------------------------------------------------
 * Amplicon reads come with their PCR primers attached, the references without: what `cutadapt` is run for in front of a classifier, on the
 * device.  Exact integers; the host function and the device agree bit for bit.
 *   bytes        one per base, codes 1 .. 15.  Two bytes match when both are codes and share a bit (IUPAC degeneracy is an AND); a read
 *                byte that is 0 or above 15 matches nothing; a pattern byte must be a code.
 *   search(p, x, w, k)   p: m codes, 1 <= m <= RTX_TRIM_MAX_PATTERN; X = x[0 .. min(len(x), w)).  E[j], j = 0 .. len(X): the least
 *                Levenshtein distance (substitution, insertion, deletion 1 each) of the WHOLE pattern to X[i .. j) over 0 <= i <= j -- the text
 *                in front of the match is free, E[0] = m.  e = min E[j]; j* = the LARGEST j with E[j] == e; found iff e <= k (k < m).
 *   5' pattern   (j*, e) = search(p, x, w, k): the read loses x[0 .. j*).
 *   3' pattern   given as it reads on the read, 5'->3': (j*, e) = search(reverse(p), reverse(x), w, k), the read loses its last j* bases
 *                (the tie rule cuts the most at either end).
 *   several patterns of one end: among the found ones the least e wins, then the lowest index in the list.  The two ends are searched
 *                independently on the untrimmed read.
 *   per read     lo = the 5' cut or 0; hi = len - the 3' cut, or len; hi < lo: hi = lo (the read is left empty);
 *                hit = pat5 | err5 << 8 | pat3 << 16 | err3 << 24, pattern RTX_TRIM_NO_PATTERN and errors 0 where nothing was found.
 *                Never depends on the rest of the batch.
 *   window       0: min(RTX_TRIM_MAX_WINDOW, m + max_errors + 32).
 *   rtx_trim_create   an object of its own on GPU `device` like rtx_derep: one stream, its own buffers (they only grow), no rtx_index, a
 *                copy of the patterns.  Checked in this order: null arguments, n == 0 or n > RTX_TRIM_MAX_PATTERNS, every pattern (a byte that
 *                is no code, len 0 or above RTX_TRIM_MAX_PATTERN, max_errors >= len, window above RTX_TRIM_MAX_WINDOW, an unknown end):
 *                RTX_ERR_INVALID; then the device: RTX_ERR_NO_DEVICE without a gfx950.
 *   rtx_trim_run      lo / hi / hit of n reads, [n] each; bases / base_off as rtx_batch_prefetch takes them.  Only the ends of the reads
 *                travel to the device.  n == 0: RTX_OK; a base_off that is not monotone or a read of 2^32 bases or more: RTX_ERR_INVALID.
 *                Synchronous; calls on one object are serialised by the caller.
 *   rtx_primer_search the search of ONE pattern in one read on the host (no device), with the function the kernel calls: *cut = j*,
 *                *errors = e; *cut = 0 and *errors = RTX_NO_DIST when not found.  RTX_ERR_INVALID as rtx_trim_create refuses a pattern.
 *   rtx_trim_apply    host: the kept ranges [lo, hi) of the reads back to back into out_bases (room for the sum of hi - lo, at most the
 *                input's bytes) with out_off[n + 1] from 0.  RTX_ERR_INVALID unless lo <= hi <= the read's length.
 *   rtx_index_set_primers  the patterns rtx_raxtax* trim every read with before anything else sees it (n == 0, the default: off -- no new
 *                code runs, nothing is allocated, every output is what it is without).  Like RTX_OPT_DEREP honoured by the mirror alone
 *                (rtx_batch_* and rtx_classify_batch ignore it), shapes no workspace, drops no uploaded batch; the handle keeps a copy.  The
 *                handles of one call must hold the same list: RTX_ERR_INVALID otherwise.  The stage runs in front of dereplication; exact
 *                matches, the `.tsv` sequence column and the identity's qlen are those of the trimmed read; an emptied read is classified
 *                as the empty read.  rtx_index_primers: how many it holds.
 *   rtx_raxtax_last_trim  the last rtx_raxtax* call of the process: its queries, those with a 5' primer, with a 3' primer, those left
 *                empty (hi == lo of a read that had bases) and the busy seconds of the stage; all 0 with no primers set. */
#define RTX_TRIM_5P 0u
#define RTX_TRIM_3P 1u
#define RTX_TRIM_MAX_PATTERNS 8
#define RTX_TRIM_MAX_PATTERN 64
#define RTX_TRIM_MAX_WINDOW 256
#define RTX_TRIM_NO_PATTERN 0xFFu
typedef struct { const uint8_t *codes; uint32_t len, end, max_errors, window; } rtx_trim_pattern;
typedef struct rtx_trim rtx_trim;
int rtx_trim_create(int device, const rtx_trim_pattern *pats, uint32_t n, rtx_trim **out);
int rtx_trim_run(rtx_trim *t, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *lo /*[n]*/, uint32_t *hi /*[n]*/, uint32_t *hit /*[n]*/);
void rtx_trim_destroy(rtx_trim *t);
int rtx_trim_kernel_time(const rtx_trim *t, float *ms); /* milliseconds of the kernel of the last rtx_trim_run, from HIP events around it */
int rtx_primer_search(const uint8_t *p, uint32_t m, const uint8_t *x, uint64_t n, uint32_t end, uint32_t window, uint32_t max_errors,
                      uint32_t *cut, uint32_t *errors);
int rtx_trim_apply(uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *lo, const uint32_t *hi, uint8_t *out_bases,
                   uint64_t *out_off /*[n + 1]*/);
int rtx_index_set_primers(rtx_index *index, const rtx_trim_pattern *pats, uint32_t n);
int rtx_index_primers(const rtx_index *index, uint32_t *n);
int rtx_raxtax_last_trim(uint64_t *queries, uint64_t *with5, uint64_t *with3, uint64_t *emptied, double *busy_seconds);

/* ---- sample demultiplexing (rtx_demux.hip) -------------------------------------------------------------------------------------------------
 * Pooled amplicon libraries carry a short tag in front of each primer that names the PCR, and with it the sample: what OBITools `ngsfilter`,
 * `cutadapt -g file:tags.fasta` or `vsearch --fastx_demux` are run for, on the device.  Exact integers; the host function and the device
 * agree bit for bit.
 *   bytes        as in the primer trimming: codes 1 .. 15, two bytes match when both are codes and share a bit; a read byte that is 0 or
 *                above 15 matches nothing; a tag byte must be a code.
 *   placement    a tag of m codes at offset s (0 <= s <= max_offset, s + m <= len) covers the read's positions s .. s + m - 1; its distance
 *                d is the number of positions that do not match.  Substitutions only: tags are designed in Hamming space, an insertion or
 *                deletion inside a tag is NOT found (out of scope).  The offsets are for the heterogeneity spacers of 0 .. N bases in front
 *                of a tag.
 *   3' tag       given as it reads on the read, 5'->3'; the offset counts from the read's end, the tag covers [len - s - m, len - s): the 5'
 *                problem of the reversed read.
 *   one end      d* = the least d over all tags of that end and all admissible offsets (none admissible: nothing is found).  The end is
 *                FOUND iff d* <= max_mismatches; it is AMBIGUOUS iff it is found and two different tags of it reach d*, at any offsets;
 *                otherwise its tag is the one that reaches d*, at its least offset.  An end HAS A TAG when it is found and not
 *                ambiguous.  An end with no tags in the list is not searched and cuts nothing.
 *   verdict      the first that applies: RTX_DEMUX_AMBIGUOUS (3) either end is ambiguous; RTX_DEMUX_NO_TAG5 (1) the list has 5' tags and
 *                none was found; RTX_DEMUX_NO_TAG3 (2) the same for 3'; RTX_DEMUX_UNKNOWN_PAIR (4) (tag5, tag3) is no pair of the table
 *                (an end without tags in the list pairs as RTX_DEMUX_NO_TAG); RTX_DEMUX_OK (0).
 *   per read     sample = the pair's sample when the verdict is RTX_DEMUX_OK, else RTX_DEMUX_NONE; lo = s5 + m5 where the 5' end has a
 *                tag, else 0; hi = len - (s3 + m3) where the 3' end has one, else len; hi < lo: hi = lo (the read is left empty);
 *                hit = tag5 | tag3 << 16 (places in the tag list, RTX_DEMUX_NO_TAG for an end that has none);
 *                info = verdict | d5 << 8 | d3 << 16 | s5 << 24 | s3 << 28, zeros for an end that has no tag.
 *                Never depends on the rest of the batch.
 *   pairs        tag5 names a 5' tag and tag3 a 3' tag of the list; either, not both, may be RTX_DEMUX_NO_TAG (single-ended: it pairs
 *                only while the list has no tag of that end); sample is any value but RTX_DEMUX_NONE.
 *   rtx_demux_create  an object of its own on GPU `device` like rtx_trim: one stream, its own buffers (they only grow), no rtx_index, a
 *                copy of the tags and a dense pair table.  Checked in this order: null arguments; n_tags == 0 or more than
 *                RTX_DEMUX_MAX_TAGS on one end; every tag (len 0 or above RTX_DEMUX_MAX_TAG, a byte that is no code, an unknown end);
 *                parameters above RTX_DEMUX_MAX_MISMATCHES / RTX_DEMUX_MAX_OFFSET; every pair (a tag out of range or of the wrong end,
 *                both RTX_DEMUX_NO_TAG, sample RTX_DEMUX_NONE); the same (tag5, tag3) twice: RTX_ERR_INVALID; then the device:
 *                RTX_ERR_NO_DEVICE without a gfx950.
 *   rtx_demux_run     sample / lo / hi / hit / info of n reads, [n] each; bases / base_off as rtx_batch_prefetch takes them.  Only the
 *                first and last max_offset + 32 bases of a read travel to the device.  n == 0: RTX_OK; a base_off that is not monotone,
 *                a read of 2^32 bases or more, n > 2^31 - 2: RTX_ERR_INVALID.  Synchronous; calls on one object are serialised by the
 *                caller.
 *   rtx_demux_read    one read on the host (no device), with the function the kernel calls; the checks of rtx_demux_create.
 *   rtx_index_set_tags  the tag list rtx_raxtax* demultiplex every read with before anything else sees it (n_tags == 0, the default: off --
 *                no new code runs, nothing is allocated, every output is what it is without; otherwise the checks of rtx_demux_create).
 *                Like rtx_index_set_primers honoured by the mirror alone, the handle keeps a copy, and the handles of one call must hold
 *                the same list: RTX_ERR_INVALID otherwise.  The stage stands behind the merging of read pairs and in front of the primer
 *                trimming: the chunk's own copies of the bases (and qualities) are cut to [lo, hi) first, so trimming, quality filter,
 *                dereplication and chimera check run unchanged on the cut read and their callbacks report positions in it.  A read
 *                whose verdict is not RTX_DEMUX_OK is reported and not classified: it goes on as the empty read, as a discarded or
 *                flagged read does.  Where a profile with samples is open (rtx_index_profile_begin_samples) every chunk's samples are
 *                staged with rtx_batch_prefetch_samples.  Tags together with RTX_OPT_DEREP and an open profile: RTX_ERR_INVALID
 *                (copies from different samples would be counted as one read); tags with RTX_OPT_DEREP alone are allowed.
 *                rtx_index_tags: how many tags it holds. */
#define RTX_DEMUX_MAX_TAGS 1024 /* per end */
#define RTX_DEMUX_MAX_TAG 32    /* codes per tag */
#define RTX_DEMUX_MAX_OFFSET 15
#define RTX_DEMUX_MAX_MISMATCHES 8
#define RTX_DEMUX_NO_TAG 0xFFFFu
#define RTX_DEMUX_NONE 0xFFFFFFFFu /* no sample */
#define RTX_DEMUX_OK 0u
#define RTX_DEMUX_NO_TAG5 1u
#define RTX_DEMUX_NO_TAG3 2u
#define RTX_DEMUX_AMBIGUOUS 3u
#define RTX_DEMUX_UNKNOWN_PAIR 4u
typedef struct { const uint8_t *codes; uint32_t len, end; } rtx_demux_tag;  /* end: RTX_TRIM_5P / RTX_TRIM_3P */
typedef struct { uint32_t tag5, tag3, sample; } rtx_demux_pair;             /* places in the tag list */
typedef struct { uint32_t max_mismatches, max_offset; } rtx_demux_params;
typedef struct rtx_demux rtx_demux;
int rtx_demux_create(int device, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                     const rtx_demux_params *params, rtx_demux **out);
int rtx_demux_run(rtx_demux *d, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *sample /*[n]*/, uint32_t *lo /*[n]*/,
                  uint32_t *hi /*[n]*/, uint32_t *hit /*[n]*/, uint32_t *info /*[n]*/);
void rtx_demux_destroy(rtx_demux *d);
int rtx_demux_kernel_time(const rtx_demux *d, float *ms); /* milliseconds of the kernel of the last rtx_demux_run, from HIP events around it */
int rtx_index_set_tags(rtx_index *index, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                       const rtx_demux_params *params);
int rtx_index_tags(const rtx_index *index, uint32_t *n_tags);
int rtx_demux_read(const rtx_demux_params *params, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                   const uint8_t *read, uint64_t len, uint32_t *sample, uint32_t *lo, uint32_t *hi, uint32_t *hit, uint32_t *info);

/* ---- quality filter (rtx_qual.hip; rtx_index_set_quality is the host mirror's use of it) -----------------------------------------------------
 * The step that starts an amplicon pipeline (`vsearch --fastq_filter`, DADA2 `filterAndTrim`) on the device: where a read is cut and whether
 * it is discarded, from its FASTQ quality string.  Exact integers; the host function, the x86 emulator and the device agree bit for bit.
 *   table        e[Q] = llround(10^(-Q/10) * 2^40), Q = 0 .. 93 (e[0] = 2^40, e[93] = 551): computed once on the host, the kernel receives
 *                that array; rtx_qual_error_table hands it out.  A threshold given as a double x is floor(x * 2^40), at most 2^63: that
 *                integer is compared.  A read has at most RTX_QUAL_MAX_READ bases, so no sum exceeds 2^60.
 *   parameters   ascii_base 33 or 64; every other field has a value that switches it off, and a struct that is entirely off is no filter:
 *                  trunc_len    0   a range shorter than this is discarded (and left as long as it is); otherwise it is cut to this length
 *                  trunc_qual  <0   cut in front of the first base with Q <= this (at most 93)
 *                  trunc_ee    <0   cut in front of the first base at which the sum of e from the start of the range, that base included,
 *                                   is above this
 *                  min_len      0   discard if fewer bases are kept
 *                  max_len      0   discard if more bases are kept
 *                  max_ns      <0   discard if the kept bases hold more bases that are none of A, C, G, T (codes 1, 2, 4, 8) than this
 *                  max_ee      <0   discard if the expected errors of the kept bases -- the sum of their e -- are above this
 *                  max_ee_rate <0   discard if they are above this times the number of kept bases
 *                RTX_ERR_INVALID: a NaN, an ascii_base other than 33 or 64, a trunc_qual above 93.
 *   per read     the input range [lo, hi_in) -- the whole read, or what the primer trimming kept; Q_i = qual_i - ascii_base.
 *                1. a byte of the range with Q_i outside 0 .. 93: the verdict is RTX_QC_BAD_QUALITY alone, hi = lo, ee = 0.
 *                2. trunc_len; 3. trunc_qual and trunc_ee, each within what trunc_len left: the shorter result wins.  hi: the end of what
 *                is kept; ee: the sum of e over [lo, hi); 4. the verdict is the OR of EVERY reason that applies (RTX_QC_*), 0: the read
 *                passes.  hi and ee are given for a discarded read as well.  Never depends on the rest of the batch.
 *   rtx_qual_create   an object of its own on GPU `device` like rtx_trim: one stream, its own buffers (they only grow), no rtx_index.
 *                Checked in this order: null arguments, the parameters (RTX_ERR_INVALID), the device (RTX_ERR_NO_DEVICE without a gfx950).
 *   rtx_qual_run      hi / ee / verdict of n reads, [n] each; bases / base_off as rtx_batch_prefetch takes them, quals indexed like bases
 *                (raw bytes: rtx_queries_quals); lo_in / hi_in [n] or both NULL (whole reads).  One byte per base of the ranges travels to
 *                the device -- the quality byte, bit 7 set where the base is no A/C/G/T -- and an offset and a length per read.  n == 0:
 *                RTX_OK; RTX_ERR_INVALID: a base_off that is not monotone, a range outside its read, a read of more than RTX_QUAL_MAX_READ
 *                bases, a quality byte of 128 or more in a range.  Synchronous; calls on one object are serialised by the caller.
 *   rtx_qual_stage_times  seconds of the last rtx_qual_run: the host's staging pass, the copies and the wait around the kernel, all of it.
 *   rtx_qual_read     the same for ONE read on the host (no device), with the functions the kernel calls.
 *   rtx_index_set_quality  the filter rtx_raxtax* run every read through (NULL or a struct that is entirely off, the default: off -- no
 *                new code runs, nothing is allocated, every output is what it is without).  Like the primers honoured by the mirror alone,
 *                shapes no workspace; the handles of one call must hold the same setting and the call must bring quals
 *                (rtx_raxtax_multi_ex5): RTX_ERR_INVALID otherwise.  Primers are trimmed first, on the raw read; the filter runs on the
 *                range they kept; dereplication comes last.  A discarded read is classified as the empty read: no message, no `align`
 *                callback, not counted by an open profile.  rtx_index_quality: the setting and whether it is on.
 *   rtx_raxtax_last_qual  the last rtx_raxtax* call of the process: its queries, those that passed, those that passed and were cut short
 *                by the filter, how often each reason applied (reasons[b]: bit b of the verdict) and the busy seconds of the stage;
 *                all 0 with the filter off. */
#define RTX_QUAL_MAX_READ (1u << 20)
#define RTX_QUAL_TABLE 94
#define RTX_QC_BAD_QUALITY 1u
#define RTX_QC_SHORT_FOR_TRUNC_LEN 2u
#define RTX_QC_TOO_SHORT 4u
#define RTX_QC_TOO_LONG 8u
#define RTX_QC_TOO_MANY_N 16u
#define RTX_QC_MAX_EE 32u
#define RTX_QC_MAX_EE_RATE 64u
typedef struct {
    uint32_t ascii_base, trunc_len;
    int32_t trunc_qual;
    double trunc_ee;
    uint32_t min_len, max_len;
    int32_t max_ns;
    double max_ee, max_ee_rate;
} rtx_qual_params;
typedef struct rtx_qual rtx_qual;
int rtx_qual_error_table(uint64_t out[RTX_QUAL_TABLE]);
int rtx_qual_create(int device, const rtx_qual_params *params, rtx_qual **out);
int rtx_qual_run(rtx_qual *q, uint64_t n, const uint8_t *bases, const uint8_t *quals, const uint64_t *base_off, const uint32_t *lo_in /*[n] or NULL*/,
                 const uint32_t *hi_in /*[n] or NULL*/, uint32_t *hi_out /*[n]*/, uint64_t *ee_out /*[n]*/, uint32_t *verdict_out /*[n]*/);
void rtx_qual_destroy(rtx_qual *q);
int rtx_qual_kernel_time(const rtx_qual *q, float *ms); /* milliseconds of the kernel of the last rtx_qual_run, from HIP events around it */
int rtx_qual_stage_times(const rtx_qual *q, double seconds[3]);
int rtx_qual_read(const rtx_qual_params *params, const uint8_t *bases, const uint8_t *quals, uint64_t len, uint32_t lo, uint32_t hi_in,
                  uint32_t *hi_out, uint64_t *ee_out, uint32_t *verdict_out);
int rtx_index_set_quality(rtx_index *index, const rtx_qual_params *params);
int rtx_index_quality(const rtx_index *index, rtx_qual_params *params, int *on);
int rtx_raxtax_last_qual(uint64_t *queries, uint64_t *passed, uint64_t *truncated, uint64_t reasons[7], double *busy_seconds);

/* ---- contaminant screen (rtx_screen.hip; host_screen.cpp has the set and the host function; rtx_index_set_screen is the host mirror's use) ----
 * The step that takes PhiX, organelle and vector reads out of an amplicon run (DADA2 `rm.phix`, `bbduk`) on the device: the 16-mers of a read
 * looked up in a set of canonical 16-mers.  Exact integers; the host function, the x86 emulator and the device agree bit for bit.
 *   window       RTX_SCREEN_K = 16.  A window at position p of a range is VALID iff its 16 codes are each one of 1, 2, 4, 8 (the parsers'
 *                4-bit codes); anything else -- IUPAC unions, 0 -- breaks every window it lies in.  Its value w is the 32-bit word of the
 *                2-bit codes A 0, C 1, G 2, T 3, the first base in the most significant bits, as the classifier packs its 8-mers.  rc(w)
 *                is the value of the reverse complement: its base j is 3 - base 15 - j.  The CANONICAL value is c = min(w, rc(w)).  No
 *                canonical value is 0xFFFFFFFF (rc of sixteen T is 0): that word marks an empty slot.
 *   set          from n contaminant sequences, bases / base_off like references: S, the distinct canonical values of all their valid
 *                windows; src(c), the lowest index of a sequence that holds c.  RTX_ERR_INVALID: a base_off that is not monotone, more
 *                than RTX_SCREEN_MAX_BASES bases in total (checked from base_off before a base is read), no valid window at all.
 *   table        m slots {key, src}, m the smallest power of two with m >= 2 |S| and m >= 1024.  The home slot of c is
 *                h(c) = (uint32)(c * 0x9E3779B1) >> (32 - log2 m); the keys are inserted in ascending order of c with linear probing
 *                modulo m; a lookup walks from h(c) until it finds c or an empty slot.  rtx_screen_set_info: |S|, m, the longest
 *                displacement of a stored key, the number of keys stored below their home slot (their chain wrapped), and a 64-bit
 *                fingerprint of the keys and their sources (any pointer may be NULL).  rtx_screen_set_table hands the slots out.
 *   parameters   min_hits (default 2, at least 1), min_pct (default 50, 0 .. 100); RTX_ERR_INVALID otherwise.
 *   per read     over the input range [lo, hi) -- the whole read, or what primers and quality kept: windows, the number of valid windows;
 *                hits, the number of valid windows whose canonical value is in S (positions are counted, not distinct values); first,
 *                the position, counted from lo, of the hitting window at the lowest position, RTX_SCREEN_NONE without one; source, src
 *                of that window, or RTX_SCREEN_NONE; verdict, RTX_SCREEN_CONTAMINANT iff hits >= min_hits and
 *                100 * hits >= min_pct * windows (compared in 64 bits), 0 otherwise.  A range shorter than 16 has windows = hits = 0 and
 *                passes.  Never depends on the rest of the batch, nor on the orientation in which the read is given (first and source
 *                speak of the read as given).
 *   rtx_screen_set_build  the set as an immutable host object holding the table, built on the host (at most 2^26 keys are sorted).
 *   rtx_screen_create  an object of its own on GPU `device` like rtx_qual: one stream, its own buffers (they only grow), the table uploaded
 *                once; the set may be freed afterwards.  Checked in this order: null arguments, the parameters (RTX_ERR_INVALID), the
 *                device (RTX_ERR_NO_DEVICE without a gfx950).
 *   rtx_screen_run    windows / hits / first / source / verdict of n reads, [n] each; bases / base_off as rtx_batch_prefetch takes them;
 *                lo_in / hi_in [n] or both NULL (whole reads).  One byte per base of the ranges travels to the device and an offset and a
 *                length per read.  n == 0: RTX_OK; RTX_ERR_INVALID: a base_off that is not monotone, a range outside its read, a read of
 *                more than RTX_SCREEN_MAX_READ bases.  Synchronous; calls on one object are serialised by the caller.
 *   rtx_screen_stage_times  seconds of the last rtx_screen_run: the host's staging pass, the copies and the wait around the kernel, all of it.
 *   rtx_screen_read   the same for ONE read on the host (no device), with the functions the kernel calls.
 *   rtx_index_set_screen  the screen rtx_raxtax* run every read through (NULL set, the default: off -- no new code runs, nothing is
 *                allocated, every output is what it is without).  The handle keeps what it needs: the caller may free the set.  Like the
 *                primers and the quality filter honoured by the mirror alone, shapes no workspace; the handles of one call must hold
 *                the same set and parameters (a 64-bit fingerprint of the keys and the two parameters is compared): RTX_ERR_INVALID
 *                otherwise.  The stage runs behind the quality filter, on the range primers and quality kept, and in front of the
 *                dereplication.  rtx_index_screen: the parameters, whether it is on, and that fingerprint (0 when off).
 *   rtx_raxtax_last_screen  see rtx_raxtax_multi_ex8. */
#define RTX_SCREEN_K 16u
#define RTX_SCREEN_NONE 0xFFFFFFFFu
#define RTX_SCREEN_MAX_READ (1u << 20)
#define RTX_SCREEN_MAX_BASES (1ull << 26)
#define RTX_SCREEN_CONTAMINANT 1u
typedef struct {
    uint32_t min_hits, min_pct;
} rtx_screen_params;
typedef struct rtx_screen_set rtx_screen_set;
typedef struct rtx_screen rtx_screen;
int rtx_screen_set_build(uint64_t n_seqs, const uint8_t *bases, const uint64_t *base_off /*[n_seqs + 1]*/, rtx_screen_set **out);
void rtx_screen_set_free(rtx_screen_set *set);
int rtx_screen_set_info(const rtx_screen_set *set, uint64_t *n_keys, uint64_t *n_slots, uint64_t *max_displacement, uint64_t *n_wrapped, uint64_t *fingerprint);
int rtx_screen_set_table(const rtx_screen_set *set, const uint32_t **slots /*[2 m]: key, src per slot; valid as long as the set*/, uint32_t *log2m);
int rtx_screen_create(int device, const rtx_screen_set *set, const rtx_screen_params *params, rtx_screen **out);
int rtx_screen_run(rtx_screen *s, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *lo_in /*[n] or NULL*/,
                   const uint32_t *hi_in /*[n] or NULL*/, uint32_t *windows /*[n]*/, uint32_t *hits /*[n]*/, uint32_t *first /*[n]*/,
                   uint32_t *source /*[n]*/, uint32_t *verdict /*[n]*/);
void rtx_screen_destroy(rtx_screen *s);
int rtx_screen_kernel_time(const rtx_screen *s, float *ms); /* milliseconds of the kernel of the last rtx_screen_run, from HIP events around it */
int rtx_screen_stage_times(const rtx_screen *s, double seconds[3]);
int rtx_screen_read(const rtx_screen_set *set, const rtx_screen_params *params, const uint8_t *bases, uint64_t len, uint32_t lo, uint32_t hi,
                    uint32_t *windows, uint32_t *hits, uint32_t *first, uint32_t *source, uint32_t *verdict);
int rtx_index_set_screen(rtx_index *index, const rtx_screen_set *set, const rtx_screen_params *params);
int rtx_index_screen(const rtx_index *index, rtx_screen_params *params, int *on, uint64_t *fingerprint);

/* ---- paired-end merging (rtx_merge.hip; host_merge.cpp has the host function) ---------------------------------------------------------------
 * The first step of an amplicon pipeline (`vsearch --fastq_mergepairs`, PEAR, DADA2 `mergePairs`) on the device: the two mates of a pair
 * overlapped into one read.  Exact integers, no tolerance anywhere; the host function, the x86 emulator and the device agree bit for bit.
 * Still ABI 6: exports only, nothing that exists changes.
 *   per pair     the forward mate F (nf base codes and raw quality bytes) and the reverse mate R (nr of each).  Codes are the 4-bit codes of
 *                the parsers (A=1, C=2, G=4, T=8, IUPAC codes as unions, 0 for anything else; a byte above 15 counts as 0).  R' is the
 *                reverse complement of R as rtx_revcomp defines it, its quality bytes reversed.  Q = byte - ascii_base.
 *   parameters   ascii_base 33 (33 or 64), min_overlap 16 (at least 1), max_diffs 10, max_diff_pct 100 (0 .. 100), q_cap 41 (0 .. 93);
 *                RTX_ERR_INVALID otherwise.  The cost of a mismatch is the constant RTX_MERGE_MISMATCH_COST.
 *   verdict      the first of these that applies, and only that one: RTX_MG_BAD_QUALITY -- a byte of either mate, anywhere, with Q outside
 *                0 .. 93; RTX_MG_TOO_LONG -- a mate of more than RTX_MERGE_MAX_READ bases; RTX_MG_TOO_SHORT -- a mate of fewer than
 *                min_overlap bases; RTX_MG_NO_OVERLAP -- no candidate is accepted; 0 -- merged.  A pair that is not merged has overlap =
 *                diffs = 0 and the empty merged read.
 *   candidates   no gaps, no staggered alignments: ov = min_overlap .. min(nf, nr), F[nf - ov + i] against R'[i] for i in [0, ov).  d(ov) is
 *                the number of positions with (a & b) == 0, score = ov - RTX_MERGE_MISMATCH_COST * d.  A candidate is accepted iff
 *                d <= max_diffs, 100 * d <= max_diff_pct * ov and score >= min_overlap.  The largest score wins, among equal scores the
 *                larger ov.
 *   merged read  nf + nr - ov bases under the forward mate's label.  In front of the overlap F, behind it R', codes and quality bytes as
 *                they are.  Inside, with a, qa of F and b, qb of R':  a == b and a != 0: code a, Q = max(max(qa, qb), min(qa + qb, q_cap));
 *                otherwise (a & b) != 0: code a & b, Q = max(qa, qb); otherwise (a diff): the code of the mate with the larger Q, the forward
 *                one on a tie, Q = max(|qa - qb|, 2).  The quality byte is ascii_base + Q: the quality filter reads a merged read like any
 *                FASTQ read.  Never depends on the rest of the batch.
 *   rtx_merge_create   an object of its own on GPU `device` like rtx_qual: one stream, its own buffers (they only grow), no rtx_index.
 *                Checked in this order: null arguments, the parameters (RTX_ERR_INVALID), the device (RTX_ERR_NO_DEVICE without a gfx950).
 *   rtx_merge_run      n pairs as two (bases, quals, base_off) triples, base_off [n + 1] each as rtx_batch_prefetch takes it.  overlap / diffs /
 *                verdict / merged_len: [n] each.  The merged read of pair i lies at slot_off[i] of merged_bases and of merged_quals; the slot
 *                of a pair has (nf + nr rounded up to 16) bytes, slot_off [n + 1] is written by the call, and slot_cap -- the bytes of each of
 *                the two arrays -- must be at least slot_off[n]; what lies in a slot behind its merged read is undefined.  One byte per base
 *                code and one per quality byte travel to the device, as given.  n == 0: RTX_OK; RTX_ERR_INVALID: offsets that are not
 *                monotone, a mate of 2^31 bases or more, a quality byte of 128 or more, slots that do not fit.  Synchronous; calls on one
 *                object are serialised by the caller.
 *   rtx_merge_stage_times  seconds of the last rtx_merge_run: the host's staging pass, the copies and the wait around the kernel, all of it.
 *   rtx_merge_pair     the same for ONE pair on the host (no device), the candidates one after the other through the functions the kernel
 *                calls; merged_bases / merged_quals take nf + nr bytes (needed only when the pair merges).
 *   rtx_merge_queries  two handles of FASTQ parses with equal record counts (the forward and the reverse file, or blocks of them cut at the
 *                same record: rtx_fastq_block_end_n) -> a new handle with the forward labels, the merged bases and the merged quality bytes,
 *                on which rtx_queries_data / _quals / _label / _len work as on any other; a pair that is not merged becomes the empty read;
 *                pairs whose forward label is in `skip` are dropped.  The labels of the two mates must be equal up to their first blank,
 *                after a final /1 of the forward and /2 of the reverse label is taken off: RTX_ERR_PARSE otherwise -- as for record counts
 *                that differ -- with the number of the pair (from 1) in rtx_last_error.  The pairing is checked before the stage is
 *                looked at (a NULL stage: RTX_ERR_INVALID).
 *   rtx_queries_merge_report  nf, nr, overlap, diffs and verdict of every pair of such a handle, owned by it; RTX_ERR_STATE for another handle.
 *   rtx_fastq_block_end_n  as rtx_fastq_block_end, but behind the last whole record among the first max_records; *n_records: how many that
 *                is.  Two files read piecewise are cut at the same record with it. */
#define RTX_MERGE_MAX_READ 1024u
#define RTX_MERGE_MISMATCH_COST 5
#define RTX_MG_BAD_QUALITY 1u
#define RTX_MG_TOO_LONG 2u
#define RTX_MG_TOO_SHORT 4u
#define RTX_MG_NO_OVERLAP 8u
typedef struct {
    uint32_t ascii_base, min_overlap, max_diffs, max_diff_pct, q_cap;
} rtx_merge_params;
typedef struct rtx_merge rtx_merge;
int rtx_merge_create(int device, const rtx_merge_params *params, rtx_merge **out);
int rtx_merge_run(rtx_merge *m, uint64_t n, const uint8_t *f_bases, const uint8_t *f_quals, const uint64_t *f_off, const uint8_t *r_bases,
                  const uint8_t *r_quals, const uint64_t *r_off, uint32_t *overlap /*[n]*/, uint32_t *diffs /*[n]*/, uint32_t *verdict /*[n]*/,
                  uint32_t *merged_len /*[n]*/, uint64_t *slot_off /*[n + 1]*/, uint8_t *merged_bases, uint8_t *merged_quals, uint64_t slot_cap);
void rtx_merge_destroy(rtx_merge *m);
int rtx_merge_kernel_time(const rtx_merge *m, float *ms); /* milliseconds of the kernel of the last rtx_merge_run, from HIP events around it */
int rtx_merge_stage_times(const rtx_merge *m, double seconds[3]);
int rtx_merge_pair(const rtx_merge_params *params, const uint8_t *f_bases, const uint8_t *f_quals, uint32_t nf, const uint8_t *r_bases,
                   const uint8_t *r_quals, uint32_t nr, uint32_t *overlap, uint32_t *diffs, uint32_t *verdict, uint32_t *merged_len,
                   uint8_t *merged_bases, uint8_t *merged_quals);
int rtx_merge_queries(rtx_merge *m, const rtx_queries *fwd, const rtx_queries *rev, const char *const *skip, uint64_t n_skip, rtx_queries **merged);
int rtx_queries_merge_report(const rtx_queries *merged, const uint32_t **nf, const uint32_t **nr, const uint32_t **overlap, const uint32_t **diffs,
                             const uint32_t **verdict);
uint64_t rtx_fastq_block_end_n(const char *text, uint64_t len, uint64_t max_records, uint64_t *n_records);

/* ---- chimera check against the references (rtx_chimera.hip) ----------------------------------------------------------------------------
 * A PCR chimera is the head of one template joined to the tail of another: one reference explains its left part, another its right part,
 * and no single reference explains both.  The check is the counting problem of hit_count with positions kept.  Exact integers; the host
 * function, the x86 emulator and the device agree in every field.
 *   parameters   segments S (2 .. RTX_CHIMERA_MAX_SEGMENTS; RTX_CHIMERA_DEFAULT_SEGMENTS) and mindelta (RTX_CHIMERA_DEFAULT_MINDELTA:
 *                one substitution removes at most 8 windows, three differences per side).
 *   per read     of len bases, in the orientation given.  Window i (0 <= i < n_pos = max(0, len - 7)) is valid when its 8 bases are all
 *                plain codes (1, 2, 4, 8).  x_r[i] = 1 when window i is valid and its 8-mer occurs in reference r: positions count, a
 *                repeated 8-mer counts once per position (the classifier counts distinct 8-mers).  n_valid: the valid windows.
 *                b_s = floor(s n_pos / S), s = 0 .. S;  P_r[s] = sum of x_r[i] over i < b_s;  T_r = P_r[S];  Suf_r[s] = T_r - P_r[s].
 *                single = max_r T_r, parent the lowest r that attains it.  two[s] = max_r P_r[s] + max_r Suf_r[s] for s = 1 .. S - 1;
 *                seg the lowest s with the largest two[s], pos = b_seg; left = max_r P_r[seg] with parent_a the lowest r that attains
 *                it, right = max_r Suf_r[seg] with parent_b likewise; delta = two[seg] - single (never negative, and both flanks are
 *                decided by at least delta); flag = delta >= mindelta.  A parent whose count is 0 is RTX_NO_REF.
 *   status       RTX_CHIM_OK; RTX_CHIM_NO_KMER: n_valid = 0, everything 0 or RTX_NO_REF, not flagged; RTX_CHIM_TOO_LONG: more than
 *                RTX_CHIMERA_MAX_QUERY bases, not checked and not flagged.  A read's record never depends on the rest of its batch.
 *   rtx_chimera_create  an object of its own in front of a handle like rtx_qual: one stream, its own buffers (they only grow).  It BORROWS
 *                the handle's bitmap and row table, which never change: the index must outlive the object.  RTX_ERR_INVALID: segments
 *                out of range, a reference shard, a handle with RTX_OPT_STRAND set (a read given as its reverse complement matches
 *                nothing: checking both orientations is not done).
 *   rtx_chimera_run     the records of n reads, bases / base_off as rtx_batch_prefetch takes them.  Processed in slices, so that the
 *                device scratch stays under about 1 GB whatever the database size.  n == 0: RTX_OK.  Synchronous; calls on one object
 *                are serialised by the caller, and may run beside the handle's own batches.
 *   rtx_chimera_kernel_time  milliseconds of the scan kernels of the last run, from HIP events around them.
 *   rtx_chimera_read    the same for ONE read on the host (no device), from the reference sequences (ref_off [n_refs + 1]).
 *   rtx_index_set_chimera  the setting a handle holds for the callers that run the stage in front of it (NULL, the default: off -- nothing
 *                runs and nothing is allocated); the handle itself never reads it.  rtx_index_chimera: the setting and whether it is on.
 *   RTX_DEFAULT_CHIMERA_SLICE (rtx_set_default_option; default and 0: no cap): a cap on the reads of a slice of rtx_chimera_run and on the
 *                entries of a slice of rtx_denovo_check, read at every call and applied as a minimum with what the scratch budget gives.
 *                For tests: a small cap makes a small batch run in many slices.  Results do not depend on it. */
#define RTX_DEFAULT_CHIMERA_SLICE 6
#define RTX_CHIMERA_MAX_QUERY 4096u
#define RTX_CHIMERA_MAX_SEGMENTS 32u
#define RTX_CHIMERA_DEFAULT_SEGMENTS 16u
#define RTX_CHIMERA_DEFAULT_MINDELTA 24u
#define RTX_CHIM_OK 0u
#define RTX_CHIM_NO_KMER 1u
#define RTX_CHIM_TOO_LONG 2u
typedef struct {
    uint32_t segments;
    uint32_t mindelta;
} rtx_chimera_params;
typedef struct {
    uint32_t status, n_valid, single, parent, seg, pos, left, parent_a, right, parent_b, delta, flag;
} rtx_chimera_rec;
typedef struct rtx_chimera rtx_chimera;
int rtx_chimera_create(const rtx_index *index, const rtx_chimera_params *params, rtx_chimera **out);
int rtx_chimera_run(rtx_chimera *ch, uint64_t n, const uint8_t *bases, const uint64_t *base_off, rtx_chimera_rec *out /*[n]*/);
void rtx_chimera_destroy(rtx_chimera *ch);
int rtx_chimera_kernel_time(const rtx_chimera *ch, float *ms);
int rtx_chimera_read(const rtx_chimera_params *params, const uint8_t *read, uint64_t len, const uint8_t *ref_bases, const uint64_t *ref_off,
                     uint64_t n_refs, rtx_chimera_rec *rec);
int rtx_index_set_chimera(rtx_index *index, const rtx_chimera_params *params);
int rtx_index_chimera(const rtx_index *index, rtx_chimera_params *params, int *on);

/* ---- de novo chimera check of a run (rtx_denovo.hip, host_denovo.cpp) ------------------------------------------------------------------
 * Is a sequence of the run the head of one MORE ABUNDANT sequence of the same run joined to the tail of another?  What
 * `vsearch --uchime_denovo` and DADA2's removeBimeraDenovo answer between clustering and the final table; the check above only knows the
 * templates the database holds.  Exact, integers only, independent of scheduling; the host function and the device agree in every field.
 *   input        an rtx_tally_table, optionally the rtx_otu made from it, and the parameters: segments S (2 .. 32, default 16) and
 *                mindelta (default 24) as in rtx_chimera_params; abskew (an integer >= 1, RTX_DENOVO_DEFAULT_ABSKEW); max_parents
 *                (0: RTX_DENOVO_DEFAULT_MAX_PARENTS, which is also the most); flags (0).  params == NULL: the defaults.
 *   entries      without an OTU object every row of the table, weight = the row's total size, in table order.  With one: the seeds,
 *                weight = the OTU's total size, ordered by (weight descending, seed rank ascending).  Entry e has the sequence seq[e], the
 *                weight w[e] and the table rank row[e] (and, with an OTU object, the OTU otu[e]).
 *   parents      of e: the entries p < lim(e) that are not themselves flagged, lim(e) = min(e, #{p : w[p] >= abskew w[e]}, max_parents).
 *                Weights never increase along the list, so the set in the middle is a prefix; `e` keeps an entry from being its own
 *                parent when abskew = 1.
 *   record       of e: the record of rtx_chimera_read above with seq[e] as the read and the live parents as the references: the same
 *                windows, x_p[i] = window i valid and its 8-mer anywhere in p, the same b_s, P, Suf, single, two[s], seg (the lowest s
 *                with the largest two), delta, the lowest parent among equals, flag = delta >= mindelta.  Parent ids are ENTRY indices;
 *                RTX_NO_REF where a count is 0.
 *   status       RTX_CHIM_TOO_LONG (more than RTX_CHIMERA_MAX_QUERY bases: not checked, but still a parent of others), else
 *                RTX_CHIM_NO_KMER (no valid window), else RTX_DENOVO_NO_PARENT when lim(e) = 0 -- each of them with everything 0 or
 *                RTX_NO_REF and not flagged -- else RTX_CHIM_OK.
 *   recursion    e's record depends on the flags of entries below lim(e) <= e only: the definition is a recursion over e = 0, 1, ... and
 *                has exactly one solution.  That a flagged sequence is no parent (uchime's greedy rule) is part of the definition: without
 *                it a rarer variant of a chimera, two or more differences away from it, is "explained" by the chimera and passes.
 *   rtx_denovo_check       on GPU `device` (RTX_ERR_NO_DEVICE without a gfx950), in an object made and released inside the call.  The stage
 *                builds a bitmap of its own over the entries below the largest lim -- the index's layout, one row per 8-mer, the zero
 *                row, and one more row that holds the live mask: 64 MiB + 2 KiB per tile of 8192 entries -- and scans entry e against the
 *                tiles below lim(e) only, the planes ANDed at every checkpoint with the live mask and the prefix mask of lim(e).  Round 1
 *                scans every entry with all parents live; after a round the new flags are compared with the old ones, the live mask is
 *                rewritten, and the next round scans exactly the entries e with lim(e) > the lowest entry whose flag changed.  It ends
 *                with a round that changed nothing (a round with nothing to scan is one): the solution of the recursion.  `rounds` counts
 *                them, `scans` the entries handed to the rounds, summed.
 *   rtx_denovo_check_host  the definition restated literally: a set of 8-mers per parent, e ascending, explicit parent lists.  Equal to the
 *                device's result field by field, except rounds (1), scans (the entries) and the times.
 *                RTX_ERR_INVALID: S out of range, abskew 0, flags != 0, max_parents above the default, an OTU object whose row count is
 *                not the table's, more than 2^31 - 2 entries.  The table is laid out (rtx_tally_table_view) and otherwise unchanged.
 *   rtx_denovo_view        valid until the object is destroyed; otu is NULL without an OTU object.  n_checked: the entries with RTX_CHIM_OK.
 *                rtx_denovo_times: seconds of upload and bitmap, the scan kernels of all rounds (from HIP events around them), the rounds'
 *                bookkeeping (row lists, reductions, flag updates, read-backs), the download; 0 for a host result.
 *   rtx_denovo_format_records  `#entry\tweight\tstatus\twindows\tsingle\tparent\tseg\tpos\tleft\ta\tright\tb\tdelta\tchimera\n`, then one
 *                line per entry: `otu{k}` (k from 1) or `uniq{rank}` (from 1), the weight, status as a number, n_valid, single, parent,
 *                seg, pos, left, parent_a, right, parent_b, delta, and Y (flagged), N (RTX_CHIM_OK, not flagged) or ? (not checked).
 *                Parents are named like the entry; RTX_NO_REF is `*`.  Buffer protocol of rtx_tally_format_fasta.
 *   rtx_denovo_format_fasta    the lines of rtx_otu_format_fasta (with an OTU object) or rtx_tally_format_fasta of the entries that are not
 *                flagged and whose weight is at least minsize, in the order of those functions; the numbers stay.  `table` as in rtx_otu_format_fasta.
 *   rtx_denovo_format_table    the same selection of rtx_otu_format_table / rtx_tally_format_table (`otu` NULL without an OTU object). */
#define RTX_DENOVO_NO_PARENT 3u
#define RTX_DENOVO_DEFAULT_ABSKEW 2u
#define RTX_DENOVO_DEFAULT_MAX_PARENTS 262144u
typedef struct rtx_denovo rtx_denovo;
typedef struct rtx_denovo_params {
    uint32_t segments;    /* 2 .. RTX_CHIMERA_MAX_SEGMENTS */
    uint32_t mindelta;
    uint32_t abskew;      /* >= 1 */
    uint32_t max_parents; /* 0: RTX_DENOVO_DEFAULT_MAX_PARENTS */
    uint32_t flags;       /* 0 */
} rtx_denovo_params;
typedef struct rtx_denovo_view_t {
    uint64_t n_entries;
    const uint32_t *row;        /* [n_entries] the table rank of an entry */
    const uint32_t *otu;        /* [n_entries] its OTU, or NULL */
    const uint64_t *weight;     /* [n_entries] */
    const uint32_t *lim;        /* [n_entries] */
    const rtx_chimera_rec *rec; /* [n_entries] */
    uint64_t n_checked, n_flagged;
    uint32_t rounds;
    uint64_t scans;
} rtx_denovo_view_t;
int rtx_denovo_check(int device, rtx_tally_table *table, rtx_otu *otu_or_null, const rtx_denovo_params *params, rtx_denovo **out);
int rtx_denovo_check_host(rtx_tally_table *table, rtx_otu *otu_or_null, const rtx_denovo_params *params, rtx_denovo **out);
int rtx_denovo_view(rtx_denovo *d, rtx_denovo_view_t *view);
int rtx_denovo_times(const rtx_denovo *d, double seconds[4]);
void rtx_denovo_destroy(rtx_denovo *d);
int64_t rtx_denovo_format_records(rtx_denovo *d, char *buf, uint64_t cap);
int64_t rtx_denovo_format_fasta(rtx_denovo *d, rtx_tally_table *table, rtx_otu *otu_or_null, uint64_t minsize, char *buf, uint64_t cap);
int64_t rtx_denovo_format_table(rtx_denovo *d, rtx_tally_table *table, rtx_otu *otu_or_null, const char *const *names, uint64_t minsize, char *buf, uint64_t cap);

/* ---- result text produced on the device (rtx_text.hip) ------------------------------------------------------------------------------
 * The `.out` lines, and with RTX_TEXT_TSV the `.tsv` lines, of every query of a download, formatted by kernels behind the final rows: byte
 * for byte what rtx_format_query prints for the view, the label, the bases and the exact matches of the query (the override of
 * raxtax.rs:73-84 unless RTX_SKIP_EXACT_MATCHES or RTX_RAW_CONFIDENCE is set in `flags`; the exact matches are those of the batch: the ids
 * passed at upload, or the device lookup's).  Off until a caller asks:
 *   rtx_index_text_setup       uploads the lineage strings of `tree` (whose tips must be the handle's database) and switches the text on with
 *                              `flags` (RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE | RTX_TEXT_TSV); tree == NULL switches it off and frees the table.
 *   rtx_batch_prefetch_labels  stages the labels of the batch that the NEXT rtx_batch_prefetch / rtx_batch_upload stages (call it first),
 *                              into the same input set, asynchronously.  A batch without labels has no text.
 *   rtx_batch_text             the text of the last download: per query (input order) its lines joined by '\n', NUL-terminated, at
 *                              out + out_off[q] (out_off[n_queries] = the bytes of all); a query with status != RTX_Q_OK has the empty
 *                              text.  tsv / tsv_off likewise, NULL without RTX_TEXT_TSV.  Valid as long as the rtx_result_view of that
 *                              download (until the second-next download).  RTX_ERR_STATE: that download has no text. */
typedef struct {
    uint64_t n_queries;
    const char *out;
    const uint64_t *out_off; /* [n_queries + 1] */
    const char *tsv;
    const uint64_t *tsv_off; /* [n_queries + 1] */
} rtx_text_view;
int rtx_index_text_setup(rtx_index *index, const rtx_tree *tree, uint32_t flags);
int rtx_batch_prefetch_labels(rtx_index *index, uint64_t n_queries, const char *const *labels);
int rtx_batch_text(rtx_index *index, rtx_text_view *out);

/* ---- staged execution of a reference-sharded handle (one sub-batch at a time) --------------------
 * Between the stages the caller exchanges two device buffers with the other shards (RCCL):
 *   after rtx_shard_count: all-reduce(sum) RTX_BUF_HIST   ([n][row_stride] uint32, n = queries of the sub-batch)
 *   after rtx_shard_prob : all-gather  RTX_BUF_PREFIX ([n][n_bnd_local] double); the global prefix row is the
 *                          concatenation over shards of prefix_s[1..] + sum of the totals prefix_s'[last] of
 *                          the shards s' < s, preceded by a 0 (n_bnd_global values) -> rtx_shard_walk.
 * Stages are asynchronous on the handle's stream: rtx_batch_sync before touching a buffer. */
#define RTX_BUF_HIST 1
#define RTX_BUF_PREFIX 2
int rtx_shard_begin(rtx_index *index, uint32_t *n_sub_batches, uint32_t *sub_batch);
/* Tile pruning on a reference shard (RTX_OPT_SHARD_PRUNE = 1 before the upload; 4 tiles or more on the shard; queries with t <= 1023):
 * the threshold of a query follows from the best block of 64 references ANYWHERE in the database, so the counting of a sub-batch
 * stops once for an exchange:   rtx_shard_bounds  ->  all-gather RTX_BUF_BEST, keep per query the record with the largest first word
 * (ties: the lowest shard) in every shard's buffer  ->  rtx_shard_count (counts the live tiles only)  ->  as before.
 * rtx_shard_prunes (after rtx_shard_begin): 1 if this run prunes -- all shards must agree (same options, same queries); the shards
 * then process the queries in their min-hash order, which is the same on every shard. */
#define RTX_OPT_SHARD_PRUNE 16
int rtx_shard_prunes(const rtx_index *index);
int rtx_shard_bounds(rtx_index *index, uint32_t sub_batch_idx, uint32_t flags);
int rtx_shard_count(rtx_index *index, uint32_t sub_batch_idx, uint32_t flags);
int rtx_shard_prob(rtx_index *index, uint32_t sub_batch_idx);
int rtx_shard_walk(rtx_index *index, uint32_t sub_batch_idx, const double *prefix_global /* device */);
int rtx_shard_info(const rtx_index *index, uint64_t *ref_lo, uint64_t *ref_hi, uint32_t *n_bnd_global,
                   uint32_t *n_bnd_local, uint32_t *first_bnd);
int rtx_device_buffer(rtx_index *index, int which, void **device_ptr, uint64_t *row_stride_elems);
/* The same for the scratch set of sub-batch `sub_batch_idx`: a staged run alternates between two sets, so that
 * the exchange of sub-batch i (on the caller's stream or RCCL's) can overlap with rtx_shard_count of sub-batch i + 1.
 * RTX_BUF_COUNTS: the u16 hit counts ([n][row_stride], needs RTX_OPT_PACKED_COUNTS = 0) -- what a k-mer-sharded
 * database (SURVEY.md 8e mode A, the literal wording of BASELINE.json configs[4]) all-reduces; rtx_shard_rehist then
 * rebuilds the histogram of prob.rs:13-19 from the summed counts before rtx_shard_prob. */
#define RTX_BUF_COUNTS 3
#define RTX_BUF_BEST 4 /* [n][66] uint32: {largest bound of a block of 64 references, 0, exact counts of that block's references} */
int rtx_shard_buffer(rtx_index *index, uint32_t sub_batch_idx, int which, void **device_ptr, uint64_t *row_stride_elems);
int rtx_shard_rehist(rtx_index *index, uint32_t sub_batch_idx);
/* The HIP stream (hipStream_t) every kernel of this handle is enqueued on: a caller that interleaves its own device
 * work (collectives) with rtx_shard_* orders it against this stream instead of synchronising the host. */
int rtx_index_stream(rtx_index *index, void **hip_stream);

/* Per-kernel device time of the last rtx_batch_run, from HIP events on the library's
 * stream (ms, summed over sub-batches), and launch counts (0 launches = stage not timed, see
 * RTX_OPT_STAGE_TIMING).  Stage order: */
#define RTX_STAGE_KMER_EXTRACT 0
#define RTX_STAGE_HIT_COUNT 1
#define RTX_STAGE_PROB_TABLE 2
#define RTX_STAGE_TAXON_PREFIX 3
#define RTX_STAGE_LINEAGE_WALK 4
#define RTX_STAGE_TILE_BOUNDS 5 /* tile pruning (RTX_OPT_TILE_PRUNE): the queries counted against the union bitmap (the hit_count kernel again); 0 launches if the run did not prune */
#define RTX_STAGE_TILE_PRUNE 6  /* ... prune_kernel (thresholds, live tiles) + the row lists of the live tiles */
#define RTX_STAGE_EXACT_MATCH 7 /* Tree.sequences.get on the device (rtx_exact.hip; RTX_OPT_DEVICE_EXACT), once per run: reported with sub-batch 0 */
#define RTX_STAGE_ORDER 8       /* processing order of the batch (rtx_cluster.hip: sketch, locator, radix sort, inverse), once per run: reported with sub-batch 0 */
#define RTX_STAGE_PAIR_UNION 9  /* union row lists of the pairs of neighbouring queries (pair_union_kernel), once per sub-batch */
#define RTX_NUM_STAGES 10
int rtx_batch_stage_times(rtx_index *index, float ms[RTX_NUM_STAGES], uint32_t launches[RTX_NUM_STAGES]);
/* Algorithmic work of the last rtx_batch_run: sum over queries of
 * H_q = sum_r count_q[r] (postings touched) and of L_q (query bytes), and the bitmap
 * bytes the hit_count kernel actually requested. */
int rtx_batch_work(rtx_index *index, uint64_t *sum_hits, uint64_t *sum_query_bytes,
                   uint64_t *bitmap_bytes_read);
/* bitmap_bytes_read split by the kind of launch of the hit_count kernel: the tiles of the database it counted, and -- with tile pruning --
 * the bounds pass on the union bitmap */
int rtx_batch_work_split(rtx_index *index, uint64_t *live_bytes, uint64_t *bounds_bytes);
/* Algorithmic work of the probability stage of the last rtx_batch_run (prob.rs:43-90):
 * sum over queries of D_q (n_q + 1) -- the points of the pmf/cmf grid the reference evaluates, D_q = number of
 * distinct hit counts, n_q = t_q / 2 -- and of D_q.  ops_prob = 3 x grid points (2 exp + 1 log each). */
int rtx_batch_prob_work(rtx_index *index, uint64_t *sum_grid_points, uint64_t *sum_distinct_counts);

/* ------------------------------------------------------------------------- */
/* Parity / debug taps (full vectors; not used on the fast path)              */
/* ------------------------------------------------------------------------- */
/* Valid after rtx_batch_run + rtx_batch_sync for queries of the LAST sub-batch only when
 * the batch spans several sub-batches; tests keep n_queries <= sub-batch.  */
int rtx_debug_kmers(rtx_index *index, uint64_t query, uint16_t *kmers /*cap 65535*/, uint32_t *t);
int rtx_debug_hit_counts(rtx_index *index, uint64_t query, uint16_t *counts /*n_refs*/);
int rtx_debug_prob_table(rtx_index *index, uint64_t query, double *table_over_z /*t+1*/, double *z);
int rtx_debug_probs(rtx_index *index, uint64_t query, double *probs /*n_refs*/);
/* tile pruning: the largest bound of every tile of 8192 references as the bounds pass left it for a query of the last sub-batch
 * (what prune_kernel's tile-aware threshold and the live masks are derived from); RTX_ERR_STATE if the last run did not prune */
int rtx_debug_tile_bounds(rtx_index *index, uint64_t query, uint16_t *tile_ub /*ceil(n_refs / 8192)*/);
/* processing order of the last run (RTX_OPT_CLUSTER / RTX_OPT_LOCATOR): perm[position] = query */
int rtx_debug_order(rtx_index *index, uint32_t *perm /*n_queries*/);
/* queries per sub-batch of the uploaded batch and the number of sub-batches: positions [(n_sub - 1) * sub_batch, n_queries) of the
 * processing order are the last sub-batch, the one the taps can read */
int rtx_batch_sub_batch(const rtx_index *index, uint32_t *sub_batch, uint32_t *n_sub_batches);
/* A batch is cut into LENGTH CLASSES (t <= 255 / t <= 1023 / t <= 2047 (ABI 5) / longer reads whose probability arrays fit LDS / up to t = 65 535): the class
 * leads the processing order, every class runs through sub-batches of its own shape (bit planes, pair kernel and tile pruning, memoised
 * tables or the recurrence kernel), so that one long read does not move a batch of barcodes off the fast path; results come back in
 * input order.  rtx_batch_sub_batch reports the sub-batch size of the LAST class and the number of sub-batches of the whole batch;
 * rtx_batch_last_sub_batch the positions [first, first + n) of the processing order that form the last sub-batch (the one the taps read);
 * rtx_batch_classes, per class c < *n_classes <= 5 (4 until ABI 4: out[16]): out[4c] queries, [4c + 1] longest query (bases), [4c + 2] sub-batch size,
 * [4c + 3] bit planes | tables << 8 | pair kernel << 9 | tile pruning << 10 | records path << 11 | global-memory forms << 12 (the last
 * four after rtx_batch_run). */
int rtx_batch_last_sub_batch(const rtx_index *index, uint64_t *first, uint32_t *n);
int rtx_batch_classes(const rtx_index *index, uint32_t *n_classes, uint64_t out[20]);
/* tile pruning of the last run (RTX_OPT_TILE_PRUNE): out[0] (pair, tile) blocks that are counted for at least one of their two queries, [1] pairs,
 * [2] sum of the lower bounds of the best hit, [3] sum of the thresholds, [4] sum of the largest tile bounds, [5] queries, [6] bounds below a count
 * they bound (must be 0), [7] (query, tile) combinations that are counted, [8] (query, tile) combinations with a count above the query's
 * threshold -- what exact knowledge would have counted --, [9] queries with a threshold; all 0 if the run did not prune.
 * The fine bounds pass (RTX_OPT_FINE_BOUNDS): [10] (query, tile) combinations it took off the lists, [11] its (pair, fine tile) blocks,
 * [12] (pair, tile) blocks the counting pass was left with (0 if the pass did not run: then [0] is that number).
 * The records path (RTX_OPT_RECORDS): [13] records written (references above their query's threshold), [14] queries on the path,
 * [15] of those, queries whose boundary entries did not fit LDS (prefix row written out, walked from memory) */
int rtx_debug_prune_stats(rtx_index *index, uint64_t *out /*16*/);
/* table / Z of a query of the last sub-batch as the PRUNED run computed it (0 for the counts up to the query's threshold), its Z and the
 * threshold; must be called before any other tap (those recount the sub-batch in full) */
int rtx_debug_pruned_prob_table(rtx_index *index, uint64_t query, double *table_over_z /*t+1*/, double *z, uint32_t *threshold);
/* The last sub-batch exactly as the run left it -- NO recount (the taps above prove the kernel that counts every tile; this one shows
 * what the timed, pruned path computed); must be called before any recounting tap.  counts[n_refs]: what hit_count wrote (0xFFFF for the
 * references of tiles it did not visit for the query's pair); tile_live[ntiles]: 1 if the tile was visited; hist[t + 1]: the histogram
 * of prob.rs:13-19 as prune_kernel (bin 0 = the references never counted) and hit_count (every counted reference) left it; the query's
 * threshold (0: none) and i* + 1 (rtx_prune.hip).  Any output pointer may be NULL. */
int rtx_debug_run_counts(rtx_index *index, uint64_t query, uint16_t *counts /*n_refs*/, uint8_t *tile_live /*ntiles*/,
                         uint32_t *hist /*t+1*/, uint32_t *threshold, uint32_t *i1);
/* A query on the records path (RTX_OPT_RECORDS) wrote no counts but the (reference, count) records of the counts above its threshold:
 * rtx_debug_run_counts then returns, for the visited tiles, the count of every reference that has a record and 0 for every other one
 * (read back from the record segments, which must be in ascending reference order).  n_segments: 0 = the query took the dense epilogues. */
int rtx_debug_run_mode(rtx_index *index, uint64_t query, uint32_t *n_segments);
/* prune_kernel's view of a query of the last sub-batch (needs RTX_OPT_DEBUG_TAPS = 1 before the run): out[0] the block of 64 references
 * with the largest bound, [1] M = the best exact count in it, [2] the threshold, [3] i* + 1, [4] the largest bound, [5] t, [8 .. 72) the exact
 * counts of the block's references (0: behind the end of the database, or zeroed by RTX_SKIP_EXACT_MATCHES) */
int rtx_debug_prune_detail(rtx_index *index, uint64_t query, uint32_t *out /*72*/);
/* Lineage::new(label, tree, probs).evaluate() (src/lineage.rs:61-112) on a caller-supplied
 * probability vector: runs taxon_prefix + lineage_walk + the host finalisation for one
 * pseudo-query.  Lets the reference's lineage KATs pin the device walk.  Mode 0 of
 * rtx_debug_evaluate_mode below (the workspace is sized as for a query with as many k-mers as probs has distinct values). */
int rtx_debug_evaluate(rtx_index *index, const double *probs /*n_refs*/, rtx_result_view *out);
/* The same evaluation through the path a run takes.  The pseudo-query is an honest one: the count of reference r is the rank of
 * probs[r] among the DISTINCT values of the vector (ascending; rank 0 is the value 0.0 where it occurs), the table holds the distinct
 * values, t = their number - 1, and the largest "count" of a tile of 8192 references is its largest rank.  At most 65 536 distinct
 * values (counts are 16 bits wide), whatever the number of references; rtx_debug_evaluate is mode 0.
 *   mode 0: taxon_prefix without tile maxima, the table in global memory, the lineage walk as a kernel of its own
 *   mode 1: the walk fused into taxon_prefix, as on every whole-database handle; no tile maxima.  The table is copied to LDS where a run
 *           would copy it (a table row of at most 16 KiB: up to 2048 distinct values), else read from global memory
 *   mode 2: mode 1 with tile maxima: tiles that hold no non-zero probability are not swept, the boundaries inside them reach the walk
 *           as gaps (up to six; further ones are written out)
 * table_in_lds (may be NULL): 1 if the launch took the table from LDS.  With probabilities that are multiples of 2^-40 and sum to 1
 * every partial sum is exact in any order, so the rows must equal the reference's bit for bit, ties included. */
int rtx_debug_evaluate_mode(rtx_index *index, const double *probs /*n_refs*/, uint32_t mode, rtx_result_view *out, uint32_t *table_in_lds);
/* out[x] = ln x! for x < n (n <= 98320) as every handle uploads it for its kernels: CPU restatements of the device arithmetic start from the
 * same table (it differs from other implementations of ln Gamma in the last place, and Z carries that once per reference).  No device needed. */
int rtx_debug_ln_factorial(uint32_t n, double *out /*n*/);
/* The probability stage (src/prob.rs:8-103) on caller-supplied histograms: n_q queries, query q with t[q] distinct k-mers and
 * hist[q * hstride + m] references of hit count m (hstride > the largest t, no count above t[q]).  n_refs is the caller's, not the handle's
 * -- a handle over a dozen references carries histograms that stand for millions -- and one per launch, as in a run: it enters the global
 * signal (its 1 / N) and nothing else, so rows of other totals may ride along.  One launch of the kernels a run launches, with
 * the parameters a sub-batch of the class of the largest t would get:
 *   kernel 0: the lookup in the memoised tables (t <= 2047, else RTX_ERR_TOO_LONG; the tables are built or grown as a batch would), through
 *             the processing order a sub-batch gets; prune_thr / prune_i1 (both or neither): the thresholds tile pruning would hand over
 *   kernel 1: the recurrence with its arrays in LDS
 *   kernel 2: the recurrence with its arrays in global memory, at any t (a run takes it for reads of tens of kilobases only)
 * Out, per query: table / Z (NaN at the counts the histogram does not hold: the kernels never write those), Z, the global signal, the
 * status (RTX_Q_*) and the number of distinct counts.  Needs no batch and leaves a later one what it would have been. */
int rtx_debug_prob_hist(rtx_index *index, uint32_t n_q, const uint32_t *t /*n_q*/, const uint32_t *hist /*n_q x hstride*/, uint32_t hstride,
                        uint64_t n_refs, uint32_t kernel, const uint16_t *prune_thr /*n_q or NULL*/, const uint16_t *prune_i1 /*n_q or NULL*/,
                        double *table_over_z /*n_q x hstride*/, double *z /*n_q*/, double *gs /*n_q*/, uint8_t *status /*n_q*/,
                        uint32_t *ndist /*n_q*/);

/* ------------------------------------------------------------------------- */
/* Host mirror of the output formatting (src/lineage.rs:17-48, utils.rs:62-89) */
/* ------------------------------------------------------------------------- */
/* Applies the single-exact-match override (raxtax.rs:73-84, unless RTX_RAW_CONFIDENCE or
 * RTX_SKIP_EXACT_MATCHES is set in flags) and formats the `.out` (and, if tsv_buf != NULL,
 * `.tsv`) lines of query q of a result view.  Returns bytes written (excluding NUL) or a
 * negative RTX_ERR_*; lines of one query are '\n'-joined without a trailing newline. */
int64_t rtx_format_query(const rtx_tree *tree, const rtx_result_view *res, uint64_t q,
                         const char *label, const uint8_t *seq, uint64_t seq_len,
                         const uint32_t *exact_ids, uint64_t n_exact, uint32_t flags, char *out_buf,
                         uint64_t out_cap, char *tsv_buf, uint64_t tsv_cap, int64_t *tsv_len);

/* Compact byte record of a result view: what a rank ships in the multi-GPU result gather (BASELINE.json
 * configs[3]; layout in raxtax_amd/dist_util.py: 32 B header, 25 B per query (begin, global signal, row count, t,
 * status) + 13 + L B per row (lineage u32, depth, L confidences as hundredths, local signal), L = depth of the
 * deepest row, so every level of every row travels).  buf == NULL: returns the size needed; else the bytes written
 * or a negative RTX_ERR_*. */
int64_t rtx_result_pack(const rtx_result_view *res, uint8_t *buf, uint64_t cap);

/* The writer's side of that gather (main.rs:126-136 for the results of every rank): the `.out` lines of all queries of ONE packed record
 * buffer, formatted natively on `threads` threads (0: the library's budget) -- the text rtx_format_query gives for the view the records
 * were packed from.  labels: [n] the labels of the buffer's queries; exact_one: [n] the id of a query's ONLY exact match (the override of
 * raxtax.rs:73-84; 0xFFFFFFFF: none or several) or NULL; flags: RTX_SKIP_EXACT_MATCHES / RTX_RAW_CONFIDENCE switch the override off as in the
 * reference.  out: the texts back to back, each NUL-terminated, lines of one query '\n'-joined; line_off: [n + 1] where each starts (a query
 * without rows -- status != 0 -- has an empty text) or NULL.  Returns the bytes written, with out == NULL the bytes needed, or a negative RTX_ERR_*;
 * a buffer that is too small: -(bytes needed) - RTX_NEED_BASE (every value below -RTX_NEED_BASE; ABI 5) -- the text has been formatted to be
 * measured, the caller allocates and calls once more. */
#define RTX_NEED_BASE 1024
int64_t rtx_records_format(const rtx_tree *tree, const uint8_t *records, uint64_t n_bytes, const char *const *labels,
                           const uint32_t *exact_one, uint32_t flags, char *out, uint64_t cap, uint64_t *line_off, uint32_t threads);

/* ------------------------------------------------------------------------- */
/* Host mirror of raxtax() itself (src/raxtax.rs:14-97)                       */
/* ------------------------------------------------------------------------- */
/* Receives one message per query, in input order: the `(label, out_lines, tsv_lines?)`
 * triple the reference sends on its crossbeam channel (raxtax.rs:85-87).  A non-zero
 * return plays the role of a closed channel: rtx_raxtax stops with RTX_ERR_SENDER. */
typedef int (*rtx_sender_fn)(void *ctx, const char *label, const char *out_lines, const char *tsv_lines);
/* Same arguments, in the same order and with the same meaning as the reference function,
 * plus the device index that replaces the CPU traversal of `tree`.  chunk_size = queries
 * per device batch (0 = all at once; the reference's rayon chunking has no other effect).
 * Exact-match lookups (raxtax.rs:42), the lineage-consistency warning (raxtax.rs:43-53,
 * written to stderr) and the override (raxtax.rs:73-84) run on the host. */
int rtx_raxtax(rtx_index *index, const rtx_tree *tree, uint64_t n_queries, const char *const *labels,
               const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches, int raw_confidence,
               uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv);

/* The same on several device handles at once -- one per GPU of the node (the index replicated, BASELINE.json configs[3]), or several
 * on one GPU: chunks of `chunk_size` queries (0: one chunk per handle) are dealt to the handles in turn, every handle is driven by a
 * thread of its own inside this call, and the messages reach `sender` in input order, as from rtx_raxtax.  The reference's parallel
 * driver is one call inside the process too (par_chunks over the rayon pool, raxtax.rs:35-36, main.rs:40-57). */
int rtx_raxtax_multi(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                     const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                     int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv);
/* The same with a second callback: `info` (may be NULL) is called directly before the sender, once for every query that has a message, in
 * input order, with the query's label, its strand (0 plus, 1 minus: RTX_OPT_STRAND), its peak (rtx_batch_strands) and t.  A non-zero return
 * ends the call like a closed channel (RTX_ERR_SENDER).  rtx_raxtax and rtx_raxtax_multi are this call with info = NULL.  All three honour
 * RTX_OPT_STRAND of their handles, which must agree on it (RTX_ERR_INVALID otherwise): the messages are those of the chosen orientation,
 * formatted on the host whatever RTX_OPT_DEVICE_TEXT says; the `.tsv` sequence column prints the orientation that was classified. */
typedef int (*rtx_query_info_fn)(void *ctx, const char *label, int strand, uint32_t peak, uint32_t t);
int rtx_raxtax_multi_ex(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                        const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                        int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                        rtx_query_info_fn info, void *info_ctx);
/* rtx_raxtax_multi_ex with a callback that also receives the nearest reference of the query and its ties (RTX_OPT_NEAREST on the handles,
 * which must agree on it: RTX_ERR_INVALID otherwise; with the option off it receives RTX_NO_REF and 0).  `hit` may be NULL. */
typedef int (*rtx_query_hit_fn)(void *ctx, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties);
int rtx_raxtax_multi_ex2(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_hit_fn hit, void *hit_ctx);
/* rtx_raxtax_multi_ex2 with a callback that also receives the alignment identity of the query (RTX_OPT_IDENTITY on the handles, which must
 * agree on it: RTX_ERR_INVALID otherwise; with the option off it receives RTX_NO_DIST and the query's length).  `align` may be NULL. */
typedef int (*rtx_query_align_fn)(void *ctx, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties,
                                  uint32_t dist, uint32_t qlen);
int rtx_raxtax_multi_ex3(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx);
/* rtx_raxtax_multi_ex3 with a callback for the primer trimming (rtx_index_set_primers): called for EVERY query of the caller, in input
 * order, directly before the `align` callback of that query (a query without a message, such as an emptied read, has no `align` call and
 * still has this one): the read's length as given, the kept range [lo, hi) and the hit word.  With no primers set: 0, raw_len and nothing
 * found.  Per query of the caller also under RTX_OPT_DEREP: every read is trimmed itself.  Either callback may be NULL. */
typedef int (*rtx_query_trim_fn)(void *ctx, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint32_t hit);
int rtx_raxtax_multi_ex4(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx);
/* rtx_raxtax_multi_ex4 with the quality strings of the reads (quals, indexed by base_off: rtx_queries_quals) and a callback for the quality
 * filter (rtx_index_set_quality): called for EVERY query of the caller, in input order, directly after its `trim` callback: the read's
 * length as given, the kept range [lo, hi) -- of the raw read, the primers off -- the expected errors of the kept bases times 2^40 and the
 * verdict (0: passed; a discarded read is classified as the empty read).  With no filter set: the range the primers left, 0 and 0, and
 * quals is ignored; a filter without quals is RTX_ERR_INVALID.  Per query of the caller also under RTX_OPT_DEREP.  Any callback may be NULL. */
typedef int (*rtx_query_qual_fn)(void *ctx, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint64_t ee, uint32_t verdict);
int rtx_raxtax_multi_ex5(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                         rtx_query_qual_fn qual, void *qual_ctx);
/* rtx_raxtax_multi_ex5 with a callback for the chimera check (rtx_index_set_chimera on the handles, which must agree on it: RTX_ERR_INVALID
 * otherwise, and with RTX_OPT_STRAND set): called for EVERY query of the caller, in input order, directly after its `qual` callback, with the
 * query's record (valid during the call).  The stage runs behind the dereplication, so a distinct read is checked once and a copy carries
 * its representative's record; a flagged read is classified as the empty read, exactly as one the quality filter discards: reported, not
 * classified, not counted by an open profile.  With no check set: RTX_CHIM_OK, zeros and RTX_NO_REF.  Any callback may be NULL. */
typedef int (*rtx_query_chimera_fn)(void *ctx, const char *label, const rtx_chimera_rec *rec);
int rtx_raxtax_multi_ex6(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                         rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx);
/* The last rtx_raxtax* call of the process: its queries, the reads the stage checked (the distinct ones under RTX_OPT_DEREP), the queries
 * whose record is flagged, and the busy seconds of the stage; all 0 when its handles had no chimera check set. */
int rtx_raxtax_last_chimera(uint64_t *queries, uint64_t *checked, uint64_t *flagged, double *busy_seconds);
/* rtx_raxtax_multi_ex6 with a callback for the sample demultiplexing (rtx_index_set_tags): called for EVERY query of the caller, in input
 * order, directly before its other callbacks: the length of the read as given, its sample, the range [lo, hi) the tags left of it and the
 * hit and info words of rtx_demux_run -- RTX_DEMUX_NONE, 0, raw_len, no tags and 0 with no tags set.  The callbacks behind it then speak of
 * the demultiplexed read: their raw_len is hi - lo (0 for a read that is not assigned), their positions count from lo.  Any callback may
 * be NULL. */
typedef int (*rtx_query_demux_fn)(void *ctx, const char *label, uint32_t raw_len, uint32_t sample, uint32_t lo, uint32_t hi, uint32_t hit, uint32_t info);
int rtx_raxtax_multi_ex7(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                         rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx, rtx_query_demux_fn demux,
                         void *demux_ctx);
/* The last rtx_raxtax* call of the process: its queries, those assigned to a sample, the queries of every verdict (reasons[v], v =
 * RTX_DEMUX_OK .. RTX_DEMUX_UNKNOWN_PAIR) and the busy seconds of the stage; all 0 when its handles had no tags set. */
int rtx_raxtax_last_demux(uint64_t *queries, uint64_t *assigned, uint64_t reasons[5], double *busy_seconds);
/* rtx_raxtax_multi_ex7 with a callback for the contaminant screen (rtx_index_set_screen on the handles, which must hold the same set and
 * parameters: RTX_ERR_INVALID otherwise): called for EVERY query of the caller, in input order, directly after its `qual` callback and
 * before `chimera`, with what rtx_screen_run says of the range that primers and quality left.  A contaminant is classified as the empty
 * read, exactly as one the quality filter discards: reported, not classified, no message, no align callback, not counted by an open
 * profile, not offered to dereplication or the chimera check.  Per query of the caller also under RTX_OPT_DEREP.  With no screen set:
 * 0, 0, RTX_SCREEN_NONE, RTX_SCREEN_NONE, 0.  The stage needs no quality strings.  Any callback may be NULL. */
typedef int (*rtx_query_screen_fn)(void *ctx, const char *label, uint32_t windows, uint32_t hits, uint32_t first, uint32_t source, uint32_t verdict);
int rtx_raxtax_multi_ex8(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                         const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                         int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                         rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                         rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx, rtx_query_demux_fn demux,
                         void *demux_ctx, rtx_query_screen_fn screen, void *screen_ctx);
/* The last rtx_raxtax* call of the process: its queries, those whose range was not already empty when the screen saw it, the
 * contaminants among them, and the busy seconds of the stage; all 0 when its handles had no screen set. */
int rtx_raxtax_last_screen(uint64_t *queries, uint64_t *screened, uint64_t *contaminants, double *busy_seconds);
/* A ready-made sender that discards the messages and only counts them: ctx = NULL or uint64_t[2] {messages, bytes of text} */
int rtx_sender_discard(void *ctx, const char *label, const char *out_lines, const char *tsv_lines);
/* Busy seconds of the stages of the last rtx_raxtax / rtx_raxtax_multi call of this process (which stage bounds an end-to-end run):
 * busy[0] exact-match lookup on the host (0 when the device does it), busy[1] device stage of the busiest handle (upload, kernels,
 * download), busy[2] formatting of the busiest handle, busy[3] sender; *n_chunks = chunks of that call.  The counterpart of the
 * reference's `timer!` log lines (raxtax.rs:13, prob.rs:7, lineage.rs:79). */
int rtx_raxtax_last_timing(double busy[4], uint64_t *n_chunks);

/* ------------------------------------------------------------------------- */
/* Host thread budget (the reference: rayon pool of std::thread::available_parallelism threads, main.rs:40-57, utils.rs:139-158) */
/* ------------------------------------------------------------------------- */
/* Every worker pool of the library (FASTA parsing, result finalisation, formatting, record packing) is sized from the CPUs this
 * process may really use -- the affinity mask capped by the cgroup CPU quota, not the logical CPUs of the machine -- divided by the
 * number of ranks that share the host.  That number is LOCAL_WORLD_SIZE (exported by torch.distributed.run) unless set here; the
 * handles driven by one rtx_raxtax_multi call divide their share among themselves. */
int rtx_set_host_share(uint32_t n_ranks_on_this_host);
uint32_t rtx_host_threads(void); /* threads a pool of this process may use (>= 1) */

#ifdef __cplusplus
}
#endif
#endif /* RAXTAX_HIP_H */

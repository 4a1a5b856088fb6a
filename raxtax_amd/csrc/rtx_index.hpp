// Internals of the device side of libraxtax_hip.so shared by its translation units (rtx_api_*.hip): the index handle, the buffer
// helpers and the functions that sequence the kernels of a sub-batch.  Not part of the ABI (include/raxtax_hip.h is).
//   rtx_api_index.hip     index creation (bitmaps, segment classes, union bitmap, locator, exact-match table), options
//   rtx_api_batch.hip     per-batch workspace, upload (prefetch / activate), the kernel sequence of a sub-batch, rtx_batch_run
//   rtx_api_download.hip  streamed download of the rows the device finalised (rtx_finalise.hip: sort lineage.rs:91-93, local signal lineage.rs:95-102)
//   rtx_api_shard.hip     the staged path of a sharded database (rtx_shard_*)
//   rtx_api_debug.hip     stage times, work counters, parity / debug taps
// There is deliberately no CPU fallback: without a gfx950 device every entry point returns RTX_ERR_NO_DEVICE.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "host_screen.hpp"
#include "rtx_internal.hpp"
#include "rtx_kernels.hpp"
#include "rtx_math.hpp"

using namespace rtx;

namespace rtxi {


constexpr uint32_t kEmptyRow = 0xFFFFFFFFu;
constexpr uint32_t kLnFactLen = 98320;  // covers t + n - 1 for every t <= 65535
constexpr size_t kProbTableLdsLimit = 160 * 1024 - 512;  // prob_table_kernel with its arrays in LDS up to here (rtx_api_batch.hip: length classes)

#define RTX_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_ == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP;                      \
        }                                                                                      \
    } while (0)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        if (count <= n && p) return RTX_OK;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
            return RTX_ERR_OOM;
        }
        n = count;
        return RTX_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    uint64_t bytes() const { return (uint64_t)n * sizeof(T); }
    ~DevBuf() { release(); }
};

// Pinned host array (hipHostMalloc): D2H copies of the result records run at PCIe rate and asynchronously.
template <class T>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0, n = 0;
    int resize(size_t count) {
        if (count > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            const size_t want = count + count / 4 + 16;
            if (hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault) != hipSuccess) {
                p = nullptr;
                cap = n = 0;
                set_error("hipHostMalloc(%zu bytes) failed", want * sizeof(T));
                return RTX_ERR_OOM;
            }
            cap = want;
        }
        n = count;
        return RTX_OK;
    }
    // room for `count` elements with the first `keep` of them preserved (the result rows of the sub-batches already copied); grows by doubling
    int grow_keep(size_t count, size_t keep) {
        if (count <= cap) { n = count; return RTX_OK; }
        T *q = nullptr;
        const size_t want = std::max(count + count / 4 + 16, cap * 2);
        if (hipHostMalloc((void **)&q, want * sizeof(T), hipHostMallocDefault) != hipSuccess) {
            set_error("hipHostMalloc(%zu bytes) failed", want * sizeof(T));
            return RTX_ERR_OOM;
        }
        if (p && keep) std::memcpy(q, p, std::min(keep, cap) * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q;
        cap = want;
        n = count;
        return RTX_OK;
    }
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
};

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

#ifndef RTX_PRUNE_MIN_TILES
#define RTX_PRUNE_MIN_TILES 4  // tiles of 8192 references from which on the tile pruning is worth its bounds pass (configs[1], 7 tiles: 5.6 -> 7.8 M queries/s; it was 8 until the bounds pass lost its stores)
#endif

}  // namespace rtxi
using namespace rtxi;

struct rtx_index {
    int device = -1;
    hipStream_t stream = nullptr;
    uint64_t n_refs = 0;    // references held by this handle (the whole database, or one shard of it)
    uint64_t n_total = 0;   // references of the whole database (Tree.num_tips)
    uint32_t ref_lo = 0;    // first global reference id of this shard
    uint32_t n_bnd_local = 0, bnd_first = 0;  // boundaries in (ref_lo, ref_hi] + 1; global index of ref_lo
    const double *ext_prefix = nullptr;       // sharded mode: assembled global prefix handed to the walk
    // ---- index proper
    uint32_t n_rows = 0;        // non-empty posting lists
    uint32_t stride_bytes = 0;  // bytes per bitmap row over all tiles (multiple of 1024)
    uint64_t npad = 0;          // references per padded row (= stride_bytes * 8)
    uint32_t ntiles = 0;        // 8192-reference tiles
    DevBuf<uint32_t> d_bitmap, d_row_of, d_list_len;
    DevBuf<uint2> d_row_len;    // {row_of, list_len} per k-mer (kmer_extract: one gather instead of two)
    // segment classes (rtx_segments.hip): class / sparse slot of every (row, tile) segment, slots of 32 local ids
    DevBuf<uint32_t> d_seginfo, d_seg_sbase, d_segcls;  // (d_segcls: the classes alone, [tile][row] two bits each)
    uint32_t cls_stride = 0;
    DevBuf<unsigned long long> d_seg_dbits, d_seg_sbits;
    uint32_t seg_blocks = 0;  // > 0: kmer_extract uses the bit tables (many tiles)
    DevBuf<uint16_t> d_segslots;
    uint64_t n_seg_slots = 0;
    uint32_t seg_stride = 0;
    DevBuf<double> d_lnfact, d_inv;
    // ---- memoised prob tables (t <= 1023), built lazily for the largest tmax seen
    int prob_mode = 0;  // 0 auto, 1 recurrence kernel only, 2 tables (error if they do not fit)
    uint32_t tab_tmax = 0;
    DevBuf<double> d_tab_cmf, d_tab_ratio;
    DevBuf<uint64_t> d_tab_off;
    DevBuf<uint32_t> d_tab_moff;
    DevBuf<uint16_t> d_tab_ilo, d_tab_sat;
    // ---- taxonomy
    FlatNodes nodes;
    std::vector<uint32_t> bnd;  // sorted unique range endpoints
    uint32_t n_bnd = 0;
    DevBuf<uint4> d_noderec;  // {blo, bhi, first_child, n_children | type << 30} per node (lineage_walk)
    // per node, for finalise_kernel (rtx_finalise.hip): depth, begin of its range (= the lineage a row reports), and the expected side of its
    // local signal ([node][fin_D] + the level it starts at; lineage.rs:95-98,137-139, rtx_math.hpp: fin_node_expected)
    DevBuf<uint8_t> d_node_depth, d_node_sig0;
    DevBuf<uint32_t> d_node_begin;
    DevBuf<double> d_node_eb;
    uint32_t fin_D = 1;  // levels of the deepest lineage = stride of the confidence arrays of a view
    DevBuf<uint32_t> d_bnd_rank;
    DevBuf<uint8_t> d_bnd_bits;
    // ---- exact-match lookup on the device (rtx_exact.hip): the distinct reference sequences ("groups") in a hash table
    uint32_t dev_exact_opt = 1;       // RTX_OPT_DEVICE_EXACT
    uint32_t nearest_opt = 0;         // RTX_OPT_NEAREST: 1 = every run also names the reference that holds each query's peak (rtx_nearest.hip)
    uint32_t identity_opt = 0;        // RTX_OPT_IDENTITY: 1 = every run also aligns each query to its nearest reference (rtx_identity.hip)
    DevBuf<uint32_t> d_em_ref_grp;    // [n_refs] reference -> its distinct sequence (built when the option is first switched on)
    uint32_t strand_opt = 0;          // RTX_OPT_STRAND: 1 = every query is classified in both orientations (rtx_strand.hip)
    bool strand_used = false;         // ... the activated batch holds the twins (queries n_user .. n_q - 1)
    uint64_t n_user = 0;              // queries of the activated batch as the caller passed them
    uint32_t em_groups = 0, em_bits = 0;
    uint64_t em_hash_mask = ~0ull;    // RTX_DEFAULT_EXACT_HASH_MASK at creation (tests: a weak hash, so that probes collide)
    DevBuf<uint2> d_em_table;         // [2^em_bits] {tag, group + 1}
    DevBuf<uint64_t> d_em_rep_off;    // [groups + 1]
    DevBuf<uint8_t> d_em_rep_bytes;   // the distinct sequences
    DevBuf<uint32_t> d_em_goff, d_em_gids;   // ids of group g: gids[goff[g] .. goff[g + 1]), ascending (tree.rs:109-112)
    std::vector<uint32_t> h_em_goff, h_em_gids;  // host copies: the ids behind the groups the device reports
    bool dev_exact_used = false;      // the activated batch came without ids: the device looks them up (every rtx_batch_run)
    struct HostExact {                // per host result set: the groups of a download and, on demand, the CSR of their ids
        std::vector<uint32_t> grp;
        std::vector<uint64_t> off;
        std::vector<uint32_t> ids;
        bool csr_valid = false, valid = false;
    } host_exact[2];
    // ---- batch inputs
    uint64_t n_q = 0;
    bool uploaded = false, ran = false, synced = false;
    uint32_t last_flags = 0;
    // ---- processing order of the batch (rtx_cluster.hip: ResultSet::d_perm, d_iperm)
    uint32_t cluster = 1;  // RTX_OPT_CLUSTER
    uint32_t packed_opt = 1;  // RTX_OPT_PACKED_COUNTS
    uint32_t tile_skip = 1;   // RTX_OPT_TILE_SKIP: taxon_prefix reads only the tiles that hold a reference with p >= 1e-30
    uint32_t pair_opt = 1;    // RTX_OPT_HIT_PAIR
    uint32_t prune_opt = 1;   // RTX_OPT_TILE_PRUNE: hit_count visits only the tiles that can hold a reference with any probability (rtx_prune.hip)
    uint32_t self_sample_opt = 1;  // RTX_OPT_PRUNE_SELF_SAMPLE: the verdict of rtx_index_self_sample is honoured
    bool prune_pays = true;        // ... which is: a sample of the database's own references keeps fewer than kSelfSampleOff of its tiles live
    double self_live = -1.0;       // the share of (query, tile) combinations the sample kept live (-1: no sample was taken)
    bool pruning() const { return prune_opt != 0u && (prune_pays || self_sample_opt == 0u); }  // tile pruning is on for this handle (where the batch allows it)
    bool dbg_full = false;    // the last sub-batch of the run was pruned (last_cls().prune) and the debug taps have recounted it in full since
    bool dbg_full_run = false;  // (the recount in progress: enqueue_hit leaves the pruning out)
    DevBuf<uint32_t> d_ubitmap;  // union bitmap: one column per block of 2^kPruneShift references, tile-major like d_bitmap
    uint32_t u_stride_bytes = 0, u_ntiles = 0;
    uint64_t u_nblocks = 0;
    // the fine union bitmap (blocks of 2^kFineShift = 8 references; databases of kFineMinTiles tiles or more, whole-database handles):
    // second stage of the bounds for the pairs the first stage leaves many live tiles (rtx_hit_pair.hip: launch_fine_bounds)
    DevBuf<uint32_t> d_fbitmap;
    uint32_t f_stride_bytes = 0, f_ntiles = 0;
    uint64_t f_nblocks = 0;
    uint32_t fine_opt = 1;  // RTX_OPT_FINE_BOUNDS
    // the bounds pass in two levels (rtx_bounds2.hip; whole-database handles): blocks of 256 references for every tile (four rows per load
    // instruction), blocks of 64 only for the B-tiles near the query's largest bound (sixteen rows per load instruction)
    DevBuf<uint32_t> d_abitmap;  // [n_atiles][n_rows + 1][64 words]
    DevBuf<uint8_t> d_bbitmap;   // [n_btiles][n_rows + 1][64 bytes]
    uint32_t n_atiles = 0, n_btiles = 0;
    DevBuf<uint8_t> d_cbitmap;   // the database block by block: [ceil(n_refs / 64)][n_rows + 1][8 bytes] (prune_kernel: exact counts of the best block)
    uint32_t two_level_opt = 1;  // RTX_OPT_TWO_LEVEL_BOUNDS
    uint32_t b2_delta[4] = {283u, 205u, 92u, 128u};  // which B-tiles are refined: c_t, c_m, lo, hi in 1/256 (Bounds2Params): dl = 1.105 t - 0.8 max within [0.36 t, 0.5 t]
    bool two_level_used = false;  // the last run's bounds pass was bounds2_kernel (its work accounting counts load instructions of 1 KiB)
    // The HBM diet of the counts buffer (round 6): a class that prunes with the records path holds sub_batch >> diet_shift rows of counts (at
    // least kDietMinRows); a run in which prune_kernel runs out of rows raises bit 2 of d_flags, the download lowers diet_shift and repeats it.
    uint32_t rec_seg_len = 1024;  // records per segment of the records path (RecordRef::seg_len): doubled, up to 8192, when a run's segment overflows
    uint32_t diet_shift = 3;
    uint32_t rec_opt = 4;   // RTX_OPT_RECORDS: pruned queries with at most this many live tiles take the records path (0: off; at most kRecMaxSlots)
    uint32_t rec_slots() const { return std::min<uint32_t>(rec_opt, kRecMaxSlots); }  // record segments per query (RecordRef::stride)
    uint32_t overlap_opt = 1;  // RTX_OPT_OVERLAP: 1 = back half of sub-batch k on a second stream beside the front half of k + 1 (2: three stages)
    uint32_t overlap_used = 0;  // scratch sets the last run used beside each other (0: one stream)
    hipStream_t stream2 = nullptr, stream3 = nullptr, hit_stream = nullptr;  // (hit_stream: where enqueue_hit launched the counting pass)
    std::vector<hipEvent_t> ev_front, ev_back, ev_mid;  // per sub-batch: front half enqueued (on stream), back half done (on stream2)
    DevBuf<unsigned long long> d_prune_stats;
    uint32_t shard_prune_opt = 0;  // RTX_OPT_SHARD_PRUNE: a reference shard prunes with the threshold of the whole database (rtx_shard_bounds)
    uint32_t debug_taps = 0;     // RTX_OPT_DEBUG_TAPS: prune_kernel leaves its view of every query (rtx_debug_prune_detail)
    DevBuf<uint32_t> d_prune_detail;  // [sub_batch][kPruneDetailWords]
    uint32_t locator_opt = 1; // RTX_OPT_LOCATOR: the sort key of the processing order is led by the query's position in the database
    DevBuf<uint32_t> d_loc_table;  // 12-mer -> lowest reference position (rtx_cluster.hip); only when built from sequences
    DevBuf<uint32_t> d_group_rows;
    uint32_t n_groups_run = 0;  // groups of the whole batch (n_sub * groups_per_sub): the second half of d_group_rows starts there
    uint32_t groups_per_sub = 0;
    bool packs(int pl) const { return packed_opt && pl <= 10; }  // counts of a class of `pl` bit planes travel packed (11 planes -- reads of 1 031 .. 2 054 bases on the pair kernel -- leave u16 counts)
    DevBuf<uint64_t> d_skey_in, d_skey_out;
    DevBuf<uint32_t> d_sidx;
    DevBuf<uint8_t> d_sort_tmp;
    DevBuf<uint8_t> d_bases;  // the current batch, one byte per base (what the kernels read): unpacked from the staged transfer at activation
    // Two input sets: a batch is STAGED (rtx_batch_prefetch: bases packed two per byte into pinned memory, offsets, exact-match ids;
    // asynchronous H2D on h2d_stream) while the batch before it runs out of the other set, and becomes the current one at
    // rtx_batch_activate.  rtx_batch_upload = prefetch + activate.
    struct Inputs {
        DevBuf<uint8_t> d_packed;          // bases two per byte (or raw, one per byte, if a byte above 15 was seen)
        DevBuf<uint64_t> d_base_off, d_exact_off;
        DevBuf<uint32_t> d_exact_ids;
        PinBuf<uint8_t> h_packed;
        PinBuf<uint64_t> h_base_off, h_exact_off;
        PinBuf<uint32_t> h_exact_ids;
        uint64_t n_q = 0, total = 0, max_len = 0, n_exact = 0;
        uint64_t n_user = 0;  // queries as the caller passed them: n_q, or half of it under RTX_OPT_STRAND (n_q counts the twins the activation appends; total does not)
        uint64_t cls_n[5] = {0, 0, 0, 0, 0}, cls_max[5] = {0, 0, 0, 0, 0};  // queries and longest query per length class (length_class)
        bool packed = true, has_exact = false, staged = false, recorded = false;
        // the labels of the batch (rtx_batch_prefetch_labels, staged before the bases: labels_pending becomes has_labels at the prefetch)
        DevBuf<char> d_labels;
        DevBuf<uint64_t> d_label_off;
        PinBuf<char> h_labels;
        PinBuf<uint64_t> h_label_off;
        uint64_t n_labels = 0;
        bool labels_pending = false, has_labels = false;
        // the weights of the batch for the taxon profile (rtx_batch_prefetch_weights: the path of the labels)
        DevBuf<uint32_t> d_weights;
        PinBuf<uint32_t> h_weights;
        uint64_t n_weights = 0;
        bool weights_pending = false, has_weights = false;
        // ... and its samples for the per-sample counters (rtx_batch_prefetch_samples: the same path)
        DevBuf<uint32_t> d_samples;
        PinBuf<uint32_t> h_samples;
        uint64_t n_samples = 0;
        bool samples_pending = false, has_samples = false;
        hipEvent_t ready = nullptr;        // its transfer has arrived
    } in[2];
    uint32_t cur_in = 0;               // the set of the current (activated) batch
    hipStream_t h2d_stream = nullptr;
    hipEvent_t ev_activated = nullptr; // on the handle's stream, behind everything that was enqueued before the current batch was activated:
                                       // the kernels that read the OTHER input set have run when it fires (a transfer into that set waits for it)
    uint64_t sum_query_bytes = 0;
    // ---- sub-batch scratch: two sets -- a staged (reference-sharded) run alternates between them, so that the exchange of
    // one sub-batch can overlap with the counting of the next; a whole-database handle uses set 0 only
    uint32_t sub_batch_req = 0;  // rtx_index_set_batch (0: sized against free HBM)
    uint32_t min_subs = 4;  // RTX_OPT_MIN_SUB_BATCHES: a pruned batch is cut into at least this many sub-batches (the host finalises one while the next run)
    uint64_t ws_key[14] = {0};  // shape and options the workspace was last prepared for (prepare_workspace)
    bool ws_valid = false;
    // ---- length classes of the batch (round 5; round 6: the class of t <= 2047).  t <= length - 7 decides how a query is counted (8 / 10 / 11 / 12 / 16 bit planes, the pair
    // kernel, tile pruning), how its probabilities are computed (memoised tables up to t = 2047, the recurrence kernel in LDS, the same
    // from global memory for reads of tens of kilobases) and how much scratch it needs.  A batch used to take ALL of that from its longest
    // query: one 1 100-base read in a file of COI barcodes moved every query off the fast path.  Now the class leads the sort key of the
    // processing order and every class is cut into sub-batches of its own shape (plan).  The shape of a class (tmax, strides, planes,
    // sub_batch, cnt_rows) and what it runs through (use_tables, pair, prune, rec, diet) are held HERE and nowhere else: a SubBatch names its
    // class (sub_batch_of), whoever fills kernel parameters reads it there, and the handle holds no "current class".  The taps read the class
    // of the last sub-batch (last_cls).  A reference shard and rtx_debug_evaluate have one class (prepare_workspace_single).  A STAGED run
    // (rtx_shard_*) has one row stride for its exchange buffers: every sub-batch of it is launched in the shape of cls[0] (shard_sb) -- which is
    // all there is on a reference shard; a k-mer shard holds every reference, so a batch of mixed lengths is cut into several classes there,
    // and its longer reads are clipped to class 0's strides as they always were.
    struct BatchClass {
        uint64_t pos0 = 0, n = 0, max_len = 0;  // positions [pos0, pos0 + n) of the processing order
        uint32_t tmax = 0, kstride = 0, rstride = 0, hstride = 0, sub_batch = 0, sb0 = 0, n_sub = 0;
        int planes = 10;
        // what its sub-batches run through: the memoised tables, hit_count_pair_kernel, tile pruning, the records path on offer (whole-database handle
        // that prunes, walk fused) -- decided by begin_run; huge: prob_table's arrays in global memory; will_prune: size_workspace's forecast of prune
        bool use_tables = false, pair = false, prune = false, rec = false, huge = false, will_prune = false;
        bool side = false;  // a handful of queries beside the bulk of the batch: they run FIRST, through a small scratch set of their own (kSideSet)
        bool diet = false;      // rows of the counts buffer are handed out by prune_kernel (behind tile pruning with the records path: HitParams::cnt_row)
        uint32_t cnt_rows = 0;  // rows of counts a sub-batch of the class lays out (diet: a fraction of sub_batch)
    } cls[5];
    uint32_t n_cls = 0;
    uint64_t key_lim[4] = {~0ull, ~0ull, ~0ull, ~0ull};  // sort rank of a query = the number of these lengths it exceeds
    struct SubPlan { uint64_t q0; uint32_t nq, cls; };  // a sub-batch of the run: first position of the processing order, queries, index of its class
    std::vector<SubPlan> plan;      // plan_sub_batches: whenever the workspace is sized and at the start of every run (an upload of the shape of the last one keeps
                                    // the plan it finds: ws_valid).  `uploaded` implies a workspace sized for at least one query: never empty behind an upload
    uint32_t n_sub_total() const { return (uint32_t)plan.size(); }
    uint32_t sub_batch_max = 0;
    bool any_prune = false;  // some class of the last run pruned (rtx_debug_prune_stats sums over the run)
    DevBuf<double> d_prob_scratch;  // prob_table_kernel's arrays of a class of very long reads (they do not fit LDS)
    struct Scratch {
        DevBuf<uint16_t> d_kmers, d_counts, d_tilemax;
        DevBuf<uint32_t> d_rows, d_t, d_nrows, d_hist, d_order, d_srows, d_nsparse;
        DevBuf<unsigned long long> d_dmask;
        DevBuf<double> d_table_z, d_prefix;
        DevBuf<uint2> d_urec;   // hit_count_pair_kernel: union row lists of the pairs of the sub-batch
        DevBuf<uint32_t> d_nu;
        // tile pruning: the queries counted against the union bitmap (every row dense) leave the largest bound of
        // every tile and the best block (bounds_epilogue); thresholds and the live tiles per pair (prune_kernel)
        DevBuf<uint32_t> d_live, d_best_key;  // (d_live: LiveLayout)
        DevBuf<uint32_t> d_items;  // the (pair, tile) blocks with a live query, live tiles per pair, offsets (ItemsLayout)
        DevBuf<uint16_t> d_tile_ub, d_prune_thr, d_prune_i1;
        DevBuf<uint32_t> d_best;  // [B][kPruneBestWords] reference shards: the candidate for the best block of the database
        DevBuf<uint8_t> d_heavy;        // two-level bounds pass: [B] queries left to the one-level pass (Bounds2Params::heavy)
        DevBuf<uint32_t> d_heavy_items; // ... and the (pair, union tile) items of that pass (HeavyItemsLayout)
        DevBuf<uint32_t> d_fine_items;  // fine bounds pass: its items and cursors (FineItemsLayout)
        // the records path (RecordRef, rtx_kernels.hpp): per query the live tiles at prune time, the records of each, their number
        DevBuf<uint16_t> d_rec_nslots, d_rec_slots;
        DevBuf<uint32_t> d_rec_cnt, d_rec;
        DevBuf<uint32_t> d_cnt_row, d_cnt_cursor;  // [B] row of the counts buffer per query | [1] rows handed out (HitParams::cnt_row)
        DevBuf<uint32_t> d_dense_q;                // [cnt_rows] the query that holds each row handed out (PruneParams::dense_q)
        // every buffer of a set, once: what release_all and bytes() (and whoever else wants all of them) walk
        template <class S, class F>
        static void each(S &s, F &&f) {
            f(s.d_kmers); f(s.d_counts); f(s.d_tilemax); f(s.d_rows); f(s.d_t); f(s.d_nrows); f(s.d_hist); f(s.d_order); f(s.d_srows); f(s.d_nsparse);
            f(s.d_dmask); f(s.d_table_z); f(s.d_prefix); f(s.d_urec); f(s.d_nu); f(s.d_live); f(s.d_best_key); f(s.d_items); f(s.d_tile_ub); f(s.d_prune_thr);
            f(s.d_prune_i1); f(s.d_best); f(s.d_heavy); f(s.d_heavy_items); f(s.d_fine_items); f(s.d_rec_nslots); f(s.d_rec_slots); f(s.d_rec_cnt); f(s.d_rec);
            f(s.d_cnt_row); f(s.d_cnt_cursor); f(s.d_dense_q);
        }
        void release_all() { each(*this, [](auto &b) { b.release(); }); }
        // HBM of the set as rtx_index_workspace_bytes reports it.  d_cnt_row and d_cnt_cursor are left out: the reported figure never held them
        // (hbm_bytes of the bench line is compared to the byte); counting them changes that figure and is a change of its own.
        uint64_t bytes() const {
            uint64_t b = 0;
            each(*this, [&](const auto &buf) { b += buf.bytes(); });
            return b - d_cnt_row.bytes() - d_cnt_cursor.bytes();
        }
    } sc[4];  // 0 .. 2: the sets that alternate (RTX_OPT_OVERLAP, rtx_shard_*); 3: the set of the side classes (a few long reads among barcodes)
    bool staged = false;  // driven with rtx_shard_*: sub-batch sb works in scratch set sb & 1, so that the exchange of one
                          // sub-batch (RCCL, on the caller's stream) can overlap with the counting of the next
    uint32_t last_set = 0;  // scratch set of the last sub-batch (debug taps)
    const BatchClass &last_cls() const { return cls[staged ? 0u : plan.back().cls]; }  // ... and the class it ran in the shape of (the last of the bulk: plan_sub_batches; staged: cls[0])
    DevBuf<double> d_probs_dbg;
    DevBuf<uint16_t> d_counts_dbg;
    DevBuf<unsigned long long> d_sub_alloc;  // WalkParams::sub_alloc
    // ---- the results of a batch, in two sets.  RTX_OPT_RUN_AHEAD (set by rtx_raxtax for its chunks): rtx_batch_download_then_run enqueues the
    // staged batch BEFORE the last sub-batch of the batch being downloaded has finished, so that the front half of the next chunk's first
    // sub-batch runs beside the back half of this chunk's last one (the two streams of RTX_OPT_OVERLAP then never drain between chunks).
    // Everything a batch writes per query and per row, and what its download reads, is in the set the batch was enqueued into (res()); the
    // download is handed that set.  The scratch sets are shared (a front half waits for the back half that last used its set: ev_set_free).
    struct ResultSet {
        DevBuf<uint8_t> d_status;
        DevBuf<uint32_t> d_t_all, d_nrows_all, d_n_rows, d_flags, d_ndist;
        DevBuf<double> d_gs, d_z;
        DevBuf<unsigned long long> d_hq, d_row_start, d_cursor;
        DevBuf<DevRow> d_arena;
        uint64_t arena_cap = 0;
        uint64_t side_base = 0;  // rows [side_base, arena_cap) take the result rows of the side classes (their walks run beside the bulk's: a cursor of their own, d_cursor[1])
        PinBuf<unsigned long long> h_side_base;  // the two cursors the run starts from (begin_run: asynchronous H2D)
        // the final result arrays (finalise_kernel): the per-query fields in input order, the rows back to back from 0 on (fin_cap = arena_cap rows)
        DevBuf<uint32_t> d_fin_t, d_fin_row_count, d_fin_lineage, d_fin_node, d_fin_depth;
        DevBuf<uint8_t> d_fin_status, d_fin_depth8, d_fin_hund;
        DevBuf<double> d_fin_gs, d_fin_local, d_fin_conf;
        DevBuf<unsigned long long> d_fin_row_begin, d_fin_cursor;
        uint64_t fin_cap = 0;
        DevBuf<uint32_t> d_perm, d_iperm;  // the processing order (rtx_cluster.hip): perm[position] = query, iperm[query] = position
        DevBuf<uint32_t> d_exact_grp;      // [n_q] group of every query of the batch (0xFFFFFFFF: none)
        // rtx_strand.hip: the peak of every query of the batch (peak_kernel, per sub-batch), and behind the last sub-batch the strand and the peak of
        // the caller's queries (strand_select_kernel) -- under RTX_OPT_STRAND with the final per-query fields of the chosen orientation, which the
        // download copies in the place of d_fin_*.  (Not part of bytes(): a few bytes per query that the reported figure never held.)
        DevBuf<uint32_t> d_peak2, d_peak, d_sel_t, d_sel_row_count;
        DevBuf<uint8_t> d_strand, d_sel_status;
        DevBuf<double> d_sel_gs;
        DevBuf<unsigned long long> d_sel_row_begin;
        hipEvent_t ev_select = nullptr;    // behind strand_select_kernel
        // rtx_nearest.hip (RTX_OPT_NEAREST; not allocated without it): nearest reference and ties of every query of the batch (nearest_kernel, per
        // sub-batch), and of the caller's queries (strand_select_kernel, beside d_peak)
        DevBuf<uint32_t> d_nearest2, d_ties2, d_nearest, d_ties;
        bool has_nearest = false;          // the run fills them
        // rtx_identity.hip (RTX_OPT_IDENTITY; not allocated without it): distance to the nearest reference and length of the caller's queries
        DevBuf<uint32_t> d_dist, d_qlen;
        bool has_identity = false;         // the run fills them
        uint64_t n_user = 0;               // queries as the caller passed them (n_q counts the twins as well)
        bool has_peak = false;             // the run filled d_peak2 (enqueue_batch; not a staged run or rtx_debug_evaluate)
        hipEvent_t ev_exact = nullptr;     // behind exact_match_kernel of the run: the download fetches the groups at its START, beside the kernels, not at its tail
        PinBuf<uint32_t> h_flags;          // the run's flags (d_flags), copied behind its last kernel: the download reads them without a round trip of its own
        hipEvent_t ev_flags = nullptr;     // ... behind that copy
        // streamed download: per sub-batch an event, the arena cursor and the cursor of the final rows behind it; rtx_batch_download copies
        // the rows of finished sub-batches on `copy_stream` while later ones are still running
        std::vector<hipEvent_t> ev_sub;
        PinBuf<unsigned long long> h_cursor_sub, h_fin_sub;
        // the batch in the set, as its download needs it (begin_run, enqueue_batch, rtx_debug_evaluate)
        uint64_t n_q = 0;
        uint32_t n_sub = 0, n_side = 0;  // sub-batches; those of the side classes among them (the first ones)
        uint32_t in_set = 0;             // its input set (in[])
        bool dev_exact = false;          // the device looked its exact matches up (d_exact_grp)
        bool stream_dl = false;          // the streamed download applies (ev_sub, h_cursor_sub, h_fin_sub are recorded)
        bool profiled = false;           // the run in the set has been added to the open profile (a second download of it adds nothing; record_batch clears it)
        // HBM as rtx_index_workspace_parts counts it: the processing order (part [6]), the exact-match groups ([5]), the rest ([7]; flags and cursors uncounted)
        struct Bytes { uint64_t order, groups, rest; };
        Bytes bytes() const {
            return {(d_perm.n + d_iperm.n) * 4, d_exact_grp.n * 4,
                    d_status.n + (d_t_all.n + d_nrows_all.n + d_n_rows.n + d_ndist.n) * 4 + (d_gs.n + d_z.n + d_hq.n + d_row_start.n) * 8 + d_arena.n * sizeof(DevRow) +
                        (d_fin_t.n + d_fin_row_count.n + d_fin_lineage.n + d_fin_node.n + d_fin_depth.n) * 4 + d_fin_status.n + d_fin_depth8.n + d_fin_hund.n +
                        (d_fin_gs.n + d_fin_local.n + d_fin_conf.n + d_fin_row_begin.n) * 8};
        }
        void destroy_events() {  // (rtx_index's destructor: before the streams they were recorded on, as every event of the handle)
            for (auto e : ev_sub) (void)hipEventDestroy(e);
            if (ev_exact) (void)hipEventDestroy(ev_exact);
            if (ev_flags) (void)hipEventDestroy(ev_flags);
            if (ev_select) (void)hipEventDestroy(ev_select);
        }
    } rs[2];
    uint32_t rs_w = 0;  // the set the batch being enqueued writes (after a run: that run's)
    ResultSet &res() { return rs[rs_w]; }
    // ---- timing
    std::vector<hipEvent_t> events;  // 2 per (sub-batch, stage)
    uint32_t n_sub_last = 0;
    std::vector<hipEvent_t> ev_near;  // 2 per sub-batch around nearest_kernel (RTX_OPT_NEAREST under RTX_OPT_STAGE_TIMING: rtx_batch_nearest_time)
    uint32_t n_near_last = 0;         // sub-batches of the last run that recorded them
    hipEvent_t ev_ident[2] = {nullptr, nullptr};  // around the kernels of rtx_identity.hip (RTX_OPT_IDENTITY under RTX_OPT_STAGE_TIMING: rtx_batch_identity_time)
    bool ident_timed = false;         // the last run recorded them
    // ---- host results
    // two alternating sets: the view of download c stays valid while batch c+1 runs and is downloaded
    // (page-locked: the device's final arrays are copied straight into them, rtx_api_download.hip)
    struct HostRes {
        PinBuf<uint32_t> v_row_lineage, v_row_node, v_row_depth;
        PinBuf<uint8_t> v_row_depth8, v_row_hund;
        PinBuf<uint32_t> h_t;
        PinBuf<uint8_t> h_status;
        PinBuf<double> v_row_conf, v_row_local;
        PinBuf<double> h_gs;
        PinBuf<unsigned long long> v_row_begin;  // by query; the rows themselves are in processing order
        PinBuf<uint32_t> v_row_count;
        PinBuf<uint8_t> h_strand;  // rtx_batch_strands
        PinBuf<uint32_t> h_peak;
        PinBuf<uint32_t> h_nearest, h_ties;  // rtx_batch_nearest (sized only under RTX_OPT_NEAREST)
        bool has_nearest = false;  // the download's run had RTX_OPT_NEAREST on
        PinBuf<uint32_t> h_dist, h_qlen;  // rtx_batch_identity (sized only under RTX_OPT_IDENTITY)
        bool has_identity = false; // the download's run had RTX_OPT_IDENTITY on
        uint64_t n_user = 0;       // queries of the view
        bool both = false;         // the download ran under RTX_OPT_STRAND: the exact matches are those of the chosen orientation
    } host_res[2];
    uint32_t res_set = 0;
    PinBuf<uint32_t> h_nrows_all;
    // ---- device text (rtx_text.hip): the lineage table of rtx_index_text_setup, the passes' scratch, the text of the downloads (one per host
    // result set, valid as long as its view)
    bool text_on = false;
    uint32_t text_flags = 0;
    uint64_t text_tree_uid = 0;      // rtx_tree::uid of the tree the lineage table was uploaded from
    uint32_t device_text_opt = 0;    // RTX_OPT_DEVICE_TEXT
    uint32_t derep_opt = 0;          // RTX_OPT_DEREP: rtx_raxtax* classify each distinct read of a chunk once (rtx_derep.hip); the handle itself never reads it
    rtx_qual_params quality{};       // rtx_index_set_quality: rtx_raxtax* filter every read by its quality string (rtx_qual.hip); the handle itself never reads it
    bool quality_on = false;
    rtx_chimera_params chimera{};    // rtx_index_set_chimera: the chimera check its callers run in front of it (rtx_chimera.hip); the handle itself never reads it
    bool chimera_on = false;
    rtx_screen_set screen_set;       // rtx_index_set_screen: the contaminant screen rtx_raxtax* run every read through (rtx_screen.hip); the handle itself never reads it
    rtx_screen_params screen{};      // (screen_set.data is null: off)
    rtx_tally *tally = nullptr;      // rtx_index_set_tally: the object rtx_raxtax* tally the classified reads into (rtx_tally.hip), the caller's; the handle itself never reads it
    rtx::DemuxList tags;  // rtx_index_set_tags: rtx_raxtax* assign every read to a sample and cut its tags first (rtx_demux.hip); the handle itself never reads them
    std::vector<rtx::TrimPrimer> primers;  // rtx_index_set_primers: rtx_raxtax* trim every read with them first (rtx_trim.hip); the handle itself never reads them
    DevBuf<char> d_lin_bytes, d_text;
    DevBuf<uint64_t> d_lin_off;
    DevBuf<uint8_t> d_lin_depth, d_text_tmp;
    DevBuf<unsigned long long> d_text_len, d_text_off;
    struct HostText {
        PinBuf<char> out, tsv;
        PinBuf<uint64_t> out_off, tsv_off;
        uint64_t nq = 0;
        bool valid = false, tsv_on = false;
    } host_text[2];
    hipStream_t copy_stream = nullptr;  // the copies of the streamed download (ResultSet::ev_sub)
    PinBuf<unsigned long long> h_hq;
    uint32_t stage_timing = 0;  // 0: HIP events around hit_count only; 1: around every kernel

    // ---- run-ahead (ResultSet above)
    uint32_t run_ahead_opt = 0;      // RTX_OPT_RUN_AHEAD
    bool join_pending = false;       // the last run left out the join of the handle's stream with the stream of its back halves (settle_join enqueues it)
    hipEvent_t join_ev = nullptr;    // ... which is a wait for this event (the run's last ev_back)
    bool hold_join = false;          // a run-ahead is being enqueued: the join of the batch before it is dropped, not enqueued
    hipEvent_t ev_set_free[3] = {nullptr, nullptr, nullptr};  // behind the back half that last used scratch set k
    bool set_busy[3] = {false, false, false};
    uint64_t n_run_ahead = 0, n_run_ahead_retry = 0;  // chunks enqueued ahead / run-aheads abandoned for an overflow of the chunk before (rtx_index_run_ahead_stats)

    // ---- the taxon profile (rtx_index_profile_*, rtx_profile.hip): open between begin and end, nothing of it exists otherwise.  Every accepted
    // download adds its batch once (enqueue_profile, where enqueue_text is called); a run that is repeated or abandoned has added nothing.
    struct Profile {
        bool on = false;
        uint32_t cutoff = 0, flags = 0;        // hundredths; RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE (either one: no override)
        DevBuf<unsigned long long> d_acc;      // clade | direct | conf_sum ([n_nodes] each) | totals [4]
        // a parent per node rather than an [n_nodes][D] table of ancestors: 4 bytes per node against 128, and the climb of at most D dependent loads
        // hits a table that stays in L2 (2 MB at 500 000 nodes); the Taxon node of every reference for the override
        DevBuf<uint32_t> d_parent, d_ref_leaf;
        std::vector<uint64_t> h_acc;           // rtx_index_profile_read: valid until the next read, reset or end
        // the per-sample counters (rtx_index_profile_begin_samples; n_samples == 0: none): direct [n_samples][n_nodes] | totals [n_samples][4]
        uint32_t n_samples = 0;
        DevBuf<unsigned long long> d_by_sample;
        std::vector<uint64_t> h_by_sample;     // rtx_index_profile_read_samples
        float ms = 0.f;                        // RTX_OPT_STAGE_TIMING: the kernel's time and launches since begin or reset
        uint32_t launches = 0;
        hipEvent_t ev[2] = {nullptr, nullptr};
    } prof;

    bool shared_device = false;  // rtx_raxtax_multi drives another handle on the same device beside this one: no second stream (begin_run)
    ~rtx_index() {
        for (auto e : events) (void)hipEventDestroy(e);
        for (auto e : prof.ev)
            if (e) (void)hipEventDestroy(e);
        for (auto e : ev_near) (void)hipEventDestroy(e);
        for (auto e : ev_ident)
            if (e) (void)hipEventDestroy(e);
        for (auto &r : rs) r.destroy_events();
        for (auto e : ev_set_free)
            if (e) (void)hipEventDestroy(e);
        for (auto e : ev_front) (void)hipEventDestroy(e);
        for (auto e : ev_back) (void)hipEventDestroy(e);
        for (auto e : ev_mid) (void)hipEventDestroy(e);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream3) (void)hipStreamDestroy(stream3);
        for (auto &i : in)
            if (i.ready) (void)hipEventDestroy(i.ready);
        if (ev_activated) (void)hipEventDestroy(ev_activated);
        if (h2d_stream) (void)hipStreamDestroy(h2d_stream);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace rtxi {

// ---- rtx_api_batch.hip
int bind(rtx_index *ix);
int ensure_events(rtx_index *ix, size_t count);

// One sub-batch = three groups of kernels.  A whole-database handle runs them back to back; a
// reference-sharded handle (config 5) stops after each group for the exchange with the other shards.
struct SubBatch {
    uint32_t sb, nq, set;
    uint64_t q0;
    const rtx_index::BatchClass *cls;  // the length class its kernels are launched in the shape of
    hipStream_t s;   // main stream
    bool timed;      // HIP events around hit_count (the roofline kernel)
    bool timed_all;  // ... and around every other kernel (RTX_OPT_STAGE_TIMING)
};
SubBatch sub_batch_of(rtx_index *ix, uint32_t sb, bool timed);
uint8_t *counts_lo(rtx_index *ix, rtx_index::Scratch &sc);
uint16_t *counts_hi(rtx_index *ix, const rtx_index::BatchClass &k, rtx_index::Scratch &sc);
uint32_t counts_rows_layout(const rtx_index *ix, const rtx_index::BatchClass &k);  // rows the counts buffer of a sub-batch of class k is laid out for right now (the diet's, or one per query)
uint32_t diet_rows(const rtx_index *ix, uint32_t B);
int ensure_full_counts(rtx_index *ix, const rtx_index::BatchClass &k, rtx_index::Scratch &sc);  // a row per query of a sub-batch of class k (the recounting taps)
hipEvent_t stage_event(rtx_index *ix, const SubBatch &b, int stage, int which);
int enqueue_kmer(rtx_index *ix, const SubBatch &b, hipStream_t s);
int enqueue_hit(rtx_index *ix, const SubBatch &b, uint32_t flags, hipStream_t s, int part = 0, hipStream_t s_mid = nullptr);
int enqueue_count(rtx_index *ix, const SubBatch &b, uint32_t flags, hipStream_t s_mid = nullptr);
int enqueue_prob_prefix(rtx_index *ix, const SubBatch &b, bool fuse_walk, bool prob_only = false);
int enqueue_walk(rtx_index *ix, const SubBatch &b, const double *prefix, hipStream_t s);
int order_batch(rtx_index *ix, bool cluster);
void record_batch(rtx_index *ix);
int begin_run(rtx_index *ix, uint32_t *n_sub_out, bool *timed_out, bool cluster);
int enqueue_batch(rtx_index *ix, uint32_t flags);
int ensure_prob_tables(rtx_index *ix, uint32_t tmax, bool *usable);
uint32_t length_class(uint64_t len);
uint64_t class3_max_len();  // 0: t <= 255, 1: t <= 1023, 2: t <= 2047, 3: longer, prob_table in LDS, 4: longer still
int prepare_workspace(rtx_index *ix, uint64_t n_queries, const uint64_t cls_n[5], const uint64_t cls_max[5]);
int prepare_workspace_single(rtx_index *ix, uint64_t n_queries, uint64_t tmax, uint64_t max_len);  // one class whatever the lengths
int plan_sub_batches(rtx_index *ix);
int alloc_scratch_set(rtx_index *ix, uint32_t k);
constexpr uint32_t kSideSet = 3;
// ---- rtx_api_download.hip
int node_tables(rtx_index *ix);  // the per-node tables of finalise_kernel, uploaded at creation
int alloc_result_set(rtx_index *ix, rtx_index::ResultSet &r, uint64_t n_queries, uint64_t min_arena = 0);  // (rtx_api_batch.hip) the per-query arrays, the arena and the final arrays of a set
int settle_join(rtx_index *ix);        // (rtx_api_batch.hip) the handle's stream waits for the back halves of the last run, if that run left the join out
int alloc_final(rtx_index *ix, rtx_index::ResultSet &r, uint64_t n_queries);  // (rtx_api_batch.hip) the final result arrays: n_queries per-query fields, arena_cap rows
int enqueue_finalise(rtx_index *ix, const SubBatch &b, hipStream_t s);  // (rtx_api_batch.hip) behind the walks of a sub-batch
int enqueue_profile(rtx_index *ix, rtx_index::ResultSet &r);  // the batch being downloaded joins the open profile, once (synchronous; nothing without one)
// ---- rtx_derep.hip
void set_derep_hash_mask(uint64_t mask);  // RTX_DEFAULT_DEREP_HASH_MASK (rtx_set_default_option)
void set_tally_hash_mask(uint64_t mask);  // RTX_DEFAULT_TALLY_HASH_MASK, rtx_tally.hip
void set_otu_hash_mask(uint64_t mask);    // RTX_DEFAULT_OTU_HASH_MASK, rtx_otu.hip
void set_chimera_slice(uint64_t cap);     // RTX_DEFAULT_CHIMERA_SLICE, rtx_chimera.hip
void set_unoise_slice(uint64_t cap);      // RTX_DEFAULT_UNOISE_SLICE, rtx_unoise.hip
uint64_t chimera_slice_cap();             // the reads or entries a slice of rtx_chimera_run / rtx_denovo_check may hold at most (all ones: no cap)
// ---- rtx_text.hip
int enqueue_text(rtx_index *ix, const rtx_index::ResultSet &r);  // the text of the batch being downloaded (synchronous)

// ---- The scratch sets described once: the layouts of the buffers that hold several arrays, the elements a set wants of every buffer
// (ScratchNeed) and the estimate that sizes a sub-batch against free HBM (class_per_q).  Whoever allocates, checks or reads a scratch
// buffer takes its numbers from here.  SIZES are computed from the sub-batch size B a set is allocated for, OFFSETS from the queries nq
// of the sub-batch being enqueued: the kernels index by nq.

// A list of (pair, tile) items as the kernels that fill it and walk it lay it out: [pairs x tiles] items | [1] their number | [8] queue per XCD
//
// The header (count(): n_items[0 .. 8]) of a list that is built by more than one workgroup holds counters that are ADDED to, so it has to be zero
// when the sub-batch starts.  The invariant, for the counting list (ItemsLayout) and the fine list (FineItemsLayout, with its cursors):
//   zeroed by  kmer_extract_kernel<false>, workgroup 0 (KmerParams::zero, filled in by enqueue_kmer): the first kernel of a sub-batch on its
//              scratch set, enqueued behind the wait for the set's previous user (ev_back / ev_set_free in enqueue_batch; one stream otherwise).
//              A reference shard's part 2 (rtx_shard_count) finds them as the kmer_extract of its part 1 left them: nothing in between adds.
//              The offsets depend on nq, so enqueue_kmer and enqueue_hit of a sub-batch must be handed the same SubBatch -- they are.
//   added to   [0] by live_items_kernel (a group's stretch of the list) or fine_count_kernel (tickets, then the length, stored by the last
//              workgroup); [1 .. 8] by the ONE launch of hit_count_pair_kernel that walks the list.  Each list is walked once per sub-batch.
//   read by    that launch of hit_count_pair_kernel ([0]: the length).  Nothing resets them afterwards: the next sub-batch's kmer_extract does.
// Both scratch sets and the chunks of a run-ahead have lists of their own (they live in the set), so no two sub-batches in flight share a header.
// The heavy list (HeavyItemsLayout) is built by one workgroup, which stores its header itself (heavy_items_kernel).
struct ItemList {
    size_t np, ntiles;  // pairs of queries; tiles per pair
    ItemList(size_t nq, size_t tiles) : np((nq + 1u) / 2u), ntiles(tiles) {}
    size_t cap() const { return np * ntiles; }
    size_t end() const { return cap() + 9u; }
    uint32_t *items(uint32_t *p) const { return p; }
    uint32_t *count(uint32_t *p) const { return p + cap(); }
};
struct ItemsLayout : ItemList {  // d_items (tiles of the database): the list (launch_live_items) | [pairs] live tiles per pair (prune_kernel)
    using ItemList::ItemList;
    size_t total() const { return end() + np; }
    uint32_t *pair_live(uint32_t *p) const { return p + end(); }
};
struct FineItemsLayout : ItemList {  // d_fine_items (tiles of the fine union bitmap): the list | [tiles] cursors (launch_fine_bounds)
    using ItemList::ItemList;
    size_t total() const { return end() + ntiles; }
    uint32_t *cursors(uint32_t *p) const { return p + end(); }
};
struct HeavyItemsLayout : ItemList {  // d_heavy_items (tiles of the union bitmap): the list alone (launch_bounds2)
    using ItemList::ItemList;
    size_t total() const { return end(); }
};
struct LiveLayout {  // d_live: [B + 1] masks of live tiles, (tiles + 31) / 32 + 1 words each
    uint32_t ntiles;
    uint32_t words() const { return (ntiles + 31u) / 32u + 1u; }
    size_t total(size_t B) const { return (B + 1u) * words(); }
};

// u16 elements of d_counts for `rows` rows: 10 bits per reference where the class packs its counts, a u16 otherwise
inline size_t counts_elems(const rtx_index *ix, int planes, size_t rows) { return ix->packs(planes) ? rows * ix->npad * 5 / 8 : rows * ix->npad; }

// Elements wanted of every buffer of a scratch set (named as the member of rtx_index::Scratch without its d_).  The numbers alone: which
// groups a handle allocates at all, and which of them it can do without, is alloc_scratch_set's business.
struct ScratchNeed {
    size_t kmers = 0, rows = 0, dmask = 0, counts = 0, hist = 0 /* d_hist and d_table_z */, prefix = 0, urec = 0;  // by the shape of a class (add_class)
    size_t prob_scratch = 0;                                                                                        // ... (rtx_index::d_prob_scratch, shared by the sets)
    size_t nsparse = 0, srows = 0, t = 0, nrows = 0, order = 0, tilemax = 0, nu = 0;                                // by the number of queries (set_queries)
    size_t tile_ub = 0, best_key = 0, prune_thr = 0, prune_i1 = 0, best = 0, live = 0, items = 0;                   // ... tile pruning
    size_t heavy = 0, heavy_items = 0, fine_items = 0;                                                              // ... two-level bounds, fine bounds
    size_t rec_nslots = 0, rec_slots = 0, rec_cnt = 0, rec = 0, cnt_row = 0, cnt_cursor = 0;                        // ... the records path and the diet
    size_t dense_q = 0;                                                                                             // ... the diet, by its rows (add_class)
    ScratchNeed &set_queries(const rtx_index *ix, size_t B) {  // a sub-batch of B queries, whatever their class
        const size_t nt = ix->ntiles;
        t = nrows = order = best_key = prune_thr = prune_i1 = rec_nslots = cnt_row = B;
        nsparse = tilemax = tile_ub = B * nt;
        srows = B * nt * (kSegMaxSparseRows + 1);
        nu = (B + 1u) / 2u;
        best = B * kPruneBestWords;
        live = LiveLayout{ix->ntiles}.total(B);
        items = ItemsLayout(B, nt).total();
        heavy = B + 1u;
        heavy_items = HeavyItemsLayout(B, ix->u_ntiles).total();
        fine_items = FineItemsLayout(B, ix->f_ntiles).total();
        rec_slots = rec_cnt = B * kRecMaxSlots;
        rec = B * ix->rec_slots() * ix->rec_seg_len;
        cnt_cursor = 4;
        return *this;
    }
    // ... of class kc, with cnt_rows rows of counts and of boundary prefix sums (the diet's, or B); raises what an earlier class left
    void add_class(const rtx_index *ix, const rtx_index::BatchClass &kc, size_t B, size_t cnt_rows) {
        auto up = [](size_t &a, size_t v) { a = std::max(a, v); };
        up(kmers, B * kc.kstride);
        up(rows, B * kc.rstride);
        up(dmask, B * ix->ntiles * (kc.rstride / 64));
        up(counts, counts_elems(ix, kc.planes, cnt_rows));
        up(prefix, cnt_rows * ix->n_bnd_local);
        up(dense_q, cnt_rows);
        up(hist, B * kc.hstride);
        up(urec, ((B + 1u) / 2u) * 2u * kc.rstride);
        if (kc.huge) up(prob_scratch, B * ((prob_table_lds_bytes(kc.tmax) + 7) / 8));
    }
};

// What scratch set k wants: every buffer sized for the class that needs most of it (set 3 serves the side classes, the others the bulk).
inline ScratchNeed scratch_set_need(const rtx_index *ix, uint32_t k) {
    ScratchNeed n;
    size_t b_max = 1;
    for (uint32_t c = 0; c < ix->n_cls; c++) {
        const rtx_index::BatchClass &kc = ix->cls[c];
        if (kc.side != (k == kSideSet)) continue;
        const size_t B = kc.sub_batch;
        b_max = std::max(b_max, B);
        // (a class that will prune with the records path starts with a fraction of the rows: begin_run enlarges the buffer if the run turns out otherwise)
        const bool diet = kc.will_prune && ix->rec_opt != 0u && ix->n_refs == ix->n_total && ix->n_bnd_local == ix->n_bnd;
        n.add_class(ix, kc, B, diet ? diet_rows(ix, (uint32_t)B) : B);
    }
    return n.set_queries(ix, b_max);
}

// Scratch bytes a sub-batch of class k costs per query: what size_workspace divides free HBM by.  An ESTIMATE, not the sum of ScratchNeed:
// the sub-batch size, and through it every result of the bench, follows from its value.
inline uint64_t class_per_q(const rtx_index *ix, const rtx_index::BatchClass &k) {
    return (uint64_t)k.kstride * 2 + (uint64_t)k.rstride * 12 + 4 + (uint64_t)ix->ntiles * (k.rstride / 8 + ((kSegMaxSparseRows + 1) * 4 + 10)) + (ix->packs(k.planes) ? ix->npad * 5 / 4 : ix->npad * 2) +
           (uint64_t)k.hstride * 12 + (uint64_t)ix->n_bnd_local * 8 + 64 + (k.huge ? prob_table_lds_bytes(k.tmax) : 0) +
           // + the scratch of the tile pruning: tile bounds, thresholds, live masks, best blocks, the lists of live blocks
           (k.will_prune ? (uint64_t)ix->ntiles * 2 + 12 + (ix->ntiles + 31u) / 32u * 2u + 2u + kPruneBestWords * 4 +
                               ((uint64_t)ix->ntiles + 2u) * 2u  /* the list of live (pair, tile) blocks: 4 bytes per pair and tile */ +
                               (ix->d_fbitmap.p ? (uint64_t)ix->f_ntiles * 2u + 1u : 0u) /* the items of the fine bounds pass */ +
                               (ix->rec_opt && ix->n_refs == ix->n_total ? (uint64_t)std::min<uint32_t>(ix->rec_opt, kRecMaxSlots) * 32768u + kRecMaxSlots * 6u + 2u : 0u) /* record segments */
                           : 0);
}

}  // namespace rtxi

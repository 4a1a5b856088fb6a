// The per-batch workspace, the upload (rtx_batch_prefetch / rtx_batch_activate) and the kernel sequence of a sub-batch on the handle's HIP
// stream: order -> kmer_extract -> [pair_union] -> [bounds -> prune -> lists of the live tiles] -> hit_count -> prob -> taxon_prefix + walk.
#include "rtx_index.hpp"

#ifndef RTX_B2_HEAVY_PER_ATILE
#define RTX_B2_HEAVY_PER_ATILE 4u  // two-level bounds pass: a query whose rule asks for more B-tiles per A-tile (of 16) than this goes to the one-level pass (with lo = 0.36 t: 2 / 3 / 4: 80.9 / 79.2 / 78.8 ms per step at configs[2], 6.19 / 6.13 / 6.10 M queries/s at 5 % divergence; lo = 0.33 t and 3: 78.7 ms, 5.84 M)
#endif

namespace rtxi {

int bind(rtx_index *ix) {
    if (!ix) { set_error("null index handle"); return RTX_ERR_INVALID; }
    RTX_HIP(hipSetDevice(ix->device));
    return RTX_OK;
}

int ensure_events(rtx_index *ix, size_t count) {
    while (ix->events.size() < count) {
        hipEvent_t e;
        RTX_HIP(hipEventCreate(&e));
        ix->events.push_back(e);
    }
    return RTX_OK;
}


SubBatch sub_batch_of(rtx_index *ix, uint32_t sb, bool timed) {
    const rtx_index::SubPlan &p = ix->plan[sb];  // the plan of the run (plan_sub_batches): classes of different sub-batch sizes follow one another
    SubBatch b;
    b.sb = sb;
    b.q0 = p.q0;
    b.nq = p.nq;
    b.cls = &ix->cls[p.cls];
    b.set = ix->staged ? (sb & 1u) : 0u;
    b.s = ix->stream;
    b.timed = timed;
    b.timed_all = timed && ix->stage_timing != 0;
    return b;
}

// The sub-batches of the run, class after class (positions of the processing order: the class leads the sort key, order_batch).
int plan_sub_batches(rtx_index *ix) {
    ix->plan.clear();
    uint64_t pos = 0;
    for (uint32_t c = 0; c < ix->n_cls; c++) {  // positions: the classes in the order of their sort rank
        ix->cls[c].pos0 = pos;
        pos += ix->cls[c].n;
    }
    if (pos != ix->n_q) { set_error("internal: the length classes hold %llu of %llu queries", (unsigned long long)pos, (unsigned long long)ix->n_q); return RTX_ERR_STATE; }
    // execution: the side classes first (a few long reads: their slow, latency-bound back halves then run beside the front halves of the
    // bulk instead of behind everything), then the others -- the last sub-batch of a run, the one the taps read, belongs to the bulk
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t c = 0; c < ix->n_cls; c++) {
            rtx_index::BatchClass &k = ix->cls[c];
            if (k.side != (pass == 0)) continue;
            k.sb0 = ix->n_sub_total();
            for (uint64_t a = 0; a < k.n; a += k.sub_batch) ix->plan.push_back({k.pos0 + a, (uint32_t)std::min<uint64_t>(k.sub_batch, k.n - a), c});
            k.n_sub = ix->n_sub_total() - k.sb0;
        }
    return RTX_OK;
}

// Counts of a sub-batch between hit_count and taxon_prefix.  With 10 bit planes (t <= 1023) they travel packed,
// 10 bits per reference: [B][npad] low bytes, then [B][npad / 8] u16 with the two high bits of eight references
// each; otherwise [B][npad] u16.  Both live in the same allocation (sized for the format in use).
// Rows: one per query of the sub-batch -- or, behind tile pruning with the records path (BatchClass::diet), sub_batch >> diet_shift rows that
// prune_kernel hands to the queries that take the dense epilogues (HitParams::cnt_row): at configs[2] 83 of the 125 GB of two scratch sets were
// counts that 99 % of the queries never wrote.  The recounting taps (rtx_api_debug.hip) count a sub-batch in full: a row per query again.
constexpr uint32_t kDietMinRows = 1024;
uint32_t diet_rows(const rtx_index *ix, uint32_t B) { return std::min<uint32_t>(B, std::max<uint32_t>(kDietMinRows, B >> ix->diet_shift)); }
uint32_t counts_rows_layout(const rtx_index *ix, const rtx_index::BatchClass &k) { return k.diet && !ix->dbg_full_run && !ix->dbg_full ? k.cnt_rows : k.sub_batch; }
uint8_t *counts_lo(rtx_index *ix, rtx_index::Scratch &sc) { return reinterpret_cast<uint8_t *>(sc.d_counts.p); }
uint16_t *counts_hi(rtx_index *ix, const rtx_index::BatchClass &k, rtx_index::Scratch &sc) {
    return reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(sc.d_counts.p) + (size_t)counts_rows_layout(ix, k) * ix->npad);
}
int ensure_full_counts(rtx_index *ix, const rtx_index::BatchClass &k, rtx_index::Scratch &sc) { return sc.d_counts.alloc(counts_elems(ix, k.planes, k.sub_batch)); }

hipEvent_t stage_event(rtx_index *ix, const SubBatch &b, int stage, int which) {
    return ix->events[((size_t)b.sb * RTX_NUM_STAGES + stage) * 2 + which];
}

// group 1: kmer_extract + hit_count -> counts, per-shard histogram
static KmerParams kmer_params(rtx_index *ix, const SubBatch &b) {
    rtx_index::Scratch &sc = ix->sc[b.set];
    rtx_index::ResultSet &r = ix->res();
    const rtx_index::BatchClass &k = *b.cls;
    KmerParams kp{};
    kp.bases = ix->d_bases.p;
    kp.base_off = ix->in[ix->cur_in].d_base_off.p;
    kp.q0 = b.q0;
    kp.perm = r.d_perm.p;
    kp.row_of = ix->d_row_of.p;
    kp.list_len = ix->d_list_len.p;
    kp.row_len = ix->d_row_len.p;
    kp.zero_row = ix->n_rows;
    kp.kmers = sc.d_kmers.p;
    kp.kstride = k.kstride;
    kp.seginfo = ix->d_seginfo.p;
    kp.seg_stride = ix->seg_stride;
    kp.segcls = ix->d_segcls.p;
    kp.cls_stride = ix->cls_stride;
    kp.ntiles = ix->ntiles;
    kp.seg_dbits = ix->d_seg_dbits.p;
    kp.seg_sbits = ix->d_seg_sbits.p;
    kp.seg_sbase = ix->d_seg_sbase.p;
    kp.seg_blocks = ix->seg_blocks;
    kp.rows = sc.d_rows.p;
    kp.rstride = k.rstride;
    kp.dmask = sc.d_dmask.p;
    kp.srows = sc.d_srows.p;
    kp.nsparse = sc.d_nsparse.p;
    kp.t = sc.d_t.p;
    kp.nrows = sc.d_nrows.p;
    kp.hq = r.d_hq.p;
    kp.t_all = r.d_t_all.p;
    kp.nrows_all = r.d_nrows_all.p;
    kp.hist = sc.d_hist.p;  // zeroed by kmer_extract for hit_count's global atomics
    kp.hstride = k.hstride;
    return kp;
}

// What a sub-batch of class k being enqueued goes through, decided once.  It prunes (the recount of the debug taps leaves the pruning out):
static bool run_prunes(const rtx_index *ix, const rtx_index::BatchClass &k) { return k.prune && !ix->dbg_full_run; }
// ... its queries may take the records path (whole-database handles whose walk rides in the prefix launch: enqueue_prob_prefix starts
// records_tail_kernel there).  BatchClass::rec implies a whole-database handle driven by enqueue_batch, which enqueues part 0 and fuses the walk;
// the two callers still ask for that themselves, so that an rtx_shard_* call on such a handle stays off the path.
static bool on_records_path(const rtx_index *ix, const rtx_index::BatchClass &k, const rtx_index::Scratch &sc) { return run_prunes(ix, k) && k.rec && sc.d_rec.p != nullptr; }
// ... and the rows of its counts buffer are handed out with the decision about the records path (the diet)
static bool on_diet(const rtx_index *ix, const rtx_index::BatchClass &k, const rtx_index::Scratch &sc) { return on_records_path(ix, k, sc) && k.diet && sc.d_cnt_row.p != nullptr; }

static RecordRef record_ref(const rtx_index *ix, const rtx_index::Scratch &sc, const rtx_index::ResultSet &r) { return RecordRef{sc.d_rec_nslots.p, sc.d_rec_slots.p, sc.d_rec_cnt.p, sc.d_rec.p, ix->rec_slots(), ix->rec_seg_len, r.d_flags.p}; }
static ProbTables prob_tables(const rtx_index *ix) { return ProbTables{ix->d_tab_cmf.p, ix->d_tab_ratio.p, ix->d_tab_off.p, ix->d_tab_moff.p, ix->d_tab_ilo.p, ix->d_tab_sat.p, ix->tab_tmax}; }

int enqueue_kmer(rtx_index *ix, const SubBatch &b, hipStream_t s) {
    KmerParams kp = kmer_params(ix, b);
    // with tile pruning the per-tile lists wait until the live tiles are known (enqueue_hit); databases of few tiles build
    // their lists in one pass per tile whatever is live
    kp.mode = run_prunes(ix, *b.cls) && ix->seg_blocks ? 1u : 0u;
    if (run_prunes(ix, *b.cls)) {  // the counters enqueue_hit's kernels add to, zeroed here instead of by fill launches on its critical chain (ItemList)
        rtx_index::Scratch &sc = ix->sc[b.set];
        const ItemsLayout items(b.nq, ix->ntiles);
        const FineItemsLayout fine(b.nq, ix->f_ntiles);
        if (sc.d_items.p) { kp.zero[0] = items.count(sc.d_items.p); kp.zero_n[0] = 9u; }
        if (sc.d_fine_items.p) { kp.zero[1] = fine.count(sc.d_fine_items.p); kp.zero_n[1] = 9u + ix->f_ntiles; }  // header | cursors
        if (sc.d_cnt_cursor.p) { kp.zero[2] = sc.d_cnt_cursor.p; kp.zero_n[2] = 1u; }
    }
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_KMER_EXTRACT, 0), s));
    launch_kmer_extract(s, kp, b.nq);
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_KMER_EXTRACT, 1), s));
    return RTX_OK;
}

// the counting pass proper; what tile pruning adds (live masks, items, thresholds, records, rows of the diet) is filled in by enqueue_hit
static HitParams hit_params(rtx_index *ix, const SubBatch &b, uint32_t flags) {
    rtx_index::Scratch &sc = ix->sc[b.set];
    rtx_index::ResultSet &r = ix->res();
    const rtx_index::BatchClass &k = *b.cls;
    HitParams hp{};
    hp.bitmap = ix->d_bitmap.p;
    hp.stride_bytes = ix->stride_bytes;
    hp.n_rows1 = ix->n_rows + 1;
    hp.n_refs = ix->n_refs;
    hp.ref_base = ix->ref_lo;
    hp.rows = sc.d_rows.p;
    hp.rstride = k.rstride;
    hp.dmask = sc.d_dmask.p;
    hp.nrows = sc.d_nrows.p;
    hp.zero_row = ix->n_rows;
    hp.srows = sc.d_srows.p;
    hp.nsparse = sc.d_nsparse.p;
    hp.segslots = ix->d_segslots.p;
    hp.ntiles = ix->ntiles;
    hp.t = sc.d_t.p;
    hp.counts = sc.d_counts.p;
    hp.counts_lo = ix->packs(k.planes) ? counts_lo(ix, sc) : nullptr;  // null: u16 counts
    hp.counts_hi = ix->packs(k.planes) ? counts_hi(ix, k, sc) : nullptr;
    hp.npad = ix->npad;
    hp.hist = sc.d_hist.p;
    hp.hstride = k.hstride;
    hp.tile_max = sc.d_tilemax.p;
    hp.flags = flags;
    hp.q0 = b.q0;
    hp.perm = r.d_perm.p;
    hp.exact = ExactRef{ix->in[ix->cur_in].d_exact_ids.p, ix->in[ix->cur_in].d_exact_off.p, r.dev_exact ? r.d_exact_grp.p : nullptr, ix->d_em_goff.p, ix->d_em_gids.p};
    hp.nq = b.nq;
    hp.group_rows = k.pair ? ix->d_group_rows.p : nullptr;
    hp.group_base = b.sb * ix->groups_per_sub;
    hp.pair_urec = sc.d_urec.p;
    hp.pair_nu = sc.d_nu.p;
    hp.pair_ustride = 2u * k.rstride;
    return hp;
}

// (1) the queries against the union bitmap: every row dense, no lists, packed counts (bounds per block of references)
static HitParams bounds_params(const rtx_index *ix, const rtx_index::Scratch &sc, const HitParams &hp) {
    HitParams up = hp;
    up.bitmap = ix->d_ubitmap.p;
    up.stride_bytes = ix->u_stride_bytes;
    up.n_refs = ix->u_nblocks;
    up.dmask = nullptr;    // (a union bitmap is read densely: the kernel takes every row of the query, no masks, no sparse lists)
    up.nsparse = nullptr;
    up.ntiles = ix->u_ntiles;
    up.counts = nullptr;  // nothing is stored per block: the epilogue keeps the largest bound per tile and the best block
    up.counts_lo = nullptr;
    up.counts_hi = nullptr;
    up.hist = nullptr;
    up.tile_max = nullptr;
    up.bounds_tile_ub = sc.d_tile_ub.p;
    up.bounds_tile_stride = ix->ntiles;
    up.bounds_ntiles = ix->ntiles;
    up.bounds_best = sc.d_best_key.p;
    up.flags = 0;
    up.group_base = hp.group_base + ix->n_groups_run;  // work accounting apart from the counting proper
    return up;
}

// ... in two levels (rtx_bounds2.hip); heavy: the set has room for the queries and items left to the one-level pass
static Bounds2Params bounds2_params(const rtx_index *ix, const rtx_index::Scratch &sc, const HitParams &up, bool heavy) {
    Bounds2Params bp{};
    bp.abitmap = ix->d_abitmap.p;
    bp.bbitmap = ix->d_bbitmap.p;
    bp.n_rows1 = ix->n_rows + 1;
    bp.n_atiles = ix->n_atiles;
    bp.ntiles = ix->ntiles;
    bp.zero_row = ix->n_rows;
    bp.pair_urec = sc.d_urec.p;
    bp.pair_nu = sc.d_nu.p;
    bp.pair_ustride = up.pair_ustride;
    bp.nq = up.nq;
    bp.t = sc.d_t.p;
    bp.tile_ub = sc.d_tile_ub.p;
    bp.tile_ub_stride = ix->ntiles;
    bp.best_key = sc.d_best_key.p;
    bp.delta_ct = ix->b2_delta[0];
    bp.delta_cm = ix->b2_delta[1];
    bp.delta_lo = ix->b2_delta[2];
    bp.delta_hi = ix->b2_delta[3];
    bp.group_rows = up.group_rows;
    bp.group_base = up.group_base;
    // queries whose rule asks for more than five B-tiles per A-tile go to the one-level pass (5 folds of level B ~ half of it)
    bp.heavy = heavy ? sc.d_heavy.p : nullptr;
    bp.heavy_max = std::max<uint32_t>(1u, std::min<uint32_t>(RTX_B2_HEAVY_PER_ATILE * ix->n_atiles, ix->n_btiles / 2u));
    return bp;
}

// (2) bounds per tile, a lower bound of the best hit, the threshold, the live tiles of every pair
static PruneParams prune_params(rtx_index *ix, const SubBatch &b, uint32_t flags, int part, const ExactRef &exact) {
    rtx_index::Scratch &sc = ix->sc[b.set];
    const rtx_index::BatchClass &k = *b.cls;
    PruneParams pr{};
    pr.tile_ub = sc.d_tile_ub.p;
    pr.best_key = sc.d_best_key.p;
    pr.tile_ub_stride = ix->ntiles;
    pr.ntiles = ix->ntiles;
    pr.nq = b.nq;
    pr.n_refs = ix->n_refs;
    pr.n_total = ix->n_total;
    pr.ref_base = ix->ref_lo;
    pr.phase = (uint32_t)part;
    pr.best = part ? sc.d_best.p : nullptr;
    pr.bitmap = ix->d_bitmap.p;
    pr.cbitmap = part == 0 && (ix->two_level_used || (k.planes > kBounds2MaxPlanes && ix->two_level_opt && ix->n_refs == ix->n_total)) ? reinterpret_cast<const uint2 *>(ix->d_cbitmap.p) : nullptr;  // (with the two-level pass: RTX_OPT_TWO_LEVEL_BOUNDS = 0 is the round-4 path whole)
    pr.n_rows1 = ix->n_rows + 1;
    pr.stride_bytes = ix->stride_bytes;
    pr.rows = sc.d_rows.p;
    pr.rstride = k.rstride;
    pr.nrows = sc.d_nrows.p;
    pr.t = sc.d_t.p;
    pr.flags = flags;
    pr.q0 = b.q0;
    pr.perm = ix->res().d_perm.p;
    pr.exact = exact;
    pr.lnfact = ix->d_lnfact.p;
    pr.inv = ix->d_inv.p;
    pr.nlf = std::min<uint32_t>(kLnFactLen, k.tmax + k.tmax / 2 + 2);  // (pruning runs with tmax <= 2047: 12 KB at t <= 1023, 25 KB at most)
    pr.hist = sc.d_hist.p;
    pr.hstride = k.hstride;
    pr.live = sc.d_live.p;
    pr.live_words = LiveLayout{ix->ntiles}.words();
    pr.pair_live = ItemsLayout(b.nq, ix->ntiles).pair_live(sc.d_items.p);
    pr.thr_out = sc.d_prune_thr.p;
    pr.i1_out = sc.d_prune_i1.p;
    pr.stats = ix->d_prune_stats.p;
    pr.detail = ix->debug_taps && ix->d_prune_detail.n >= (size_t)b.nq * kPruneDetailWords ? ix->d_prune_detail.p : nullptr;
    return pr;
}

// (2b) the pairs that are left many live tiles against the fine union bitmap (blocks of 8 references)
static HitParams fine_params(const rtx_index *ix, const rtx_index::Scratch &sc, const HitParams &hp) {
    HitParams fp = hp;
    fp.bitmap = ix->d_fbitmap.p;
    fp.stride_bytes = ix->f_stride_bytes;
    fp.n_refs = ix->f_nblocks;
    fp.ntiles = ix->f_ntiles;
    fp.counts = nullptr;
    fp.counts_lo = nullptr;
    fp.counts_hi = nullptr;
    fp.tile_max = nullptr;
    fp.flags = 0;
    fp.group_rows = nullptr;  // (its rows are not part of the work accounting of the roofline: reported through its own counters)
    fp.live = sc.d_live.p;
    fp.live_words = LiveLayout{ix->ntiles}.words();
    fp.prune_thr = sc.d_prune_thr.p;
    fp.fine_n_refs = ix->n_refs;
    fp.fine_ref_ntiles = ix->ntiles;
    fp.fine_stats = ix->d_prune_stats.p + 2 * kPruneStatCopies * 8;
    return fp;
}

// part 0: everything.  A reference shard that prunes stops in the middle for the exchange of the best blocks: part 1 = up to the
// candidates (bounds pass, prune_kernel phase 1), part 2 = the rest (prune_kernel phase 2, lists of the live tiles, counting).
int enqueue_hit(rtx_index *ix, const SubBatch &b, uint32_t flags, hipStream_t s, int part, hipStream_t s_mid) {
    rtx_index::Scratch &sc = ix->sc[b.set];
    rtx_index::ResultSet &r = ix->res();
    const rtx_index::BatchClass &k = *b.cls;
    ix->last_set = b.set;
    HitParams hp = hit_params(ix, b, flags);
    const bool prune = run_prunes(ix, k);
    if (k.pair && part != 2) {
        if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_PAIR_UNION, 0), s));
        launch_pair_union(s, sc.d_rows.p, sc.d_nrows.p, k.rstride, b.nq, sc.d_urec.p, sc.d_nu.p, 2u * k.rstride);
        if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_PAIR_UNION, 1), s));
    }
    if (b.timed && !prune) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_HIT_COUNT, 0), s));
    if (part != 0 && !prune) { set_error("internal: a split run without tile pruning"); return RTX_ERR_STATE; }
    if (prune) {
        if (part != 2) {  // (1) bounds
            const HitParams up = bounds_params(ix, sc, hp);
            if (b.timed) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TILE_BOUNDS, 0), s));
            // whole-database handles: the two-level pass (rtx_bounds2.hip); reference shards and RTX_OPT_TWO_LEVEL_BOUNDS = 0: blocks of 64 throughout
            ix->two_level_used = part == 0 && ix->two_level_opt && ix->d_abitmap.p && ix->d_bbitmap.p && ix->n_refs == ix->n_total && k.planes <= kBounds2MaxPlanes;
            if (ix->two_level_used) {
                const bool heavy_ok = sc.d_heavy.p && sc.d_heavy_items.p && sc.d_heavy_items.n >= HeavyItemsLayout(b.nq, ix->u_ntiles).total();
                launch_bounds2(s, bounds2_params(ix, sc, up, heavy_ok), b.nq, k.planes, up, ix->u_ntiles, heavy_ok ? sc.d_heavy_items.p : nullptr);
            } else {
                RTX_HIP(hipMemsetAsync(sc.d_best_key.p, 0, (size_t)b.nq * 4, s));  // the waves of a query's union tiles meet in an atomicMax
                launch_hit_count_pair_bounds(s, up, b.nq, ix->u_ntiles, k.planes);  // the union of the pair's rows serves both passes
            }
            if (b.timed) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TILE_BOUNDS, 1), s));
        }
        if (s_mid && s_mid != s && part == 0) {  // RTX_OPT_OVERLAP = 2: threshold, lists and counting go on on a stream of their own
            RTX_HIP(hipEventRecord(ix->ev_mid[b.sb], s));
            RTX_HIP(hipStreamWaitEvent(s_mid, ix->ev_mid[b.sb], 0));
            s = s_mid;
        }
        if (b.timed && part != 1) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TILE_PRUNE, 0), s));
        // (2) threshold
        PruneParams pr = prune_params(ix, b, flags, part, hp.exact);
        const bool records = part == 0 && on_records_path(ix, k, sc), diet = part == 0 && on_diet(ix, k, sc);
        const RecordRef rr = record_ref(ix, sc, r);
        if (records) { pr.rec = rr; pr.rec_max_slots = rr.stride; }
        if (k.diet && !diet) { set_error("internal: the counts buffer is on its diet without the records path"); return RTX_ERR_STATE; }
        if (diet) {
            pr.cnt_row = sc.d_cnt_row.p;
            pr.cnt_cursor = sc.d_cnt_cursor.p;  // (zero since this sub-batch's kmer_extract: enqueue_kmer)
            pr.cnt_cap = k.cnt_rows;
            pr.dense_q = sc.d_dense_q.p;
            pr.flags_out = r.d_flags.p;
            hp.cnt_row = sc.d_cnt_row.p;
        }
        launch_prune(s, pr, prob_tables(ix), b.nq);
        if (part == 1) { RTX_HIP(hipGetLastError()); return RTX_OK; }  // the caller exchanges RTX_BUF_BEST, then part 2
        // (2b) second stage of the bounds (whole-database handles with a fine union bitmap): the pairs that are left many live tiles are
        // counted against the union bitmap over blocks of 8 references, which takes the tiles without a block above the threshold off
        // their lists (fine_epilogue); the list below is built from the masks as this pass leaves them
        if (part == 0 && ix->fine_opt && ix->d_fbitmap.p && k.pair && sc.d_fine_items.p) {
            const FineItemsLayout fine(b.nq, ix->f_ntiles);
            uint32_t *const fi = sc.d_fine_items.p;
            launch_fine_bounds(s, fine_params(ix, sc, hp), b.nq, ix->f_ntiles, pr.pair_live, fine.cursors(fi), fine.items(fi), fine.count(fi), k.planes);
        }
        // (3) tiles that are not counted keep a largest count of 0: taxon_prefix leaves them out
        RTX_HIP(hipMemsetAsync(sc.d_tilemax.p, 0, (size_t)b.nq * ix->ntiles * 2, s));
        hp.live = sc.d_live.p;
        hp.live_words = pr.live_words;
        hp.prune_thr = sc.d_prune_thr.p;
        if (records) hp.rec = rr;
        if (k.pair) {  // the grid of the counting pass walks the live (pair, tile) blocks instead of all of them
            const ItemsLayout items(b.nq, ix->ntiles);
            launch_live_items(s, sc.d_live.p, pr.live_words, b.nq, ix->ntiles, items.items(sc.d_items.p), items.count(sc.d_items.p),
                              ix->d_prune_stats.p ? ix->d_prune_stats.p + 2 * kPruneStatCopies * 8 : nullptr);
            hp.items = items.items(sc.d_items.p);
            hp.n_items = items.count(sc.d_items.p);
        }
        if (ix->seg_blocks) {  // (4) the row lists of the live tiles (kmer_extract left them out)
            KmerParams kp = kmer_params(ix, b);
            kp.mode = 2u;
            kp.live = sc.d_live.p;
            kp.live_words = pr.live_words;
            launch_kmer_extract(s, kp, b.nq);
        }
        if (b.timed) {
            RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TILE_PRUNE, 1), s));
            RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_HIT_COUNT, 0), s));
        }
    }
    if (k.pair) launch_hit_count_pair(s, hp, b.nq, ix->ntiles, k.planes);
    else launch_hit_count(s, hp, b.nq, ix->ntiles, k.planes);
    if (b.timed) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_HIT_COUNT, 1), s));
    ix->hit_stream = s;
    return RTX_OK;
}

int enqueue_count(rtx_index *ix, const SubBatch &b, uint32_t flags, hipStream_t s_mid) {
    int rc = enqueue_kmer(ix, b, b.s);
    return rc ? rc : enqueue_hit(ix, b, flags, b.s, 0, s_mid);
}

static WalkParams walk_params(rtx_index *ix, const SubBatch &b, const double *prefix);
static int reset_sub_alloc(rtx_index *ix, hipStream_t s);

// group 2: prob table from the (whole-database) histogram + prefix sums over this handle's references; with
// fuse_walk (whole database on this handle) the taxonomy walk of group 3 runs inside the prefix kernel
int enqueue_prob_prefix(rtx_index *ix, const SubBatch &b, bool fuse_walk, bool prob_only) {
    rtx_index::Scratch &sc = ix->sc[b.set];
    const rtx_index::BatchClass &k = *b.cls;
    hipStream_t s = b.s;
    ProbParams pp{};
    pp.t = sc.d_t.p;
    pp.hist = sc.d_hist.p;
    pp.hstride = k.hstride;
    pp.tmax = k.tmax;
    pp.n1max = k.tmax / 2 + 1;
    pp.lnfact = ix->d_lnfact.p;
    pp.n_refs = ix->n_total;
    pp.q0 = b.q0;
    pp.table_z = sc.d_table_z.p;
    rtx_index::ResultSet &r = ix->res();
    pp.z = r.d_z.p;
    pp.gs = r.d_gs.p;
    pp.status = r.d_status.p;
    pp.ndist = r.d_ndist.p;
    pp.prune_thr = run_prunes(ix, k) ? sc.d_prune_thr.p : nullptr;
    pp.prune_i1 = pp.prune_thr ? sc.d_prune_i1.p : nullptr;
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_PROB_TABLE, 0), s));
    if (k.use_tables) {
        launch_prob_order(s, sc.d_t.p, b.nq, sc.d_order.p);
        pp.order = sc.d_order.p;
        launch_prob_lookup(s, pp, prob_tables(ix), b.nq);
    } else {
        if (k.huge) {  // its arrays do not fit LDS: a stretch of global memory per query
            pp.gstride = (uint32_t)((prob_table_lds_bytes(k.tmax) + 7) / 8);
            if (ix->d_prob_scratch.n < (size_t)b.nq * pp.gstride) { set_error("internal: scratch of prob_table too small"); return RTX_ERR_STATE; }
            pp.gscratch = ix->d_prob_scratch.p;
        }
        launch_prob_table(s, pp, b.nq);
    }
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_PROB_TABLE, 1), s));
    if (prob_only) return RTX_OK;  // debug taps after a pruned run: counts and table again, the result rows stay

    PrefixParams fp{};
    fp.status = r.d_status.p;
    fp.t = sc.d_t.p;
    fp.tz_in_lds = (size_t)k.hstride * 8 <= 16 * 1024 ? 1u : 0u;
    fp.q0 = b.q0;
    fp.counts = sc.d_counts.p;
    fp.counts_lo = counts_lo(ix, sc);
    fp.counts_hi = counts_hi(ix, k, sc);
    fp.packed = ix->packs(k.planes) ? 1u : 0u;
    fp.npad = ix->npad;
    fp.table_z = sc.d_table_z.p;
    fp.hstride = k.hstride;
    fp.n_refs = ix->n_refs;
    fp.bnd_bits = ix->d_bnd_bits.p;
    fp.bnd_rank = ix->d_bnd_rank.p;
    fp.prefix = sc.d_prefix.p;
    fp.n_bnd = ix->n_bnd_local;
    fp.tile_max = ix->tile_skip ? sc.d_tilemax.p : nullptr;
    fp.ntiles = ix->ntiles;
    fp.prune_thr = pp.prune_thr;
    fp.prune_stats = fp.prune_thr ? ix->d_prune_stats.p + kPruneStatCopies * 8 : nullptr;
    fp.fuse_walk = fuse_walk ? 1u : 0u;
    const bool records = fuse_walk && on_records_path(ix, k, sc);
    fp.rec_nslots = records ? sc.d_rec_nslots.p : nullptr;
    fp.cnt_row = fuse_walk && on_diet(ix, k, sc) ? sc.d_cnt_row.p : nullptr;
    if (fp.cnt_row) {  // the launch is over the rows prune_kernel handed out, not over the queries (PrefixParams::dense_q)
        fp.dense_q = sc.d_dense_q.p;
        fp.cnt_cursor = sc.d_cnt_cursor.p;
        fp.cnt_cap = k.cnt_rows;
        fp.nq = b.nq;
    }
    if (fuse_walk) {
        fp.walk = walk_params(ix, b, sc.d_prefix.p);
        int rc_r = fp.walk.sub_alloc ? reset_sub_alloc(ix, s) : RTX_OK;
        if (rc_r) return rc_r;
    }
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TAXON_PREFIX, 0), s));
    launch_taxon_prefix(s, fp, b.nq);
    if (records) {  // the queries on the records path: prefix sums from their records, the walk from LDS (rtx_records.hip)
        TailParams tp{};
        tp.rec = record_ref(ix, sc, r);
        tp.t = sc.d_t.p;
        tp.table_z = sc.d_table_z.p;
        tp.hstride = k.hstride;
        tp.bnd_bits = ix->d_bnd_bits.p;
        tp.bnd_rank = ix->d_bnd_rank.p;
        tp.prefix = sc.d_prefix.p;
        if (fp.cnt_row) { tp.cnt_cursor = sc.d_cnt_cursor.p; tp.cnt_cap = k.cnt_rows; tp.flags_out = r.d_flags.p; }
        tp.n_bnd = ix->n_bnd_local;
        tp.nq = b.nq;
        tp.walk = fp.walk;
        tp.prefix_stats = fp.prune_stats;
        tp.stats = ix->d_prune_stats.p ? ix->d_prune_stats.p + 3 * kPruneStatCopies * 8 : nullptr;
        launch_records_tail(s, tp, b.nq);
    }
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_TAXON_PREFIX, 1), s));
    return RTX_OK;
}

// The per-query arrays, the cursors, the arena (at least min_arena rows) and the final arrays of a set, for a batch of n_queries
int alloc_result_set(rtx_index *ix, rtx_index::ResultSet &r, uint64_t n_queries, uint64_t min_arena) {
    int rc;
    if ((rc = r.d_status.alloc(n_queries)) || (rc = r.d_t_all.alloc(n_queries)) || (rc = r.d_nrows_all.alloc(n_queries)) ||
        (rc = r.d_n_rows.alloc(n_queries)) || (rc = r.d_gs.alloc(n_queries)) || (rc = r.d_z.alloc(n_queries)) ||
        (rc = r.d_hq.alloc(n_queries)) || (rc = r.d_row_start.alloc(n_queries)) || (rc = r.d_ndist.alloc(n_queries)) ||
        (rc = r.d_cursor.alloc(2)) || (rc = r.d_flags.alloc(1)))
        return rc;
    // eight rows per query + two for what the sub-allocators leave unused (walk_params)
    const uint64_t want_arena = std::max<uint64_t>(n_queries * 10 + 4096, min_arena);
    if (r.arena_cap < want_arena) {
        if ((rc = r.d_arena.alloc(want_arena))) return rc;
        r.arena_cap = want_arena;
    }
    return alloc_final(ix, r, n_queries);
}

// A run that may be followed by a run-ahead (RTX_OPT_RUN_AHEAD) leaves out the wait of the handle's stream for the stream of its back
// halves; whoever needs the handle's stream to cover the whole run asks for it here.
int settle_join(rtx_index *ix) {
    if (ix->join_pending && ix->join_ev) RTX_HIP(hipStreamWaitEvent(ix->stream, ix->join_ev, 0));
    ix->join_pending = false;
    return RTX_OK;
}

// The final result arrays (finalise_kernel): the per-query fields of the batch in input order, as many rows as the arena holds
int alloc_final(rtx_index *ix, rtx_index::ResultSet &r, uint64_t n_queries) {
    int rc;
    if ((rc = r.d_fin_t.alloc(n_queries)) || (rc = r.d_fin_status.alloc(n_queries)) || (rc = r.d_fin_gs.alloc(n_queries)) ||
        (rc = r.d_fin_row_begin.alloc(n_queries)) || (rc = r.d_fin_row_count.alloc(n_queries)) || (rc = r.d_fin_cursor.alloc(2)))
        return rc;
    if ((rc = r.d_peak2.alloc(n_queries)) || (rc = r.d_peak.alloc(n_queries)) || (rc = r.d_strand.alloc(n_queries))) return rc;  // (rtx_strand.hip)
    if (ix->nearest_opt && ((rc = r.d_nearest2.alloc(n_queries)) || (rc = r.d_ties2.alloc(n_queries)) || (rc = r.d_nearest.alloc(n_queries)) || (rc = r.d_ties.alloc(n_queries))))  // (rtx_nearest.hip)
        return rc;
    if (ix->identity_opt && ((rc = r.d_dist.alloc(n_queries)) || (rc = r.d_qlen.alloc(n_queries)))) return rc;  // (rtx_identity.hip)
    if (ix->strand_opt && ((rc = r.d_sel_t.alloc(n_queries)) || (rc = r.d_sel_status.alloc(n_queries)) || (rc = r.d_sel_gs.alloc(n_queries)) ||
                           (rc = r.d_sel_row_begin.alloc(n_queries)) || (rc = r.d_sel_row_count.alloc(n_queries))))
        return rc;
    const uint64_t rows = r.arena_cap, D = ix->fin_D;
    if ((rc = r.d_fin_lineage.alloc(rows)) || (rc = r.d_fin_node.alloc(rows)) || (rc = r.d_fin_depth.alloc(rows)) || (rc = r.d_fin_depth8.alloc(rows)) ||
        (rc = r.d_fin_local.alloc(rows)) || (rc = r.d_fin_conf.alloc(rows * D)) || (rc = r.d_fin_hund.alloc(rows * D)))
        return rc;
    r.fin_cap = rows;
    return RTX_OK;
}

// Behind the walks of a sub-batch: its rows sorted, finished and laid out for the host's view (rtx_finalise.hip).  The launches of a run
// follow one another (the bulk's on the stream of the back halves, the side classes' behind the join: enqueue_batch), so the rows of a
// sub-batch are [cursor before its launch, cursor behind it) -- h_fin_sub keeps the latter for the streamed download.
int enqueue_finalise(rtx_index *ix, const SubBatch &b, hipStream_t s) {
    rtx_index::ResultSet &r = ix->res();
    FinaliseParams fp{};
    fp.status = r.d_status.p;
    fp.t_all = r.d_t_all.p;
    fp.gs = r.d_gs.p;
    fp.n_rows = r.d_n_rows.p;
    fp.row_start = r.d_row_start.p;
    fp.arena = r.d_arena.p;
    fp.arena_cap = r.arena_cap;
    fp.perm = r.d_perm.p;
    fp.q0 = b.q0;
    fp.nq = b.nq;
    fp.node_depth = ix->d_node_depth.p;
    fp.node_sig0 = ix->d_node_sig0.p;
    fp.node_begin = ix->d_node_begin.p;
    fp.node_eb = ix->d_node_eb.p;
    fp.D = ix->fin_D;
    fp.o_t = r.d_fin_t.p;
    fp.o_status = r.d_fin_status.p;
    fp.o_gs = r.d_fin_gs.p;
    fp.o_row_begin = r.d_fin_row_begin.p;
    fp.o_row_count = r.d_fin_row_count.p;
    fp.r_lineage = r.d_fin_lineage.p;
    fp.r_node = r.d_fin_node.p;
    fp.r_depth = r.d_fin_depth.p;
    fp.r_depth8 = r.d_fin_depth8.p;
    fp.r_hund = r.d_fin_hund.p;
    fp.r_local = r.d_fin_local.p;
    fp.r_conf = r.d_fin_conf.p;
    fp.row_cap = r.fin_cap;
    fp.fin_cursor = r.d_fin_cursor.p;
    fp.flags_out = r.d_flags.p;
    launch_finalise(s, fp);
    if (r.stream_dl && b.sb < r.h_fin_sub.size())
        RTX_HIP(hipMemcpyAsync(&r.h_fin_sub[b.sb], r.d_fin_cursor.p, 8, hipMemcpyDeviceToHost, s));
    return RTX_OK;
}

// group 3: taxonomy walk over prefix sums covering the WHOLE database ([nq][n_bnd], device)
static WalkParams walk_params(rtx_index *ix, const SubBatch &b, const double *prefix) {
    rtx_index::ResultSet &r = ix->res();
    WalkParams wp{};
    wp.status = r.d_status.p;
    wp.q0 = b.q0;
    wp.prefix = prefix;
    wp.n_bnd = ix->n_bnd;
    wp.rec = ix->d_noderec.p;
    wp.arena = r.d_arena.p;
    const bool side = b.cls->side;  // its rows go to the top of the arena through a cursor of their own
    wp.arena_cap = side ? r.arena_cap : r.side_base;
    wp.arena_cursor = r.d_cursor.p + (side ? 1 : 0);
    // (launches of a few thousand walks do not contend, and the rows the sub-allocators leave unused must stay within the arena's
    // allowance of two rows per query: at most kWalkSubAllocs * kWalkChunkRows = 8192 per launch of kWalkSubMinQueries or more)
    wp.sub_alloc = !side && b.nq >= kWalkSubMinQueries && r.arena_cap < (1ull << 32) ? ix->d_sub_alloc.p : nullptr;
    wp.n_rows = r.d_n_rows.p;
    wp.row_start = r.d_row_start.p;
    wp.flags_out = r.d_flags.p;
    return wp;
}
// the sub-allocators of the result arena start empty in every launch that walks (WalkParams::sub_alloc)
static int reset_sub_alloc(rtx_index *ix, hipStream_t s) {
    if (ix->d_sub_alloc.p) RTX_HIP(hipMemsetAsync(ix->d_sub_alloc.p, 0, (size_t)kWalkSubAllocs * kWalkSubStride * 8, s));
    return RTX_OK;
}

int enqueue_walk(rtx_index *ix, const SubBatch &b, const double *prefix, hipStream_t s) {
    const WalkParams wp = walk_params(ix, b, prefix);
    int rc_r = wp.sub_alloc ? reset_sub_alloc(ix, s) : RTX_OK;
    if (rc_r) return rc_r;
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_LINEAGE_WALK, 0), s));
    launch_lineage_walk(s, wp, b.nq);
    if (b.timed_all) RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_LINEAGE_WALK, 1), s));
    return RTX_OK;
}

// Processing order of the uploaded batch: related queries next to each other (rtx_cluster.hip), or input order.
int order_batch(rtx_index *ix, bool cluster) {
    const uint32_t n = (uint32_t)ix->n_q;
    rtx_index::ResultSet &r = ix->res();
    int rc;
    if ((rc = r.d_perm.alloc(n)) || (rc = r.d_iperm.alloc(n))) return rc;
    const bool multi = ix->n_cls > 1;       // several length classes: the class leads the key, whatever orders the queries inside a class
    const bool sketch = cluster && n > 2;
    if (sketch || multi) {
        if ((rc = ix->d_skey_in.alloc(n)) || (rc = ix->d_skey_out.alloc(n)) || (rc = ix->d_sidx.alloc(n))) return rc;
        size_t tmp = 0;
        if (cluster_sort(ix->stream, nullptr, &tmp, ix->d_skey_in.p, ix->d_skey_out.p, ix->d_sidx.p, r.d_perm.p, n, multi)) {
            set_error("radix sort: size query failed");
            return RTX_ERR_HIP;
        }
        if (ix->d_sort_tmp.n < tmp && (rc = ix->d_sort_tmp.alloc(tmp + 256))) return rc;
        if (sketch) {
            if (ix->d_loc_table.p && ix->locator_opt)  // (takes the min-hashes its key holds itself)
                launch_locator(ix->stream, ix->d_bases.p, ix->in[ix->cur_in].d_base_off.p, n, ix->d_loc_table.p, ix->n_total, ix->d_skey_in.p, ix->d_sidx.p);
            else
                launch_sketch(ix->stream, ix->d_bases.p, ix->in[ix->cur_in].d_base_off.p, n, ix->d_skey_in.p, ix->d_sidx.p);
        }
        if (multi) launch_class_keys(ix->stream, ix->d_skey_in.p, ix->in[ix->cur_in].d_base_off.p, n, ix->key_lim, !sketch, ix->d_sidx.p);
        tmp = ix->d_sort_tmp.n;
        if (cluster_sort(ix->stream, ix->d_sort_tmp.p, &tmp, ix->d_skey_in.p, ix->d_skey_out.p, ix->d_sidx.p, r.d_perm.p, n, multi)) {
            set_error("radix sort of the query sketches failed");
            return RTX_ERR_HIP;
        }
        launch_invert_perm(ix->stream, r.d_perm.p, n, r.d_iperm.p);
    } else {
        launch_identity_perm(ix->stream, n, r.d_perm.p, r.d_iperm.p);
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// What the download of the run being enqueued reads of its batch, into the result set the run writes (enqueue_batch adds stream_dl)
void record_batch(rtx_index *ix) {
    rtx_index::ResultSet &r = ix->res();
    r.n_q = ix->n_q;
    r.n_user = ix->strand_used ? ix->n_user : ix->n_q;
    r.has_peak = false;
    r.has_nearest = false;
    r.has_identity = false;
    r.profiled = false;
    r.n_sub = ix->n_sub_total();
    r.n_side = 0;
    for (uint32_t c = 0; c < ix->n_cls; c++)
        if (ix->cls[c].side) r.n_side += ix->cls[c].n_sub;  // (plan_sub_batches: their sub-batches come first)
    r.in_set = ix->cur_in;
    r.dev_exact = ix->dev_exact_used;
    r.stream_dl = false;
}

int begin_run(rtx_index *ix, uint32_t *n_sub_out, bool *timed_out, bool cluster) {
    int rc_p = plan_sub_batches(ix);
    if (rc_p) return rc_p;
    const uint32_t n_sub = ix->n_sub_total();
    record_batch(ix);
    rtx_index::ResultSet &r = ix->res();
    const bool timed = n_sub <= 4096;
    if (timed) {
        int rc = ensure_events(ix, (size_t)n_sub * RTX_NUM_STAGES * 2);
        if (rc) return rc;
    }
    const bool ev_all = timed && ix->stage_timing;
    if (ev_all) RTX_HIP(hipEventRecord(ix->events[(size_t)RTX_STAGE_ORDER * 2], ix->stream));  // sub-batch 0
    int rc_o = order_batch(ix, cluster);
    if (rc_o) return rc_o;
    if (ev_all) RTX_HIP(hipEventRecord(ix->events[(size_t)RTX_STAGE_ORDER * 2 + 1], ix->stream));
    {   // the result arena: the bulk's rows from 0 on, the side classes' (kWalkMaxRows per query at most) at its top
        uint64_t n_side_q = 0;
        for (uint32_t c = 0; c < ix->n_cls; c++)
            if (ix->cls[c].side) n_side_q += ix->cls[c].n;
        const uint64_t side_rows = n_side_q ? n_side_q * kWalkMaxRows + 64 : 0;
        if (side_rows + ix->n_q * 2 + 1024 > r.arena_cap) {  // (size_workspace has made room; a sharded or debug run has no side class)
            int rc_a = r.d_arena.alloc(r.arena_cap + side_rows);
            if (rc_a) return rc_a;
            r.arena_cap += side_rows;
        }
        if (r.fin_cap < r.arena_cap || r.d_fin_t.n < ix->n_q) {
            int rc_f = alloc_final(ix, r, ix->n_q);
            if (rc_f) return rc_f;
        }
        r.side_base = r.arena_cap - side_rows;
        int rc_h = r.h_side_base.resize(2);
        if (rc_h) return rc_h;
        r.h_side_base[0] = 0;
        r.h_side_base[1] = r.side_base;
        RTX_HIP(hipMemcpyAsync(r.d_cursor.p, r.h_side_base.data(), 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, ix->stream));
    }
    RTX_HIP(hipMemsetAsync(r.d_flags.p, 0, sizeof(uint32_t), ix->stream));
    RTX_HIP(hipMemsetAsync(r.d_fin_cursor.p, 0, 2 * sizeof(unsigned long long), ix->stream));  // the final rows of this run start at 0
    // tile pruning: the pair kernel, the memoised tables (their ln cmf rows give the threshold), taxon_prefix skipping tiles by
    // their largest count, the whole database on this handle
    // a whole-database handle driven by rtx_batch_run, or a reference shard that was asked to (RTX_OPT_SHARD_PRUNE: the caller then
    // drives rtx_shard_bounds and exchanges the best blocks); never a k-mer shard (its counts are partial sums)
    const bool whole = ix->n_refs == ix->n_total && !ix->staged;
    const bool shard = ix->staged && ix->shard_prune_opt && ix->n_refs != ix->n_total;
    auto scratch_ok = [&](const rtx_index::Scratch &sc, uint32_t B) {  // sized at the upload / rtx_shard_begin (alloc_scratch_set) for this sub-batch size
        const ScratchNeed n = ScratchNeed().set_queries(ix, B);
        return sc.d_tile_ub.p != nullptr && sc.d_tile_ub.n >= n.tile_ub && sc.d_best_key.n >= n.best_key && sc.d_prune_thr.n >= n.prune_thr &&
               sc.d_live.n >= n.live && sc.d_best.n >= n.best && sc.d_items.n >= n.items;
    };
    bool any_pair = false, any_prune = false;
    uint32_t b_max = 1;
    for (uint32_t c = 0; c < ix->n_cls; c++) {  // what every class of the batch runs through
        rtx_index::BatchClass &k = ix->cls[c];
        // two neighbours per wave only pays when neighbours are related: with the processing order on
        k.pair = ix->pair_opt && cluster && k.planes <= 11 && ix->n_q > 1 && k.rstride <= 4096;
        const rtx_index::Scratch &s0 = ix->sc[k.side ? kSideSet : 0u];  // (a side class runs through the set of its own)
        ScratchNeed need = ScratchNeed().set_queries(ix, k.sub_batch);  // of a sub-batch of the class
        if (whole && ix->rec_opt != 0u && ix->pruning())  // (segments that have grown since the workspace was sized: RecordRef::seg_len)
            for (uint32_t j = 0; j < 4u; j++) {
                rtx_index::Scratch &sc = ix->sc[j];
                if ((j == kSideSet) != k.side || sc.d_kmers.p == nullptr || sc.d_rec.p == nullptr || sc.d_rec.n >= need.rec) continue;
                RTX_HIP(hipStreamSynchronize(ix->stream));
                if (sc.d_rec.alloc(need.rec)) sc.d_rec.release();
            }
        k.prune = ix->pruning() && k.pair && k.use_tables && ix->tile_skip && ix->d_ubitmap.p && (whole || shard) &&
                  scratch_ok(s0, k.sub_batch) && (!ix->staged || scratch_ok(ix->sc[1], k.sub_batch));
        k.rec = k.prune && whole && ix->rec_opt != 0u && ix->n_bnd_local == ix->n_bnd && s0.d_rec.p != nullptr && s0.d_rec.n >= need.rec;
        // the diet of the counts buffer: only with the records path (the queries without rows are exactly those on it), in every set the class may run through
        auto diet_ok = [&](const rtx_index::Scratch &sc) { return sc.d_rec.p != nullptr && sc.d_cnt_row.p != nullptr && sc.d_cnt_cursor.p != nullptr && sc.d_dense_q.p != nullptr && sc.d_cnt_row.n >= need.cnt_row; };
        k.diet = k.rec && diet_rows(ix, k.sub_batch) < k.sub_batch && diet_ok(s0);
        if (k.diet && !k.side)
            for (uint32_t j = 1; j <= 2u; j++)
                if (ix->sc[j].d_kmers.p != nullptr && !diet_ok(ix->sc[j])) k.diet = false;
        k.cnt_rows = k.diet ? diet_rows(ix, k.sub_batch) : k.sub_batch;
        {   // room for that many rows in the sets the class runs through (a class that was sized for the diet and runs without it, a diet that has grown)
            need.add_class(ix, k, k.sub_batch, k.cnt_rows);  // (the rows of the boundary prefix sums go with those of the counts)
            for (uint32_t j = 0; j < 4u; j++) {
                rtx_index::Scratch &sc = ix->sc[j];
                const bool list_ok = !k.diet || sc.d_dense_q.n >= need.dense_q;  // (the list of the rows' queries grows with the rows)
                if ((j == kSideSet) != k.side || sc.d_kmers.p == nullptr || (sc.d_counts.n >= need.counts && sc.d_prefix.n >= need.prefix && list_ok)) continue;
                RTX_HIP(hipStreamSynchronize(ix->stream));  // (nothing of an earlier run may still read the old buffers)
                int rc_c = sc.d_counts.alloc(need.counts);
                if (!rc_c) rc_c = sc.d_prefix.alloc(need.prefix);
                if (!rc_c && !list_ok) rc_c = sc.d_dense_q.alloc(need.dense_q);
                if (rc_c) return rc_c;
            }
        }
        any_pair = any_pair || k.pair;
        any_prune = any_prune || k.prune;
        b_max = std::max(b_max, k.sub_batch);
    }
    ix->sub_batch_max = b_max;
    ix->any_prune = any_prune;
    ix->groups_per_sub = (b_max + 1u) / 2u;
    ix->dbg_full = false;
    if (any_prune) {
        int rc_s = ix->d_prune_stats.alloc(kPruneStatCopies * 32);
        if (!rc_s && ix->debug_taps) rc_s = ix->d_prune_detail.alloc((size_t)b_max * kPruneDetailWords);
        if (rc_s) return rc_s;
        RTX_HIP(hipMemsetAsync(ix->d_prune_stats.p, 0, kPruneStatCopies * 256, ix->stream));
    }
    if (any_pair) {
        ix->n_groups_run = n_sub * ix->groups_per_sub;
        int rc_g = ix->d_group_rows.alloc((size_t)2 * n_sub * ix->groups_per_sub);  // second half: the bounds pass of the tile pruning
        if (rc_g) return rc_g;
        RTX_HIP(hipMemsetAsync(ix->d_group_rows.p, 0, (size_t)2 * n_sub * ix->groups_per_sub * 4, ix->stream));
    }
    ix->n_sub_last = timed ? n_sub : 0;
    ix->overlap_used = 0;  // scratch sets in use beside each other (RTX_OPT_OVERLAP)
    // (only behind tile pruning: where every tile is counted the counting pass lives on its rows staying in L2, and the sweeps of a back half
    // beside it cost more than they hide: 990 against 955 ms per 1 M queries at configs[2] with RTX_OPT_TILE_PRUNE = 0)
    if (ix->overlap_opt != 0u && whole && n_sub >= 2 && !ix->shared_device && any_prune && ix->sc[1].d_kmers.p != nullptr && scratch_ok(ix->sc[1], b_max) == scratch_ok(ix->sc[0], b_max)) {
        ix->overlap_used = 2;
        if (ix->overlap_opt >= 2u && n_sub >= 3 && ix->sc[2].d_kmers.p != nullptr && scratch_ok(ix->sc[2], b_max) == scratch_ok(ix->sc[0], b_max)) ix->overlap_used = 3;
    }
    if (r.dev_exact) {  // Tree.sequences.get for every query of the batch (raxtax.rs:42), part of the run
        ExactParams xp{ix->d_bases.p, ix->in[ix->cur_in].d_base_off.p, (uint32_t)ix->n_q, ix->d_em_table.p, ix->em_bits, ix->d_em_rep_off.p,
                       ix->d_em_rep_bytes.p, r.d_exact_grp.p, ix->em_hash_mask};
        const bool ev = timed && ix->stage_timing;
        if (ev) RTX_HIP(hipEventRecord(ix->events[(size_t)RTX_STAGE_EXACT_MATCH * 2], ix->stream));  // sub-batch 0
        launch_exact_match(ix->stream, xp);
        if (ev) RTX_HIP(hipEventRecord(ix->events[(size_t)RTX_STAGE_EXACT_MATCH * 2 + 1], ix->stream));
        if (!r.ev_exact) RTX_HIP(hipEventCreateWithFlags(&r.ev_exact, hipEventDisableTiming));
        RTX_HIP(hipEventRecord(r.ev_exact, ix->stream));
    }
    *n_sub_out = n_sub;
    *timed_out = timed;
    return RTX_OK;
}

// Enqueues every kernel of the uploaded batch (whole-database handle), sub-batch after sub-batch on the handle's stream.
// (Round 2 also offered side streams -- the two small latency-bound kernels, or prob/prefix/walk of sub-batch i, beside the
// counting of sub-batch i + 1: no gain on MI355X in any arrangement, hit_count holds every wave slot of the chip; DESIGN.md
// section 3.  Removed in round 3.)
int enqueue_batch(rtx_index *ix, uint32_t flags) {
    if (ix->n_refs != ix->n_total) {
        set_error("this handle holds a reference shard: drive it with rtx_shard_count/_prob/_walk");
        return RTX_ERR_STATE;
    }
    uint32_t n_sub = 0;
    bool timed = false;
    int rc;
    // (a run that left its join out, and no run-ahead in progress: the kernels of this run write what its back halves may still read)
    if (ix->join_pending && !ix->hold_join && (rc = settle_join(ix))) return rc;
    rc = begin_run(ix, &n_sub, &timed, ix->cluster != 0);
    if (rc) return rc;
    rtx_index::ResultSet &r = ix->res();
    ix->n_near_last = 0;
    r.has_nearest = ix->nearest_opt != 0u && r.d_nearest2.p != nullptr && r.d_nearest2.n >= r.n_q && r.d_nearest.n >= r.n_user;
    if (ix->nearest_opt != 0u && !r.has_nearest) { set_error("internal: RTX_OPT_NEAREST without its arrays"); return RTX_ERR_STATE; }
    ix->ident_timed = false;
    r.has_identity = ix->identity_opt != 0u && r.has_nearest && r.d_dist.p != nullptr && r.d_dist.n >= r.n_user && r.d_qlen.n >= r.n_user && ix->d_em_ref_grp.p != nullptr;
    if (ix->identity_opt != 0u && !r.has_identity) { set_error("internal: RTX_OPT_IDENTITY without its arrays"); return RTX_ERR_STATE; }
    if (n_sub <= 4096) {  // per sub-batch: completion event (+ cursor snapshots) for the streamed download
        if (!ix->copy_stream) RTX_HIP(hipStreamCreateWithFlags(&ix->copy_stream, hipStreamNonBlocking));
        while (r.ev_sub.size() < n_sub) {
            hipEvent_t e;
            RTX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            r.ev_sub.push_back(e);
        }
        if ((rc = r.h_cursor_sub.resize(n_sub)) || (rc = r.h_fin_sub.resize(n_sub))) return rc;
        r.stream_dl = true;
    }
    // the walk rides inside the prefix kernel (the stage time of lineage_walk is then part of taxon_prefix)
    const bool fuse = ix->n_bnd_local == ix->n_bnd;
    // RTX_OPT_OVERLAP: the back half of sub-batch k (prob_lookup, taxon_prefix / records tail: chains of dependent round trips) on a second
    // stream beside the front half of sub-batch k + 1 (bounds and counting: VALU and L1 rate); two scratch sets alternate (sb & 1), a
    // front half waits for the back half that last used its set.
    const uint32_t nsets = ix->overlap_used;  // 0: one stream; 2: two stages, two scratch sets; 3: front | threshold + counting | back
    const bool overlap = nsets != 0u;
    if (overlap) {
        if (!ix->stream2) RTX_HIP(hipStreamCreateWithFlags(&ix->stream2, hipStreamNonBlocking));
        if (nsets == 3u && !ix->stream3) RTX_HIP(hipStreamCreateWithFlags(&ix->stream3, hipStreamNonBlocking));
        while (ix->ev_front.size() < n_sub) {
            hipEvent_t e, f, g;
            RTX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            RTX_HIP(hipEventCreateWithFlags(&f, hipEventDisableTiming));
            RTX_HIP(hipEventCreateWithFlags(&g, hipEventDisableTiming));
            ix->ev_front.push_back(e);
            ix->ev_back.push_back(f);
            ix->ev_mid.push_back(g);
        }
    }
    const uint32_t n_side = r.n_side;
    // RTX_OPT_RUN_AHEAD: a run of this shape (two streams, no side class) leaves out the join at its end -- the next chunk may be enqueued
    // behind its last FRONT half (rtx_batch_download_then_run) -- and, enqueued that way itself (hold_join: into the other result set),
    // drops the join of the run before it: its first front halves wait for the scratch sets only.
    const bool ra = ix->run_ahead_opt != 0u && nsets == 2u && n_side == 0u && r.stream_dl && n_sub >= 2u;  // (RTX_OPT_STAGE_TIMING: the stage events are then those of whichever run recorded them last)
    if (ix->join_pending) {  // (hold_join)
        if (ra) ix->join_pending = false;
        else if ((rc = settle_join(ix))) return rc;
    }
    if (ra)
        for (uint32_t k = 0; k < 2u; k++)
            if (!ix->ev_set_free[k]) RTX_HIP(hipEventCreateWithFlags(&ix->ev_set_free[k], hipEventDisableTiming));
    for (uint32_t sb = 0; sb < n_sub; sb++) {
        SubBatch b = sub_batch_of(ix, sb, timed);  // (with its length class: planes, strides, kernels)
        const bool side = b.cls->side;
        if (side) {  // (the side classes come first: sub-batches 0 .. n_side - 1, one after the other through their own set)
            b.set = kSideSet;
            if (overlap) {
                // ... and as a whole on the stream of the BACK halves, in front of them: a few waves per kernel, every one a long chain of
                // round trips (6 000 rows through one wave, the recurrence of prob_table) -- 3 ms for ten reads of 1 .. 8 kb -- that hides
                // under the bulk's first front half.  (Until the library asked for eight hardware queues this was a stream of its own that
                // SHARED a queue: 12.0 ms per batch of 131 072 barcodes + ten long reads; with a queue of its own every launch of the chain
                // queued for a slot on a full device and the batch took 13.0; in front of the bulk on the handle's stream: 14.7.)
                // Their result rows go to the top of the arena through a cursor of their own (walk_params); they are finalised first.
                if (sb == 0) {
                    RTX_HIP(hipEventRecord(ix->ev_mid[0], ix->stream));  // the processing order and the exact matches are in place
                    RTX_HIP(hipStreamWaitEvent(ix->stream2, ix->ev_mid[0], 0));
                }
                b.s = ix->stream2;
            }
        } else if (overlap) {
            const uint32_t m = sb - n_side;  // among the sub-batches of the bulk
            b.set = m % nsets;
            if (m >= nsets) RTX_HIP(hipStreamWaitEvent(ix->stream, ix->ev_back[sb - nsets], 0));  // the scratch set is free again
            else if (ra && ix->set_busy[b.set]) RTX_HIP(hipStreamWaitEvent(ix->stream, ix->ev_set_free[b.set], 0));  // ... of the run before (run-ahead)
        }
        if ((rc = enqueue_count(ix, b, flags, nsets == 3u && !side && n_side == 0 ? ix->stream3 : nullptr))) return rc;
        if (overlap && !side) {
            RTX_HIP(hipEventRecord(ix->ev_front[sb], ix->hit_stream));
            b.s = ix->stream2;
            RTX_HIP(hipStreamWaitEvent(b.s, ix->ev_front[sb], 0));
        }
        {   // the peak of every query of the sub-batch, from the histogram the probability stage is about to read (rtx_strand.hip)
            const rtx_index::Scratch &sc = ix->sc[b.set];
            launch_peak(b.s, PeakParams{sc.d_hist.p, b.cls->hstride, sc.d_t.p, b.q0, r.d_perm.p, b.nq, r.d_peak2.p});
        }
        if (r.has_nearest) {  // RTX_OPT_NEAREST: which reference holds it, from what the counting epilogues left (rtx_nearest.hip)
            rtx_index::Scratch &sc = ix->sc[b.set];
            const rtx_index::BatchClass &k = *b.cls;
            NearestParams np{};
            np.hist = sc.d_hist.p;
            np.hstride = k.hstride;
            np.t = sc.d_t.p;
            np.q0 = b.q0;
            np.perm = r.d_perm.p;
            np.nq = b.nq;
            np.tile_max = sc.d_tilemax.p;
            np.ntiles = ix->ntiles;
            np.n_refs = ix->n_refs;
            np.counts = sc.d_counts.p;
            np.counts_lo = ix->packs(k.planes) ? counts_lo(ix, sc) : nullptr;
            np.counts_hi = ix->packs(k.planes) ? counts_hi(ix, k, sc) : nullptr;
            np.npad = ix->npad;
            np.cnt_rows = counts_rows_layout(ix, k);
            np.cnt_row = on_diet(ix, k, sc) ? sc.d_cnt_row.p : nullptr;
            if (on_records_path(ix, k, sc)) {
                const RecordRef rr = record_ref(ix, sc, r);
                np.rec_nslots = rr.nslots;
                np.rec_slots = rr.slots;
                np.rec_cnt = rr.cnt;
                np.rec = rr.rec;
                np.rec_stride = rr.stride;
                np.rec_seg_len = rr.seg_len;
            }
            np.nearest = r.d_nearest2.p;
            np.ties = r.d_ties2.p;
            if (b.timed_all) {  // (not one of the stages of rtx_batch_stage_times, whose number is part of the ABI: rtx_batch_nearest_time)
                while (ix->ev_near.size() < 2u * ((size_t)sb + 1u)) {
                    hipEvent_t e;
                    RTX_HIP(hipEventCreate(&e));
                    ix->ev_near.push_back(e);
                }
                RTX_HIP(hipEventRecord(ix->ev_near[2u * sb], b.s));
            }
            launch_nearest(b.s, np);
            if (b.timed_all) {
                RTX_HIP(hipEventRecord(ix->ev_near[2u * sb + 1u], b.s));
                ix->n_near_last = sb + 1u;
            }
        }
        if ((rc = enqueue_prob_prefix(ix, b, fuse))) return rc;
        if (!fuse && (rc = enqueue_walk(ix, b, ix->sc[b.set].d_prefix.p, b.s))) return rc;
        if (fuse && b.timed_all) {  // keeps rtx_batch_stage_times whole: an empty interval
            RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_LINEAGE_WALK, 0), b.s));
            RTX_HIP(hipEventRecord(stage_event(ix, b, RTX_STAGE_LINEAGE_WALK, 1), b.s));
        }
        // the rows of the sub-batch finalised on the device (rtx_finalise.hip).  The launches of a run follow one another -- a sub-batch's rows
        // are then a range of the final arrays: the side classes' first, then the bulk's, on the stream of the back halves
        if ((rc = enqueue_finalise(ix, b, b.s))) return rc;
        if (r.stream_dl) {
            RTX_HIP(hipMemcpyAsync(&r.h_cursor_sub[sb], r.d_cursor.p + (side ? 1 : 0), 8, hipMemcpyDeviceToHost, b.s));
            RTX_HIP(hipEventRecord(r.ev_sub[sb], b.s));
        }
        if (overlap) RTX_HIP(hipEventRecord(ix->ev_back[sb], b.s));
        if (ra) {
            RTX_HIP(hipEventRecord(ix->ev_set_free[b.set], b.s));
            ix->set_busy[b.set] = true;
        }
    }
    if (ra) {  // the join is left to whoever needs it (settle_join)
        ix->join_pending = true;
        ix->join_ev = ix->ev_back[n_sub - 1];
    } else if (overlap && n_sub) {  // a wait for the handle's stream covers all of them
        RTX_HIP(hipStreamWaitEvent(ix->stream, ix->ev_back[n_sub - 1], 0));
        if (n_side && n_side < n_sub) RTX_HIP(hipStreamWaitEvent(ix->stream, ix->ev_back[n_side - 1], 0));  // (a batch of side classes alone)
    }
    {   // the flags of the run, behind its last kernel (the handle's stream has joined the others): the download finds them in page-locked memory
        int rc_f = r.h_flags.resize(1);
        if (rc_f) return rc_f;
        const hipStream_t fs = ra ? ix->stream2 : ix->stream;  // (run-ahead: behind the last back half -- every front half lies before it)
        {   // strand and peak of the caller's queries; under RTX_OPT_STRAND the final fields of the chosen orientation (rtx_strand.hip)
            const bool both = r.n_user != r.n_q;
            if (both && (r.n_q != 2u * r.n_user || !r.d_sel_t.p || r.d_sel_t.n < r.n_user)) { set_error("internal: a batch of both strands without its twins"); return RTX_ERR_STATE; }
            launch_strand_select(fs, StrandParams{(uint32_t)r.n_user, both ? 1u : 0u, r.d_peak2.p, r.d_fin_status.p, r.d_fin_t.p, r.d_fin_gs.p, r.d_fin_row_begin.p,
                                                  r.d_fin_row_count.p, r.d_strand.p, r.d_peak.p, r.d_sel_status.p, r.d_sel_t.p, r.d_sel_gs.p, r.d_sel_row_begin.p,
                                                  r.d_sel_row_count.p, r.has_nearest ? r.d_nearest2.p : nullptr, r.has_nearest ? r.d_ties2.p : nullptr,
                                                  r.has_nearest ? r.d_nearest.p : nullptr, r.has_nearest ? r.d_ties.p : nullptr});
            if (r.has_identity) {  // RTX_OPT_IDENTITY: every query of the caller against the reference just chosen for it (rtx_identity.hip)
                // The query bytes are those of the batch's input set, which is not staged again before this run has been downloaded (a
                // prefetch goes to the OTHER set until the next activation, and that follows this run's download, which waits for the
                // event below): the guarantee the text kernel reads the same bytes under.
                const rtx_index::Inputs &in = ix->in[r.in_set];
                IdentityParams ip{};
                ip.n = (uint32_t)r.n_user;
                ip.max_len = (uint32_t)std::min<uint64_t>(in.max_len, 0xFFFFFFFFull);
                ip.nearest = r.d_nearest.p;
                ip.strand = r.d_strand.p;
                ip.qbytes = in.d_packed.p;
                ip.qoff = in.d_base_off.p;
                ip.packed = in.packed;
                ip.ref_grp = ix->d_em_ref_grp.p;
                ip.rep_off = ix->d_em_rep_off.p;
                ip.rep_bytes = ix->d_em_rep_bytes.p;
                ip.n_refs = (uint32_t)ix->n_refs;
                ip.dist = r.d_dist.p;
                ip.qlen = r.d_qlen.p;
                const bool timed_id = ix->stage_timing != 0u;  // (not one of the stages of rtx_batch_stage_times: rtx_batch_identity_time)
                if (timed_id) {
                    for (auto &e : ix->ev_ident)
                        if (!e) RTX_HIP(hipEventCreate(&e));
                    RTX_HIP(hipEventRecord(ix->ev_ident[0], fs));
                }
                launch_identity(fs, ip);
                if (timed_id) {
                    RTX_HIP(hipEventRecord(ix->ev_ident[1], fs));
                    ix->ident_timed = true;
                }
            }
            if (!r.ev_select) RTX_HIP(hipEventCreateWithFlags(&r.ev_select, hipEventDisableTiming));
            RTX_HIP(hipEventRecord(r.ev_select, fs));
            r.has_peak = true;
        }
        RTX_HIP(hipMemcpyAsync(r.h_flags.data(), r.d_flags.p, 4, hipMemcpyDeviceToHost, fs));
        if (!r.ev_flags) RTX_HIP(hipEventCreateWithFlags(&r.ev_flags, hipEventDisableTiming));
        RTX_HIP(hipEventRecord(r.ev_flags, fs));
    }
    RTX_HIP(hipGetLastError());
    return RTX_OK;
}

// Builds (once per handle and tmax) the memoised cmf tables used by prob_lookup_kernel.
constexpr uint32_t kProbTablesMaxT = (uint32_t)2047;  // (= kMidClassMaxT: 0.74 GB at t = 651, 9 GB at t = 1 493, 23 GB at t = 2 047)
int ensure_prob_tables(rtx_index *ix, uint32_t tmax, bool *usable) {
    *usable = false;
    if (ix->prob_mode == 1 || tmax < 2) return RTX_OK;
    if (tmax > kProbTablesMaxT) {
        if (ix->prob_mode == 2) { set_error("prob tables need t <= %u (got %u)", kProbTablesMaxT, tmax); return RTX_ERR_TOO_LONG; }
        return RTX_OK;
    }
    if (ix->tab_tmax >= tmax) { *usable = true; return RTX_OK; }
    const uint32_t T = tmax;
    std::vector<uint64_t> off(T + 1, 0);
    std::vector<uint32_t> moff(T + 1, 0);
    uint64_t run = 0;
    uint32_t mrun = 0;
    for (uint32_t t = 2; t <= T; t++) {
        off[t] = run;
        moff[t] = mrun;
        run += (uint64_t)t * (t / 2 + 1);
        mrun += t;
    }
    int rc;
    size_t free_b = 0, total_b = 0;
    RTX_HIP(hipMemGetInfo(&free_b, &total_b));
    if (run * 16 > free_b / 2) {  // keep at least half of the free HBM for the batch workspace
        if (ix->prob_mode == 2) { set_error("prob tables (%llu bytes) do not fit", (unsigned long long)(run * 16)); return RTX_ERR_OOM; }
        return RTX_OK;
    }
    if ((rc = ix->d_tab_cmf.alloc(run)) || (rc = ix->d_tab_ratio.alloc(run)) || (rc = ix->d_tab_off.alloc(T + 1)) ||
        (rc = ix->d_tab_moff.alloc(T + 1)) || (rc = ix->d_tab_ilo.alloc(mrun)) || (rc = ix->d_tab_sat.alloc(2 * (size_t)mrun)))
        return rc;
    RTX_HIP(hipMemcpy(ix->d_tab_off.p, off.data(), (T + 1) * 8, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(ix->d_tab_moff.p, moff.data(), (T + 1) * 4, hipMemcpyHostToDevice));
    ProbTables tb = prob_tables(ix);
    tb.tmax = T;  // (tab_tmax follows once they are built)
    launch_prob_tables_build(ix->stream, tb, ix->d_lnfact.p, ix->d_inv.p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(ix->stream));
    ix->tab_tmax = T;
    *usable = true;
    return RTX_OK;
}

// Queries per kernel launch: larger sub-batches amortise launch tails (measured: 4096 -> 8192 queries saves
// 5 % of a step at N = 50k).
constexpr uint32_t kMaxSubBatch = 65536;
// default: fewer, larger launches save the drain/fill between the kernels of a sub-batch (N = 50k, per 100k queries: 10 000:
// 20.4 ms, 14 286: 21.3, 25 000: 20.3, 50 000: 22.0).  A large database gains from more queries per launch -- every tile's
// bitmap region is fetched once per launch and XCD, whatever the number of queries (N = 500k, per 1M queries: 10 240: 1 094 ms,
// 16 384: 1 072, 24 576: 1 070, 32 768: 1 098).  With the kernels of the end of round 2: N = 50k, per 100k queries: 10 000: 19.55 ms,
// 20 000: 19.08, 25 000: 21.1 (the last sub-batch's host work is no longer hidden), 50 000: 20.7; N = 500k, per 1 M queries:
// 8 192: 971 ms, 16 384: 953, 32 768: 964, 65 536: 995
// With tile pruning a sub-batch is far less work and the fixed cost of its nine launches counts: N = 500k, per 1 M queries:
// 8 192: 191 ms, 16 384: 171, 32 768: 159.5, 49 152: 158.1, 65 536: 157.8
// Round 4 (stages for every kernel, 113 ms per step): 32 768: 113.1 ms, 49 152: 111.0, 65 536: 109.7 -- fewer launches, fewer tails.
constexpr uint32_t kDefaultSubBatch = 20480, kDefaultSubBatchLarge = 16384, kDefaultSubBatchPruned = 65536;


// ---- length classes ----------------------------------------------------------------------------------------------------------
// class of a query by its length (t <= length - 7, known on the host when the batch is staged):
//   0: t <= 255    8 bit planes, pair kernel, memoised tables, tile pruning
//   1: t <= 1023  10 bit planes, the same
//   2: t <= 2047  11 bit planes, the same with u16 counts (round 6: full-length 16S -- until then every read beyond 1 030 bases fell to class 3's
//                 one-query-per-wave kernel without pruning: 0.26 M reads of 1 500 bases per second against 12.9 M barcodes); fewer than
//                 kMinMidClass of them in a batch ride with class 3 (the tables of this class are gigabytes, built for the batch's longest read)
//   3: longer     12 / 16 planes, one query per wave, prob_table_kernel with its arrays in LDS (t up to ~ 6 600)
//   4: up to t = 65 535 (raxtax.rs:56): 16 planes, the histogram of hit_count and the arrays of prob_table in global memory
constexpr uint64_t kMidClassMaxT = 2047;

uint32_t length_class(uint64_t len) {
    const uint64_t t = len >= 8 ? len - 7 : 1;
    if (t <= 255) return 0;
    if (t <= 1023) return 1;
    if (t <= kMidClassMaxT) return 2;
    return t <= 65535 && prob_table_lds_bytes((uint32_t)t) <= kProbTableLdsLimit ? 3u : 4u;
}
uint64_t class3_max_len() {  // the longest query of class 3: where prob_table's arrays still fit LDS
    static uint64_t cached = 0;
    if (!cached) {
        uint64_t lo = kMidClassMaxT + 8, hi = 65535 + 7;
        while (lo < hi) { const uint64_t mid = (lo + hi + 1) / 2; if (length_class(mid) <= 3u) lo = mid; else hi = mid - 1; }
        cached = lo;
    }
    return cached;
}
constexpr uint64_t kSideMaxQueries = 2048;  // a class of at most this many queries (and a 64th of the bulk) runs as a side class
constexpr uint64_t kMinShortClass = 4096;  // fewer queries of t <= 255 than this ride with the t <= 1023 class (same results: 8 or 10 planes hold their counts)
constexpr uint64_t kMinMidClass = 4096;    // fewer queries of 1024 <= t <= 2047 than this ride with the longer reads (one query per wave, the recurrence kernel)

// mid: the class of 1024 <= t <= 2047 proper (eleven planes: pair kernel, pruning, tables); reads of that length that ride with the longer
// ones (too few of them, a reference shard) keep the twelve-plane form of the one-query-per-wave kernel and the recurrence kernel
static void shape_class(rtx_index::BatchClass &k, uint64_t n, uint64_t max_len, bool mid = false) {
    // t <= min(len - 7, 65536): the reference asserts on the DISTINCT k-mers of a read (raxtax.rs:56, utils.rs:27-40), so a read of any
    // length is served; one that really holds all 65 536 8-mers is reported per query (RTX_Q_ALL_KMERS, kmer_extract_kernel)
    const uint64_t tmax = std::min<uint64_t>(max_len >= 8 ? max_len - 7 : 1, 65535);
    k = rtx_index::BatchClass();
    k.n = n;
    k.max_len = max_len;
    k.tmax = (uint32_t)tmax;
    k.kstride = (uint32_t)align_up(tmax, 8);
    k.rstride = (uint32_t)align_up(tmax, 64) + 64;  // row list padded to whole 64-row chunks
    k.hstride = (uint32_t)align_up(tmax + 1, 8);
    k.planes = tmax <= 255 ? 8 : (tmax <= 1023 ? 10 : (tmax <= kMidClassMaxT && mid ? 11 : (tmax <= 4095 ? 12 : 16)));  // (8 / 10 / 11: the pair kernel)
    k.huge = prob_table_lds_bytes((uint32_t)tmax) > kProbTableLdsLimit;
}

static int size_workspace(rtx_index *ix, uint64_t n_queries);

// Sizes and allocates the per-batch workspace for the staged batch: n_queries queries, cls_n[c] of them in length class c (the longest of
// which has cls_max[c] bases).
int prepare_workspace(rtx_index *ix, uint64_t n_queries, const uint64_t cls_n_in[5], const uint64_t cls_max_in[5]) {
    uint64_t cn[5], cm[5];
    for (int c = 0; c < 5; c++) { cn[c] = cls_n_in[c]; cm[c] = cls_max_in[c]; }
    if (ix->n_refs != ix->n_total) {  // a reference shard: the exchange buffers of rtx_shard_* have one row stride -- one class (a k-mer shard holds every reference and is not
                                      // caught here: its staged run is launched in the shape of cls[0] whatever its classes, shard_sb)
        uint64_t mx = 0;
        for (int c = 0; c < 5; c++) mx = std::max(mx, cm[c]);
        return prepare_workspace_single(ix, n_queries, mx >= 8 ? mx - 7 : 1, mx);
    }
    // a handful of short reads among barcodes ride with them (the results do not depend on the number of planes)
    if (cn[0] && cn[1] && cn[0] < kMinShortClass) { cn[1] += cn[0]; cm[1] = std::max(cm[1], cm[0]); cn[0] = 0; cm[0] = 0; }
    // a few reads of 1 031 .. 2 054 bases (among barcodes, or alone) ride with the longer ones: the pruned path of their own class needs
    // memoised tables of gigabytes (t^3), built for the longest read -- not for a handful of queries.  (No pair kernel, no pruning: no such class.)
    if (cn[2] && ((cn[2] < kMinMidClass && ix->prob_mode != 2) || !ix->pair_opt || !ix->pruning() || ix->prob_mode == 1)) { cn[3] += cn[2]; cm[3] = std::max(cm[3], cm[2]); cn[2] = 0; cm[2] = 0; }
    // ... and a handful of reads of a few kilobases with the longer ones still (one set of launches; the global-memory forms compute the same values)
    if (cn[3] && cn[4] && cn[3] + cn[4] <= kSideMaxQueries) { cn[4] += cn[3]; cm[4] = std::max(cm[4], cm[3]); cn[3] = 0; cm[3] = 0; }
    const uint64_t key[14] = {n_queries, cn[0], cn[1], cn[2] << 32 | cn[3], cn[4], cm[0], cm[1], cm[2] << 32 | cm[3], cm[4], ix->sub_batch_req,
                              (uint64_t)ix->packed_opt | (uint64_t)ix->pair_opt << 1 | (uint64_t)ix->pruning() << 2 | (uint64_t)ix->shard_prune_opt << 3 | (uint64_t)ix->fine_opt << 4 |
                                  (uint64_t)(ix->prob_mode & 3) << 5 | (uint64_t)ix->rec_opt << 8 | (uint64_t)ix->overlap_opt << 16 | (uint64_t)ix->min_subs << 20,
                              (uint64_t)ix->n_bnd_local, ix->shared_device ? 1u : 0u, ix->strand_opt | ix->nearest_opt << 1 | ix->identity_opt << 2};
    // A batch of the shape of the last one under the same options (the chunks of rtx_raxtax): everything below would come out the same --
    // and hipMemGetInfo alone costs a good part of a millisecond between two chunks, with the device idle
    if (ix->ws_valid && std::memcmp(key, ix->ws_key, sizeof key) == 0 && !ix->staged) {
        ix->n_q = n_queries;
        return RTX_OK;
    }
    ix->ws_valid = false;
    // (reads beyond 65 542 bases belong to the last class; t is what kmer_extract finds, at most 65 535 -- or the query is flagged)
    ix->n_cls = 0;
    // the longest query each class may hold: the sort rank of a query is the number of class boundaries its length exceeds
    const uint64_t cls_len[4] = {255 + 7, 1023 + 7, kMidClassMaxT + 7, class3_max_len()};
    for (int c = 0; c < 4; c++) ix->key_lim[c] = ~0ull;
    int last = -1;
    for (int c = 0; c < 5; c++) {
        if (!cn[c]) continue;
        if (last >= 0) ix->key_lim[ix->n_cls - 1] = cls_len[last];  // a boundary between two classes that both exist
        shape_class(ix->cls[ix->n_cls], cn[c], cm[c], c == 2);
        ix->n_cls++;
        last = c;
    }
    if (ix->n_cls == 0) { set_error("internal: a batch without queries"); return RTX_ERR_INVALID; }
    ix->n_q = n_queries;
    int rc = size_workspace(ix, n_queries);
    if (rc) return rc;
    std::memcpy(ix->ws_key, key, sizeof key);
    ix->ws_valid = true;
    return RTX_OK;
}

// One class whatever the lengths: reference shards (rtx_shard_*: one row stride for the exchange buffers), rtx_debug_evaluate.
int prepare_workspace_single(rtx_index *ix, uint64_t n_queries, uint64_t tmax, uint64_t max_len) {
    ix->ws_valid = false;
    ix->strand_used = false;
    tmax = std::min<uint64_t>(tmax, 65535);  // (shape_class)
    ix->n_cls = 1;
    for (int c = 0; c < 4; c++) ix->key_lim[c] = ~0ull;
    shape_class(ix->cls[0], n_queries, tmax + 7);
    ix->cls[0].max_len = max_len;
    ix->n_q = n_queries;
    return size_workspace(ix, n_queries);
}

static int size_workspace(rtx_index *ix, uint64_t n_queries) {
    int rc;
    // the memoised probability tables serve every class with t <= 1023: built for the longest of them
    uint32_t tab_t = 0;
    for (uint32_t c = 0; c < ix->n_cls; c++) {
        if (ix->cls[c].tmax > kProbTablesMaxT && ix->prob_mode == 2) { set_error("prob tables need t <= %u (got %u)", kProbTablesMaxT, ix->cls[c].tmax); return RTX_ERR_TOO_LONG; }
        if (ix->cls[c].tmax <= kProbTablesMaxT && ix->cls[c].planes <= 11) tab_t = std::max(tab_t, ix->cls[c].tmax);  // (not for mid-length reads that ride with the longer ones)
    }
    bool tables = false;
    if (tab_t && (rc = ensure_prob_tables(ix, tab_t, &tables))) return rc;
    for (uint32_t c = 0; c < ix->n_cls; c++) ix->cls[c].use_tables = tables && ix->cls[c].tmax >= 2 && ix->cls[c].tmax <= kProbTablesMaxT && ix->cls[c].planes <= 11;
    // ---- per-query results
    rtx_index::ResultSet &r = ix->res();
    if ((rc = alloc_result_set(ix, r, n_queries))) return rc;
    if ((rc = ix->d_sub_alloc.alloc((size_t)kWalkSubAllocs * kWalkSubStride))) return rc;
    const uint64_t want_arena = n_queries * 10 + 4096;  // (alloc_result_set)
    // ---- sub-batch scratch, sized against free HBM: every class gets the sub-batch size its own shape allows, the buffers the largest
    // product over the classes (a class runs after the other through the same buffers)
    // RTX_OPT_OVERLAP: two (three) scratch sets -- not for a handle that shares its device with another one driven beside it (rtx_raxtax_multi):
    // two sets of 60 GB each per handle (N = 500k, sub-batches of 65 536) left the second handle of a device a sliver of HBM and sub-batches of
    // a few thousand queries: a tenth of the speed
    uint32_t n_sets = ix->n_refs == ix->n_total && !ix->shared_device ? 1u + std::min<uint32_t>(ix->overlap_opt, 2u) : 1u;
    size_t free_b = 0, total_b = 0;
    RTX_HIP(hipMemGetInfo(&free_b, &total_b));
    uint64_t held = 0;  // scratch already held by this handle is reusable
    for (const auto &sc : ix->sc) held += sc.d_counts.n * 2 + sc.d_prefix.n * 8 + sc.d_rec.n * 4 + sc.d_srows.n * 4;
    const uint64_t budget = (uint64_t)((free_b + held) * 0.6);
    uint64_t worst = 0;
    for (uint32_t c = 0; c < ix->n_cls; c++) {
        rtx_index::BatchClass &k = ix->cls[c];
        k.will_prune = ix->pruning() && ix->d_ubitmap.p && ix->pair_opt && ix->ntiles >= RTX_PRUNE_MIN_TILES && k.tmax <= kProbTablesMaxT && (ix->n_refs == ix->n_total || ix->shard_prune_opt);  // begin_run decides
        const uint64_t per_q = class_per_q(ix, k);
        uint32_t B = ix->sub_batch_req;
        if (B == 0) {
            B = (uint32_t)std::min<uint64_t>(k.will_prune ? kDefaultSubBatchPruned : ix->ntiles >= 16 ? kDefaultSubBatchLarge : kDefaultSubBatch,
                                             std::max<uint64_t>(64, budget / per_q));
            if (k.huge) B = std::min<uint32_t>(B, 1024u);
            // at least four sub-batches per batch (of 16 384 queries or more): the records of a finished sub-batch are copied and finalised on
            // the host while the next ones run, and what is left when the device is done is the last sub-batch -- a chunk of 131 072 queries
            // (rtx_raxtax) in two halves left 7 ms of host work exposed on real barcodes (ten result rows per query)
            if (k.will_prune && k.n < (uint64_t)ix->min_subs * B) B = (uint32_t)std::max<uint64_t>(16384, (k.n + ix->min_subs - 1) / ix->min_subs);
        }
        if (B > kMaxSubBatch) B = kMaxSubBatch;
        B = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(B, k.n));
        k.sub_batch = B;
        worst = std::max<uint64_t>(worst, (uint64_t)B * per_q);
    }
    // side classes: a handful of queries of another length beside the bulk (ten 16S reads in a file of barcodes)
    {
        uint32_t bulk = 0;
        for (uint32_t c = 1; c < ix->n_cls; c++)
            if (ix->cls[c].n > ix->cls[bulk].n) bulk = c;
        worst = 0;
        for (uint32_t c = 0; c < ix->n_cls; c++) {
            ix->cls[c].side = ix->n_refs == ix->n_total && c != bulk && ix->cls[c].n <= kSideMaxQueries && ix->cls[c].n * 64u <= ix->cls[bulk].n;
            if (!ix->cls[c].side) worst = std::max<uint64_t>(worst, (uint64_t)ix->cls[c].sub_batch * class_per_q(ix, ix->cls[c]));
        }
    }
    {   // room for the rows of the side classes at the top of the arena (begin_run: side_base)
        uint64_t n_side_q = 0;
        for (uint32_t c = 0; c < ix->n_cls; c++)
            if (ix->cls[c].side) n_side_q += ix->cls[c].n;
        const uint64_t want2 = want_arena + (n_side_q ? n_side_q * kWalkMaxRows + 64 : 0);
        if (r.arena_cap < want2) {
            if ((rc = r.d_arena.alloc(want2))) return rc;
            r.arena_cap = want2;
        }
    }
    // the further sets of the overlap never shrink a sub-batch: they are taken only while they fit the budget beside the first
    while (n_sets > 1u && (uint64_t)n_sets * worst > budget) n_sets--;
    ix->staged = false;
    if ((rc = plan_sub_batches(ix))) return rc;
    if ((rc = alloc_scratch_set(ix, 0))) return rc;
    {
        bool any_side = false;
        for (uint32_t c = 0; c < ix->n_cls; c++) any_side = any_side || ix->cls[c].side;
        if (any_side) { if ((rc = alloc_scratch_set(ix, kSideSet))) return rc; }
        else ix->sc[kSideSet].release_all();
    }
    for (uint32_t k = 1; k <= 2u; k++) {  // (without the further sets the run stays on one stream)
        if (k < n_sets && ix->n_sub_total() > 1) {
            if (alloc_scratch_set(ix, k)) ix->sc[k].d_kmers.release();
        } else if (ix->n_refs == ix->n_total) {
            ix->sc[k].release_all();  // none wanted on a whole-database handle: given back (a shard keeps its second set for rtx_shard_begin)
        }
    }
    return RTX_OK;
}

// One set of sub-batch scratch (scratch_set_need).  The buffers every run needs are mandatory; a group that only a faster path needs is given
// up whole when one of its allocations fails (begin_run and enqueue_hit then leave that path out).
int alloc_scratch_set(rtx_index *ix, uint32_t k) {
    int rc;
    rtx_index::Scratch &sc = ix->sc[k];
    const ScratchNeed n = scratch_set_need(ix, k);
    if ((rc = sc.d_kmers.alloc(n.kmers)) || (rc = sc.d_rows.alloc(n.rows)) || (rc = sc.d_dmask.alloc(n.dmask)) || (rc = sc.d_nsparse.alloc(n.nsparse)) || (rc = sc.d_srows.alloc(n.srows)) ||
        (rc = sc.d_t.alloc(n.t)) || (rc = sc.d_nrows.alloc(n.nrows)) || (rc = sc.d_counts.alloc(n.counts)) || (rc = sc.d_hist.alloc(n.hist)) || (rc = sc.d_table_z.alloc(n.hist)) ||
        (rc = sc.d_prefix.alloc(n.prefix)) || (rc = sc.d_order.alloc(n.order)) || (rc = sc.d_tilemax.alloc(n.tilemax)) || (rc = sc.d_urec.alloc(n.urec)) || (rc = sc.d_nu.alloc(n.nu)))
        return rc;
    if (n.prob_scratch && (rc = ix->d_prob_scratch.alloc(std::max(n.prob_scratch, ix->d_prob_scratch.n)))) return rc;
    if (ix->pruning() && ix->d_ubitmap.p && (ix->n_refs == ix->n_total || ix->shard_prune_opt)) {
        if ((rc = sc.d_tile_ub.alloc(n.tile_ub)) || (rc = sc.d_best_key.alloc(n.best_key)) || (rc = sc.d_prune_thr.alloc(n.prune_thr)) || (rc = sc.d_prune_i1.alloc(n.prune_i1)) ||
            (rc = sc.d_best.alloc(n.best)) || (rc = sc.d_live.alloc(n.live)) || (rc = sc.d_items.alloc(n.items)))
            return rc;
        if (ix->d_abitmap.p && (sc.d_heavy.alloc(n.heavy) || sc.d_heavy_items.alloc(n.heavy_items))) { sc.d_heavy.release(); sc.d_heavy_items.release(); }
        // (a failed allocation of the fine pass's lists only switches the pass off: enqueue_hit tolerates a null pointer)
        if (ix->d_fbitmap.p && sc.d_fine_items.alloc(n.fine_items)) sc.d_fine_items.release();
        if (ix->rec_opt && ix->n_refs == ix->n_total) {  // the records path; without its buffers the run takes the dense epilogues
            if (sc.d_rec_nslots.alloc(n.rec_nslots) || sc.d_rec_slots.alloc(n.rec_slots) || sc.d_rec_cnt.alloc(n.rec_cnt) ||
                sc.d_rec.alloc(n.rec) || sc.d_cnt_row.alloc(n.cnt_row) || sc.d_cnt_cursor.alloc(n.cnt_cursor) || sc.d_dense_q.alloc(n.dense_q))
                sc.d_rec.release();
        }
    }
    return RTX_OK;
}

}  // namespace rtxi

extern "C" {

// Stages a batch in the input set that is NOT the current one: validation, bases packed two per byte into pinned memory (threads of
// the library's budget), offsets and exact-match ids beside them, asynchronous H2D on a stream of its own.  The batch that is running
// (or whose results are being downloaded) is not touched: rtx_raxtax stages chunk c + 1 while chunk c is classified.
int rtx_batch_prefetch(rtx_index *ix, uint64_t n_queries, const uint8_t *bases, const uint64_t *base_off,
                       const uint32_t *exact_ids, const uint64_t *exact_off) {
    int rc = bind(ix);
    if (rc) return rc;
    rtx_index::Inputs &in = ix->in[ix->cur_in ^ 1u];
    // labels staged for this batch (rtx_batch_prefetch_labels) belong to it alone: taken or dropped here, whatever becomes of the call
    const bool with_labels = in.labels_pending && in.n_labels == n_queries;
    in.labels_pending = in.has_labels = false;
    const bool with_weights = in.weights_pending && in.n_weights == n_queries;  // ... and so do its weights (rtx_batch_prefetch_weights)
    in.weights_pending = in.has_weights = false;
    const bool with_samples = in.samples_pending && in.n_samples == n_queries;  // ... and its samples (rtx_batch_prefetch_samples)
    in.samples_pending = in.has_samples = false;
    if (n_queries == 0 || !base_off || (!bases && base_off[n_queries])) {
        set_error("rtx_batch_upload: invalid argument");
        return RTX_ERR_INVALID;
    }
    // RTX_OPT_STRAND: the activation appends the reverse complement of every query (rtx_strand.hip); room for the twins is made here
    const bool both = ix->strand_opt != 0u;
    if (both) {
        if (exact_off || exact_ids) { set_error("RTX_OPT_STRAND: exact-match ids cannot be passed in (those of the reverse complements must come from the same lookup: pass NULL)"); return RTX_ERR_INVALID; }
        if (!rtx_index_has_exact_lookup(ix) || ix->n_refs != ix->n_total) { set_error("RTX_OPT_STRAND needs the exact-match lookup of the device (a handle built from the reference sequences, RTX_OPT_DEVICE_EXACT on)"); return RTX_ERR_STATE; }
        if (n_queries > 0x7FFFFFFFull) { set_error("RTX_OPT_STRAND: too many queries in one batch"); return RTX_ERR_INVALID; }
    }
    const uint64_t n_dev = both ? 2 * n_queries : n_queries;  // queries of the batch on the device
    if (!ix->h2d_stream) RTX_HIP(hipStreamCreateWithFlags(&ix->h2d_stream, hipStreamNonBlocking));
    if (!in.ready) RTX_HIP(hipEventCreateWithFlags(&in.ready, hipEventDisableTiming));
    if (in.recorded) RTX_HIP(hipEventSynchronize(in.ready));  // the last transfer out of this set's pinned buffers (long done, as a rule)
    in.staged = false;
    if (ix->ev_activated) RTX_HIP(hipStreamWaitEvent(ix->h2d_stream, ix->ev_activated, 0));  // the batch that read this set has run
    uint64_t max_len = 0;
    uint64_t cls_n[5] = {0, 0, 0, 0, 0}, cls_max[5] = {0, 0, 0, 0, 0};  // the length classes of the batch (length_class)
    {
        const uint64_t lim3 = class3_max_len();
        for (uint64_t q = 0; q < n_queries; q++) {
            if (base_off[q + 1] < base_off[q]) { set_error("base_off not monotone at query %llu", (unsigned long long)q); return RTX_ERR_INVALID; }
            const uint64_t len = base_off[q + 1] - base_off[q];
            max_len = std::max(max_len, len);
            const int c = len <= 262 ? 0 : (len <= 1030 ? 1 : (len <= kMidClassMaxT + 7 ? 2 : (len <= lim3 ? 3 : 4)));
            cls_n[c]++;
            cls_max[c] = std::max(cls_max[c], len);
        }
    }
    const uint64_t total = base_off[n_queries] - base_off[0];
    uint64_t n_exact = 0;
    if (exact_off) {
        if (exact_off[0] != 0) { set_error("exact_off[0] must be 0"); return RTX_ERR_INVALID; }
        n_exact = exact_off[n_queries];
        for (uint64_t q = 0; q < n_queries; q++)
            if (exact_off[q + 1] < exact_off[q]) { set_error("exact_off not monotone"); return RTX_ERR_INVALID; }
        if (n_exact && !exact_ids) { set_error("exact_ids is null"); return RTX_ERR_INVALID; }
        for (uint64_t i = 0; i < n_exact; i++)
            if (exact_ids[i] >= ix->n_total) { set_error("exact id %u out of range", exact_ids[i]); return RTX_ERR_INVALID; }
    }
    const uint64_t n_packed = (total + 1) / 2;
    if ((rc = in.h_packed.resize(total + 64)) || (rc = in.h_base_off.resize(n_queries + 1)) || (rc = in.d_packed.alloc(total + 64)) ||
        (rc = in.d_base_off.alloc(n_dev + 1)) || (rc = in.d_exact_off.alloc(n_dev + 1)) || (rc = in.d_exact_ids.alloc(n_exact + 1)))
        return rc;
    for (uint64_t q = 0; q <= n_queries; q++) in.h_base_off[q] = base_off[q] - base_off[0];
    // two bases per byte; a byte above 15 is no code of parser.rs:11-34 -- such a batch travels as it is (the kernels see the caller's bytes)
    in.packed = total == 0 || rtx::pack_nibbles_mt(bases + base_off[0], total, in.h_packed.data(), rtx::host_threads(8u));
    if (!in.packed) std::memcpy(in.h_packed.data(), bases + base_off[0], total);
    RTX_HIP(hipMemcpyAsync(in.d_packed.p, in.h_packed.data(), in.packed ? n_packed : total, hipMemcpyHostToDevice, ix->h2d_stream));
    RTX_HIP(hipMemcpyAsync(in.d_base_off.p, in.h_base_off.data(), (n_queries + 1) * 8, hipMemcpyHostToDevice, ix->h2d_stream));
    if (exact_off) {
        if ((rc = in.h_exact_off.resize(n_queries + 1)) || (rc = in.h_exact_ids.resize(n_exact + 1))) return rc;
        std::memcpy(in.h_exact_off.data(), exact_off, (n_queries + 1) * 8);
        if (n_exact) std::memcpy(in.h_exact_ids.data(), exact_ids, n_exact * 4);
        RTX_HIP(hipMemcpyAsync(in.d_exact_off.p, in.h_exact_off.data(), (n_queries + 1) * 8, hipMemcpyHostToDevice, ix->h2d_stream));
        if (n_exact) RTX_HIP(hipMemcpyAsync(in.d_exact_ids.p, in.h_exact_ids.data(), n_exact * 4, hipMemcpyHostToDevice, ix->h2d_stream));
    } else {
        RTX_HIP(hipMemsetAsync(in.d_exact_off.p, 0, (n_dev + 1) * 8, ix->h2d_stream));
    }
    RTX_HIP(hipEventRecord(in.ready, ix->h2d_stream));
    in.recorded = true;
    in.n_q = n_dev;
    in.n_user = n_queries;
    in.total = total;
    in.max_len = max_len;
    for (int c = 0; c < 5; c++) { in.cls_n[c] = both ? 2 * cls_n[c] : cls_n[c]; in.cls_max[c] = cls_max[c]; }  // (a twin has the length of its query)
    in.n_exact = n_exact;
    in.has_exact = exact_off != nullptr;
    in.has_labels = with_labels;
    in.has_weights = with_weights;
    in.has_samples = with_samples;
    in.staged = true;
    return RTX_OK;
}

// The staged batch becomes the current one: the handle's stream waits for the transfer (the host does not), the workspace is sized
// for the batch (options that shape it are read here), the bases are unpacked.  The batch before it must have been downloaded.
int rtx_batch_activate(rtx_index *ix) {
    int rc = bind(ix);
    if (rc) return rc;
    rtx_index::Inputs &in = ix->in[ix->cur_in ^ 1u];
    if (!in.staged) { set_error("rtx_batch_activate without a staged batch (rtx_batch_prefetch)"); return RTX_ERR_STATE; }
    ix->uploaded = ix->ran = ix->synced = false;
    if ((rc = prepare_workspace(ix, in.n_q, in.cls_n, in.cls_max))) return rc;
    const bool both = in.n_q != in.n_user;  // staged under RTX_OPT_STRAND (setting the option drops what was staged)
    const uint64_t total_dev = both ? 2 * in.total : in.total;
    ix->sum_query_bytes = total_dev;
    if ((rc = ix->d_bases.alloc(total_dev + 64))) return rc;
    RTX_HIP(hipStreamWaitEvent(ix->stream, in.ready, 0));
    if (in.packed) {
        rtx::launch_unpack_nibbles(ix->stream, in.d_packed.p, ix->d_bases.p, in.total, in.total + 64);
    } else {
        RTX_HIP(hipMemcpyAsync(ix->d_bases.p, in.d_packed.p, in.total, hipMemcpyDeviceToDevice, ix->stream));
        RTX_HIP(hipMemsetAsync(ix->d_bases.p + in.total, 0, 64, ix->stream));
    }
    if (both) {  // query n + q = the reverse complement of query q; from here on the batch is 2 n queries for every stage
        rtx::launch_revcomp(ix->stream, ix->d_bases.p, in.d_base_off.p, (uint32_t)in.n_user, in.total);
        RTX_HIP(hipMemsetAsync(ix->d_bases.p + total_dev, 0, 64, ix->stream));
    }
    ix->strand_used = both;
    ix->n_user = in.n_user;
    ix->dev_exact_used = !in.has_exact && ix->dev_exact_opt && ix->d_em_table.p && ix->n_refs == ix->n_total;
    if (ix->dev_exact_used && (rc = ix->res().d_exact_grp.alloc(in.n_q))) return rc;
    if (!ix->ev_activated) RTX_HIP(hipEventCreateWithFlags(&ix->ev_activated, hipEventDisableTiming));
    RTX_HIP(hipEventRecord(ix->ev_activated, ix->stream));
    in.staged = false;
    ix->cur_in ^= 1u;
    ix->uploaded = true;
    return RTX_OK;
}

int rtx_pack_bases(const uint8_t *bases, uint64_t n_bases, uint8_t *packed) {
    if ((!bases || !packed) && n_bases) { set_error("rtx_pack_bases: null argument"); return RTX_ERR_INVALID; }
    return rtx::pack_nibbles_mt(bases, n_bases, packed, rtx::host_threads(8u)) ? 1 : 0;
}

int rtx_batch_upload(rtx_index *ix, uint64_t n_queries, const uint8_t *bases, const uint64_t *base_off,
                     const uint32_t *exact_ids, const uint64_t *exact_off) {
    if (ix) ix->uploaded = ix->ran = ix->synced = false;
    int rc = rtx_batch_prefetch(ix, n_queries, bases, base_off, exact_ids, exact_off);
    return rc ? rc : rtx_batch_activate(ix);
}

int rtx_batch_run(rtx_index *ix, uint32_t flags) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!ix->uploaded) { set_error("rtx_batch_run before rtx_batch_upload"); return RTX_ERR_STATE; }
    ix->last_flags = flags;
    ix->synced = false;
    rc = enqueue_batch(ix, flags);
    ix->ran = rc == RTX_OK;
    return rc;
}

int rtx_batch_sync(rtx_index *ix) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!ix->ran) { set_error("rtx_batch_sync before rtx_batch_run"); return RTX_ERR_STATE; }
    if ((rc = settle_join(ix))) return rc;
    RTX_HIP(hipStreamSynchronize(ix->stream));
    ix->synced = true;
    return RTX_OK;
}

}  // extern "C"

// Result download: the device finalises the rows of every sub-batch (rtx_finalise.hip: sort lineage.rs:91-93, expected vectors and local
// signal lineage.rs:95-102, final layout); the rows of finished sub-batches are copied into the page-locked arrays of the view while
// later sub-batches still run -- the host copies, it computes nothing; exact matches as the device found them; rtx_classify_batch.
#include "rtx_index.hpp"

namespace rtxi {

// The per-node tables of finalise_kernel (rtx_finalise.hip): depth, begin of the node's range (the lineage a row reports, lineage.rs:105),
// and the expected side of the local signal (lineage.rs:95-98,137-139): the level it starts at and per level the expected share
// |range of the ancestor| / N over the sum of those shares (rtx_math.hpp: fin_node_expected) -- everything of a row's local signal
// that depends on the node alone.
int node_tables(rtx_index *ix) {
    const FlatNodes &f = ix->nodes;
    const uint32_t D = std::max(1u, f.max_depth), nn = f.size();
    ix->fin_D = D;
    std::vector<uint8_t> depth(nn), sig0(nn);
    std::vector<double> eb((size_t)nn * D, 0.0);
    std::vector<uint32_t> size(D);
    const double N = (double)ix->n_total;
    for (uint32_t v = 0; v < nn; v++) {
        depth[v] = (uint8_t)f.depth[v];
        uint32_t anc = v;
        for (int d = (int)f.depth[v] - 1; d >= 0; d--) {
            size[d] = f.end[anc] - f.begin[anc];
            anc = f.parent[anc];
        }
        sig0[v] = (uint8_t)fin_node_expected(size.data(), f.depth[v], N, eb.data() + (size_t)v * D);
    }
    int rc;
    if ((rc = ix->d_node_depth.alloc(nn)) || (rc = ix->d_node_sig0.alloc(nn)) || (rc = ix->d_node_begin.alloc(nn)) || (rc = ix->d_node_eb.alloc((size_t)nn * D))) return rc;
    RTX_HIP(hipMemcpy(ix->d_node_depth.p, depth.data(), nn, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(ix->d_node_sig0.p, sig0.data(), nn, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(ix->d_node_begin.p, f.begin.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(ix->d_node_eb.p, eb.data(), (size_t)nn * D * 8, hipMemcpyHostToDevice));
    return RTX_OK;
}

// Host arrays of a download: the per-query fields for nq queries, the row arrays for at least `rows` rows with the first `keep` preserved
static int size_host_results(rtx_index *ix, rtx_index::HostRes &hr, uint64_t nq, uint64_t rows, uint64_t keep) {
    int rc;
    if ((rc = hr.h_t.resize(nq)) || (rc = hr.h_status.resize(nq)) || (rc = hr.h_gs.resize(nq)) || (rc = hr.v_row_begin.resize(nq)) ||
        (rc = hr.v_row_count.resize(nq)) || (rc = hr.h_strand.resize(nq)) || (rc = hr.h_peak.resize(nq)))
        return rc;
    if (ix->nearest_opt && ((rc = hr.h_nearest.resize(nq)) || (rc = hr.h_ties.resize(nq)))) return rc;  // (rtx_batch_nearest)
    if (ix->identity_opt && ((rc = hr.h_dist.resize(nq)) || (rc = hr.h_qlen.resize(nq)))) return rc;  // (rtx_batch_identity)
    const uint64_t D = ix->fin_D;
    if ((rc = hr.v_row_lineage.grow_keep(rows, keep)) || (rc = hr.v_row_node.grow_keep(rows, keep)) || (rc = hr.v_row_depth.grow_keep(rows, keep)) ||
        (rc = hr.v_row_depth8.grow_keep(rows, keep)) || (rc = hr.v_row_local.grow_keep(rows, keep)) || (rc = hr.v_row_conf.grow_keep(rows * D, keep * D)) ||
        (rc = hr.v_row_hund.grow_keep(rows * D, keep * D)))
        return rc;
    return RTX_OK;
}

// D2H of the final rows [r0, r1) on stream cs (asynchronous): the device laid them out as the view wants them
static int copy_rows(rtx_index *ix, const rtx_index::ResultSet &r, rtx_index::HostRes &hr, uint64_t r0, uint64_t r1, hipStream_t cs) {
    if (r1 <= r0) return RTX_OK;
    const uint64_t n = r1 - r0, D = ix->fin_D;
    RTX_HIP(hipMemcpyAsync(hr.v_row_lineage.data() + r0, r.d_fin_lineage.p + r0, n * 4, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_node.data() + r0, r.d_fin_node.p + r0, n * 4, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_depth.data() + r0, r.d_fin_depth.p + r0, n * 4, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_depth8.data() + r0, r.d_fin_depth8.p + r0, n, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_local.data() + r0, r.d_fin_local.p + r0, n * 8, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_conf.data() + r0 * D, r.d_fin_conf.p + r0 * D, n * D * 8, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_hund.data() + r0 * D, r.d_fin_hund.p + r0 * D, n * D, hipMemcpyDeviceToHost, cs));
    return RTX_OK;
}
// ... and of the per-query fields (input order: complete when the last sub-batch has been finalised)
// Under RTX_OPT_STRAND (r.n_user queries, r.n_q = twice as many on the device) they are those of the chosen orientation, gathered by
// strand_select_kernel; strand and peak come with them either way (rtx_batch_strands).
static int copy_queries(const rtx_index::ResultSet &r, rtx_index::HostRes &hr, hipStream_t cs) {
    const uint64_t nq = r.n_user;
    const bool both = r.n_user != r.n_q;
    hr.n_user = nq;
    hr.both = both;
    if (r.has_peak) RTX_HIP(hipStreamWaitEvent(cs, r.ev_select, 0));
    else if (both) { set_error("internal: a batch of both strands without its selection"); return RTX_ERR_STATE; }
    RTX_HIP(hipMemcpyAsync(hr.h_t.data(), both ? r.d_sel_t.p : r.d_fin_t.p, nq * 4, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.h_status.data(), both ? r.d_sel_status.p : r.d_fin_status.p, nq, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.h_gs.data(), both ? r.d_sel_gs.p : r.d_fin_gs.p, nq * 8, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_begin.data(), both ? r.d_sel_row_begin.p : r.d_fin_row_begin.p, nq * 8, hipMemcpyDeviceToHost, cs));
    RTX_HIP(hipMemcpyAsync(hr.v_row_count.data(), both ? r.d_sel_row_count.p : r.d_fin_row_count.p, nq * 4, hipMemcpyDeviceToHost, cs));
    if (r.has_peak) {
        RTX_HIP(hipMemcpyAsync(hr.h_strand.data(), r.d_strand.p, nq, hipMemcpyDeviceToHost, cs));
        RTX_HIP(hipMemcpyAsync(hr.h_peak.data(), r.d_peak.p, nq * 4, hipMemcpyDeviceToHost, cs));
    } else {  // (a staged run, rtx_debug_evaluate: no peak was taken)
        std::memset(hr.h_strand.data(), 0, nq);
        std::memset(hr.h_peak.data(), 0, nq * 4);
    }
    hr.has_nearest = r.has_peak && r.has_nearest;  // RTX_OPT_NEAREST (rtx_nearest.hip)
    if (hr.has_nearest) {
        if (hr.h_nearest.size() < nq || hr.h_ties.size() < nq) { set_error("internal: RTX_OPT_NEAREST without its host arrays"); return RTX_ERR_STATE; }
        RTX_HIP(hipMemcpyAsync(hr.h_nearest.data(), r.d_nearest.p, nq * 4, hipMemcpyDeviceToHost, cs));
        RTX_HIP(hipMemcpyAsync(hr.h_ties.data(), r.d_ties.p, nq * 4, hipMemcpyDeviceToHost, cs));
    }
    hr.has_identity = hr.has_nearest && r.has_identity;  // RTX_OPT_IDENTITY (rtx_identity.hip, in front of ev_select)
    if (hr.has_identity) {
        if (hr.h_dist.size() < nq || hr.h_qlen.size() < nq) { set_error("internal: RTX_OPT_IDENTITY without its host arrays"); return RTX_ERR_STATE; }
        RTX_HIP(hipMemcpyAsync(hr.h_dist.data(), r.d_dist.p, nq * 4, hipMemcpyDeviceToHost, cs));
        RTX_HIP(hipMemcpyAsync(hr.h_qlen.data(), r.d_qlen.p, nq * 4, hipMemcpyDeviceToHost, cs));
    }
    return RTX_OK;
}
// The flags of a run and the arena cursor of its bulk, once its streams have drained
static int read_flags(const rtx_index::ResultSet &r, uint32_t *flags, unsigned long long *cursor) {
    RTX_HIP(hipMemcpy(flags, r.d_flags.p, 4, hipMemcpyDeviceToHost));
    RTX_HIP(hipMemcpy(cursor, r.d_cursor.p, 8, hipMemcpyDeviceToHost));
    return RTX_OK;
}

// The batch in result set r joins the open taxon profile (rtx_profile.hip), once: called where the text of a download is produced -- the run's
// flags have been accepted, its final rows, its selection and its exact-match groups are complete on the device, and the next run has not
// been let onto these rows.  A staged run and rtx_debug_evaluate (no peak, no selection) add nothing.  Synchronous like the text, and for
// the same reason: the input set with the ids a caller passed in is free for the next rtx_batch_prefetch when the download returns.
int enqueue_profile(rtx_index *ix, rtx_index::ResultSet &r) {
    rtx_index::Profile &pf = ix->prof;
    if (!pf.on || r.profiled || !r.has_peak) return RTX_OK;
    const rtx_index::Inputs &in = ix->in[r.in_set];
    const bool both = r.n_user != r.n_q;
    ProfileParams p{};
    p.src = ProfileSrc{both ? r.d_sel_status.p : r.d_fin_status.p, both ? r.d_sel_row_count.p : r.d_fin_row_count.p,
                       both ? r.d_sel_row_begin.p : r.d_fin_row_begin.p, r.d_fin_node.p, r.d_fin_depth8.p, r.d_fin_hund.p, ix->fin_D,
                       pf.d_parent.p, ix->d_node_depth.p, pf.d_ref_leaf.p, ix->nodes.size(), (uint32_t)ix->n_total};
    p.n_pos = r.n_q;
    p.n_user = (uint32_t)r.n_user;
    p.perm = r.d_perm.p;
    p.strand = both ? r.d_strand.p : nullptr;
    p.exact = ExactRef{in.d_exact_ids.p, in.d_exact_off.p, r.dev_exact ? r.d_exact_grp.p : nullptr, ix->d_em_goff.p, ix->d_em_gids.p};
    p.override_ok = !(pf.flags & (RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE));
    p.cutoff = pf.cutoff;
    p.weight = in.has_weights && in.n_weights == r.n_user ? in.d_weights.p : nullptr;
    p.n_nodes = ix->nodes.size();
    p.clade = pf.d_acc.p;
    p.direct = p.clade + p.n_nodes;
    p.conf_sum = p.direct + p.n_nodes;
    p.totals = p.conf_sum + p.n_nodes;
    if (r.d_perm.n < r.n_q || !p.src.status || !p.src.row_begin) { set_error("internal: a profile over a batch without its arrays"); return RTX_ERR_STATE; }
    hipStream_t s = ix->copy_stream ? ix->copy_stream : ix->stream;
    if (both) RTX_HIP(hipStreamWaitEvent(s, r.ev_select, 0));
    const bool timed = ix->stage_timing != 0u;
    if (timed) {
        for (auto &e : pf.ev)
            if (!e) RTX_HIP(hipEventCreate(&e));
        RTX_HIP(hipEventRecord(pf.ev[0], s));
    }
    launch_profile(s, p);
    RTX_HIP(hipGetLastError());
    if (pf.n_samples && in.has_samples && in.n_samples == r.n_user) {  // the per-sample counters beside it (nothing staged: the batch counts in no sample)
        SampleProfileParams sp{};
        sp.p = p;
        sp.sample = in.d_samples.p;
        sp.n_samples = pf.n_samples;
        sp.direct = pf.d_by_sample.p;
        sp.totals = sp.direct + (size_t)pf.n_samples * p.n_nodes;
        launch_profile_samples(s, sp);
        RTX_HIP(hipGetLastError());
    }
    if (timed) RTX_HIP(hipEventRecord(pf.ev[1], s));
    RTX_HIP(hipStreamSynchronize(s));
    if (timed) {
        float ms = 0.f;
        RTX_HIP(hipEventElapsedTime(&ms, pf.ev[0], pf.ev[1]));
        pf.ms += ms;
        pf.launches++;
    }
    r.profiled = true;
    return RTX_OK;
}

// Streamed download: while later sub-batches are still running, the records of every finished one are copied
// (copy_stream) and finalised on the calling thread, so that only the last sub-batch is left once the device is
// done.  *done = false: not applicable (batch already complete: the bulk path with its threads is faster) or the
// arena overflowed (the bulk path repeats the run).
// the exact matches the device found belong to the download (same alternation as the result sets)
static int fetch_exact_groups(rtx_index *ix, const rtx_index::ResultSet &r) {
    rtx_index::HostExact &hx = ix->host_exact[ix->res_set];
    hx.valid = hx.csr_valid = false;
    if (r.dev_exact) {
        hx.grp.resize(r.n_q);
        if (r.ev_exact) RTX_HIP(hipEventSynchronize(r.ev_exact));  // the lookup ran at the head of the batch (a re-run: of the re-run)
        RTX_HIP(hipMemcpy(hx.grp.data(), r.d_exact_grp.p, r.n_q * 4, hipMemcpyDeviceToHost));
        hx.valid = true;
    }
    return RTX_OK;
}

// rtx_batch_download_then_run: the staged batch becomes the current one and is enqueued -- called when the last records of the batch
// being downloaded have left the device, while its last sub-batch is still to be finalised on the host
static int run_staged(rtx_index *ix, uint32_t flags, bool *ran_next) {
    *ran_next = false;
    if (!ix->in[ix->cur_in ^ 1u].staged) return RTX_OK;
    int rc = rtx_batch_activate(ix);
    if (!rc) rc = rtx_batch_run(ix, flags);
    *ran_next = rc == RTX_OK;
    return rc;
}

// What a run asked for that it did not have (its flags; the arena cursor it reached): more rows of counts, longer record segments, a larger
// arena with its final arrays in its result set r.  The caller repeats the (deterministic) run.
static int grow_for_flags(rtx_index *ix, rtx_index::ResultSet &r, uint32_t flags, unsigned long long cursor) {
    int rc;
    if (flags & 4u) {  // more queries took the dense epilogues than the counts buffer had rows (HitParams::cnt_row): twice the rows
        if (ix->diet_shift == 0u) { set_error("the counts buffer ran out of rows without being on its diet (internal error)"); return RTX_ERR_HIP; }
        ix->diet_shift--;
    }
    if (flags & 8u) {  // a query left a tile more records than a segment holds (RecordRef::seg_len): twice the length
        if (ix->rec_seg_len >= 8192u) { set_error("a record segment of a whole tile overflowed (internal error)"); return RTX_ERR_HIP; }
        ix->rec_seg_len *= 2u;
    }
    if ((flags & 12u) && !(flags & 1u)) return RTX_OK;
    // arena too small: grow to what this run asked for
    // (+ what the sub-allocators of the walk may leave unused on top of this run's share: their holes differ from run to run, and an
    // arena cut to this run's cursor overflowed again on every other step of the same batch -- 3.3 instead of 4.5 M queries/s on real barcodes)
    // and at least half as much again as the arena that overflowed: walks that find their sub-allocator's piece used up at the
    // same moment each take a fresh one, so the holes of a launch are not bounded by the number of sub-allocators
    const uint64_t want = std::max<uint64_t>(cursor + 4096 + (uint64_t)(r.n_sub ? r.n_sub : 1u) * kWalkSubAllocs * kWalkChunkRows,
                                             r.arena_cap + r.arena_cap / 2) + (r.arena_cap - r.side_base);  // (+ the side classes' region)
    if ((rc = r.d_arena.alloc(want))) return rc;
    r.arena_cap = want;
    return alloc_final(ix, r, r.n_q);  // (the final arrays hold as many rows as the arena)
}

// RTX_OPT_RUN_AHEAD: the staged batch is enqueued while the batch being downloaded is still on the device, into the other result set; its
// first front half starts behind this batch's last FRONT half (the handle's stream), its scratch sets wait for the back halves that last used
// them (enqueue_batch).  A failure leaves the handle writing the set it wrote before.
static int run_ahead(rtx_index *ix, uint32_t flags) {
    const uint64_t arena_cap = ix->res().arena_cap;
    ix->rs_w ^= 1u;
    // (an arena as large as the other set's has grown: this batch will need it as well, and would find out by an abandoned run-ahead)
    int rc = alloc_result_set(ix, ix->res(), ix->in[ix->cur_in ^ 1u].n_q, arena_cap);
    ix->hold_join = true;
    bool ran = false;
    if (!rc) rc = run_staged(ix, flags, &ran);
    ix->hold_join = false;
    if (rc) ix->rs_w ^= 1u;
    else ix->n_run_ahead++;
    return rc;
}

// Streamed download of the batch in result set r.  Under RTX_OPT_RUN_AHEAD (`ahead` below) the staged batch is enqueued FIRST (run_ahead,
// into the other set): two batches are then on the device, and the host has a whole batch's time to come back with the one after.  An
// overflow of this batch found now -- with the next one on the device already -- ends in RTX_RETRY_CHUNK: both streams drained, r grown and
// the set the handle writes again, no batch on the handle; the caller runs this chunk again and stages the next one anew (host_raxtax.cpp).
// Happens while a handle's buffers find their size (its first chunks), not in steady state.
static int download_streamed(rtx_index *ix, rtx_index::ResultSet &r, rtx_index::HostRes &hr, bool *done, uint64_t *nrows_out, bool then_run,
                             uint32_t next_flags, bool *ran_next) {
    *done = false;
    const uint32_t n_sub = r.n_sub;
    const uint32_t n_side = r.n_side;  // the side classes' sub-batches come first in the plan (and on the stream of the back halves): they are waited for LAST, their rows left with the first range
    if (!r.stream_dl || n_sub < 2) return RTX_OK;
    const bool ahead = then_run && ix->run_ahead_opt != 0u && ix->join_pending && n_side == 0 && ix->in[ix->cur_in ^ 1u].staged;
    // (a batch that is complete already takes the bulk path -- unless the next one is about to be enqueued ahead: the device comes first)
    if (!ahead && hipEventQuery(r.ev_sub[n_sub - 1]) == hipSuccess && hipEventQuery(r.ev_sub[0]) == hipSuccess) return RTX_OK;
    const uint64_t nq = r.n_q;
    int rc = size_host_results(ix, hr, nq, nq + nq / 4 + 64, 0);
    if (rc) return rc;
    if ((rc = fetch_exact_groups(ix, r))) return rc;  // (now, beside the kernels: 4 MB per 1 M queries that used to cross at the tail, with the device idle)
    if (ahead) {
        if ((rc = run_ahead(ix, next_flags))) return rc;
        *ran_next = true;
    }
    uint64_t prev = 0;
    uint32_t redo = 0;  // what sends this batch round again (bits of d_flags)
    for (uint32_t k = 0; k < n_sub && !redo; k++) {
        const uint32_t sb = k + n_side < n_sub ? k + n_side : k + n_side - n_sub;
        RTX_HIP(hipEventSynchronize(r.ev_sub[sb]));
        const bool side = sb < n_side;  // its rows lie in the side region of the arena, behind its own cursor
        if (r.h_cursor_sub[sb] > (side ? r.arena_cap : r.side_base)) { redo = 1u; break; }  // arena overflow
        const uint64_t cur = r.h_fin_sub[sb];  // final rows [prev, cur): this sub-batch's (the finalise launches follow one another)
        if (cur > r.fin_cap) { redo = 1u; break; }
        // (cur <= prev: a side class that ran in front of the bulk on the one stream -- its rows left with the first range)
        if (cur > std::min<uint64_t>({hr.v_row_lineage.cap, hr.v_row_depth8.cap, hr.v_row_local.cap, hr.v_row_conf.cap / ix->fin_D, hr.v_row_hund.cap / ix->fin_D}))
            RTX_HIP(hipStreamSynchronize(ix->copy_stream));  // an array is about to move: the copies into it have to have landed
        if (cur > prev && ((rc = size_host_results(ix, hr, nq, cur, prev)) || (rc = copy_rows(ix, r, hr, prev, cur, ix->copy_stream)))) return rc;
        prev = std::max(prev, cur);
        if (k + 1 == n_sub) {  // the last records leave the device
            if ((rc = copy_queries(r, hr, ix->copy_stream))) return rc;
            RTX_HIP(hipStreamSynchronize(ix->copy_stream));
            if (!ahead) {
                if ((rc = settle_join(ix))) return rc;
                RTX_HIP(hipStreamSynchronize(ix->stream));
            }
            // the run's flags have arrived (copied behind its last kernel -- under RTX_OPT_RUN_AHEAD on the stream of the back halves, which the
            // handle's stream joins in FRONT of that copy: the event behind the copy is what says so)
            if (r.ev_flags) RTX_HIP(hipEventSynchronize(r.ev_flags));
            uint32_t flags = r.h_flags.size() ? r.h_flags[0] : 0u;  // (copied behind the run's last kernel: enqueue_batch)
            if (ahead && ix->run_ahead_opt == 2u && (ix->n_run_ahead & 1u)) flags |= 1u;  // (test aid: as if the arena had overflowed)
            if (flags & 12u) { redo = flags & 13u; break; }  // the rows of the counts buffer ran out, or a record segment was too short (whatever else such a run flagged)
            if (flags & 2u) { set_error("lineage walk exceeded its row/depth bounds (internal error)"); return RTX_ERR_HIP; }
            if (flags & 1u) { redo = 1u; break; }  // arena overflow
            if ((rc = enqueue_text(ix, r))) return rc;  // the text (rtx_text.hip)
            if ((rc = enqueue_profile(ix, r))) return rc;  // ... and the taxon profile (rtx_profile.hip)
            if (!ahead && then_run && (rc = run_staged(ix, next_flags, ran_next))) return rc;  // the device is free for the next batch
        }
    }
    if (redo && !ahead) return RTX_OK;  // the bulk path repeats the run
    if (redo) {  // this batch has to run again, and the next one is on the device: drain, grow, hand both back to the caller
        RTX_HIP(hipStreamSynchronize(ix->copy_stream));
        RTX_HIP(hipStreamSynchronize(ix->stream));
        if (ix->stream2) RTX_HIP(hipStreamSynchronize(ix->stream2));
        uint32_t flags = 0;
        unsigned long long cursor = 0;
        if ((rc = read_flags(r, &flags, &cursor))) return rc;
        ix->rs_w = (uint32_t)(&r - ix->rs);  // this batch's set is the one that grows, and the one its repeated run writes
        if ((rc = grow_for_flags(ix, r, (flags & 13u) | redo, cursor))) return rc;
        ix->join_pending = false;
        ix->uploaded = ix->ran = false;
        ix->synced = true;
        ix->in[0].staged = ix->in[1].staged = false;
        ix->ws_valid = false;
        ix->res_set ^= 1u;  // (the repeated download takes this host set again: the other one holds the view of the chunk before)
        ix->n_run_ahead_retry++;
        *ran_next = false;
        return RTX_RETRY_CHUNK;
    }
    if (!*ran_next) ix->synced = true;  // (else: the next batch is running)
    *nrows_out = prev;
    *done = true;
    return RTX_OK;
}


}  // namespace rtxi

extern "C" {

static int download_impl(rtx_index *ix, rtx_result_view *out, bool then_run, uint32_t next_flags) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!ix->ran || !out) { set_error("rtx_batch_download before rtx_batch_run"); return RTX_ERR_STATE; }
    rtx_index::ResultSet &r = ix->res();  // the batch that ran last (a run-ahead below moves the handle on to the other set)
    const uint64_t nq = r.n_q, n_user = r.n_user;  // (read now: a batch that this call enqueues behind the download records itself in the same set)
    ix->res_set ^= 1u;
    rtx_index::HostRes &hr = ix->host_res[ix->res_set];
    ix->host_text[ix->res_set].valid = false;
    bool streamed = false, ran_next = false;
    uint64_t nrows = 0;
    if ((rc = download_streamed(ix, r, hr, &streamed, &nrows, then_run, next_flags, &ran_next))) return rc;
    if (!streamed) {  // (nothing ran ahead: the handle still writes r -- a repeated run included)
        // (a streamed download that gave up half way -- an overflow: the run is repeated -- may have copies in flight into this result set)
        if (ix->copy_stream) RTX_HIP(hipStreamSynchronize(ix->copy_stream));
        for (int attempt = 0;; attempt++) {
            if ((rc = settle_join(ix))) return rc;
            RTX_HIP(hipStreamSynchronize(ix->stream));
            ix->synced = true;
            uint32_t flags = 0;
            unsigned long long cursor = 0;
            if ((rc = read_flags(r, &flags, &cursor))) return rc;
            if ((flags & 2u) && !(flags & 12u)) { set_error("lineage walk exceeded its row/depth bounds (internal error)"); return RTX_ERR_HIP; }
            if (!(flags & 13u)) break;
            if (attempt >= 8) { set_error("result arena / counts rows overflow persists"); return RTX_ERR_HIP; }
            if ((rc = grow_for_flags(ix, r, flags, cursor))) return rc;
            if ((flags & 12u) && !(flags & 1u)) {
                if ((rc = enqueue_batch(ix, ix->last_flags))) return rc;
                continue;
            }
            if (ix->n_refs != ix->n_total) {  // a sharded run is driven by the caller: ask it to repeat
                set_error("result arena overflow: repeat the sharded run (the arena has been enlarged)");
                return RTX_ERR_STATE;
            }
            if ((rc = enqueue_batch(ix, ix->last_flags))) return rc;
        }
        unsigned long long fin = 0;
        RTX_HIP(hipMemcpy(&fin, r.d_fin_cursor.p, 8, hipMemcpyDeviceToHost));
        if (fin > r.fin_cap) { set_error("final result arrays overflowed without a flag (internal error)"); return RTX_ERR_HIP; }
        if ((rc = size_host_results(ix, hr, nq, fin, 0)) || (rc = copy_rows(ix, r, hr, 0, fin, ix->stream)) || (rc = copy_queries(r, hr, ix->stream))) return rc;
        RTX_HIP(hipStreamSynchronize(ix->stream));
        nrows = fin;
        if ((rc = enqueue_text(ix, r))) return rc;  // (before run_staged: the next batch writes these rows)
        if ((rc = enqueue_profile(ix, r))) return rc;
    }
    {   // the first download of a handle: the other result set (the two alternate, a view stays valid until the second-next
        // download) is allocated now, so that the second batch does not pay for its page-locked allocations
        rtx_index::HostRes &other = ix->host_res[ix->res_set ^ 1u];
        if (other.h_t.empty() && other.v_row_lineage.empty() && (rc = size_host_results(ix, other, nq, hr.v_row_lineage.size(), 0))) return rc;
    }
    if (!streamed) {  // (the streamed path has fetched them before it let the next batch onto the device)
        if ((rc = fetch_exact_groups(ix, r))) return rc;
        if (then_run && (rc = run_staged(ix, next_flags, &ran_next))) return rc;
    }
    out->n_queries = (uint32_t)n_user;  // (under RTX_OPT_STRAND: the caller's queries, each with the fields of its chosen orientation)
    out->n_rows = nrows;               // the length of the row arrays: the rows of the orientation that lost stay in them, unreferenced
    out->t = hr.h_t.data();
    out->status = hr.h_status.data();
    out->global_signal = hr.h_gs.data();
    out->row_begin = reinterpret_cast<const uint64_t *>(hr.v_row_begin.data());
    out->row_count = hr.v_row_count.data();
    out->row_lineage = hr.v_row_lineage.data();
    out->row_node = hr.v_row_node.data();
    out->row_depth = hr.v_row_depth.data();
    out->row_conf = hr.v_row_conf.data();
    out->row_local_signal = hr.v_row_local.data();
    out->row_conf_stride = ix->fin_D;
    out->row_depth_u8 = hr.v_row_depth8.data();
    out->row_conf_hundredths = hr.v_row_hund.data();
    return RTX_OK;
}

int rtx_batch_download(rtx_index *ix, rtx_result_view *out) { return download_impl(ix, out, false, 0); }

// Download of the current batch; as soon as its last records have left the device the STAGED batch (rtx_batch_prefetch) is activated and
// run with `flags` -- the host finalises the last sub-batch of this batch while the device already classifies the next one.  Without a
// staged batch: rtx_batch_download.
int rtx_batch_download_then_run(rtx_index *ix, rtx_result_view *out, uint32_t flags) { return download_impl(ix, out, true, flags); }

int rtx_index_has_exact_lookup(const rtx_index *index) { return index && index->d_em_table.p && index->dev_exact_opt ? 1 : 0; }

// Tree.sequences.get(query) for every query of the last download, as the device found it: CSR over the queries
int rtx_batch_exact_matches(rtx_index *ix, const uint64_t **exact_off, const uint32_t **exact_ids) {
    if (!ix || !exact_off || !exact_ids) { set_error("null argument"); return RTX_ERR_INVALID; }
    rtx_index::HostExact &hx = ix->host_exact[ix->res_set];
    const rtx_index::HostRes &hres = ix->host_res[ix->res_set];
    if (!hx.valid) { set_error("rtx_batch_exact_matches: the last download has no device lookup (ids were passed in, or no table)"); return RTX_ERR_STATE; }
    if (!hx.csr_valid) {
        // under RTX_OPT_STRAND the groups hold the twins' as well: a query reports those of its chosen orientation
        const bool both = hres.both && hx.grp.size() == 2 * hres.n_user;
        const size_t nq = both ? hres.n_user : hx.grp.size();
        auto group = [&](size_t q) { return hx.grp[both && hres.h_strand[q] ? q + nq : q]; };
        hx.off.assign(nq + 1, 0);
        for (size_t q = 0; q < nq; q++) {
            const uint32_t g = group(q);
            hx.off[q + 1] = hx.off[q] + (g == 0xFFFFFFFFu ? 0u : ix->h_em_goff[g + 1] - ix->h_em_goff[g]);
        }
        hx.ids.resize(hx.off[nq] + 1);
        for (size_t q = 0; q < nq; q++) {
            const uint32_t g = group(q);
            if (g != 0xFFFFFFFFu) std::copy(ix->h_em_gids.begin() + ix->h_em_goff[g], ix->h_em_gids.begin() + ix->h_em_goff[g + 1], hx.ids.begin() + hx.off[q]);
        }
        hx.csr_valid = true;
    }
    *exact_off = hx.off.data();
    *exact_ids = hx.ids.data();
    return RTX_OK;
}

// Strand (0 plus, 1 minus) and peak of every query of the last download (rtx_strand.hip)
int rtx_batch_strands(rtx_index *ix, const uint8_t **strand, const uint32_t **peak) {
    if (!ix || (!strand && !peak)) { set_error("rtx_batch_strands: null argument"); return RTX_ERR_INVALID; }
    const rtx_index::HostRes &hr = ix->host_res[ix->res_set];
    if (hr.h_strand.empty() || hr.h_peak.empty() || hr.h_strand.size() < hr.n_user) { set_error("rtx_batch_strands before a download"); return RTX_ERR_STATE; }
    if (strand) *strand = hr.h_strand.data();
    if (peak) *peak = hr.h_peak.data();
    return RTX_OK;
}

// Nearest reference and ties of every query of the last download (rtx_nearest.hip)
int rtx_batch_nearest(rtx_index *ix, const uint32_t **nearest, const uint32_t **ties) {
    if (!ix || (!nearest && !ties)) { set_error("rtx_batch_nearest: null argument"); return RTX_ERR_INVALID; }
    const rtx_index::HostRes &hr = ix->host_res[ix->res_set];
    if (!hr.has_nearest || hr.h_nearest.size() < hr.n_user || hr.h_ties.size() < hr.n_user) { set_error("rtx_batch_nearest: the last download's run had RTX_OPT_NEAREST off (or there was no download)"); return RTX_ERR_STATE; }
    if (nearest) *nearest = hr.h_nearest.data();
    if (ties) *ties = hr.h_ties.data();
    return RTX_OK;
}

// ---- the taxon profile of the handle (rtx_profile.hip): open between begin and end; every accepted download adds its batch once
// n_samples != 0: with the per-sample counters (rtx_index_profile_begin_samples)
static int profile_begin(rtx_index *ix, uint32_t cutoff_hundredths, uint32_t flags, uint32_t n_samples) {
    int rc = bind(ix);
    if (rc) return rc;
    rtx_index::Profile &pf = ix->prof;
    if (cutoff_hundredths < 1u || cutoff_hundredths > 100u) { set_error("rtx_index_profile_begin: the cutoff is %u hundredths, not 1 .. 100", cutoff_hundredths); return RTX_ERR_INVALID; }
    if (flags & ~(RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE)) { set_error("rtx_index_profile_begin: unknown flags %#x", flags); return RTX_ERR_INVALID; }
    if (ix->n_refs != ix->n_total) { set_error("rtx_index_profile_begin: not on a reference-shard handle (its downloads hold no whole result)"); return RTX_ERR_INVALID; }
    if (pf.on) { set_error("rtx_index_profile_begin: a profile is open already (rtx_index_profile_end)"); return RTX_ERR_STATE; }
    const FlatNodes &f = ix->nodes;
    const uint32_t nn = f.size();
    if ((uint64_t)n_samples * nn > RTX_PROFILE_MAX_SAMPLE_COUNTERS) {
        set_error("rtx_index_profile_begin_samples: %u samples x %u nodes are more than RTX_PROFILE_MAX_SAMPLE_COUNTERS = %llu counters", n_samples, nn,
                  (unsigned long long)RTX_PROFILE_MAX_SAMPLE_COUNTERS);
        return RTX_ERR_INVALID;
    }
    const size_t by_sample = (size_t)n_samples * ((size_t)nn + 4u);
    // the Taxon node of every reference: the nodes come breadth first, so the deepest Taxon node over a reference is the last one written
    std::vector<uint32_t> leaf(ix->n_total ? ix->n_total : 1u, kNoNode);
    for (uint32_t v = 0; v < nn; v++)
        if (f.type[v] == kTaxon) std::fill(leaf.begin() + f.begin[v], leaf.begin() + f.end[v], v);
    if ((rc = pf.d_parent.alloc(nn)) || (rc = pf.d_ref_leaf.alloc(leaf.size())) || (rc = pf.d_acc.alloc(3u * (size_t)nn + 4u)) ||
        (by_sample && (rc = pf.d_by_sample.alloc(by_sample)))) {
        pf.d_parent.release(); pf.d_ref_leaf.release(); pf.d_acc.release(); pf.d_by_sample.release();
        return rc;
    }
    if (by_sample) RTX_HIP(hipMemset(pf.d_by_sample.p, 0, by_sample * 8));
    pf.n_samples = n_samples;
    RTX_HIP(hipMemcpy(pf.d_parent.p, f.parent.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
    RTX_HIP(hipMemcpy(pf.d_ref_leaf.p, leaf.data(), leaf.size() * 4, hipMemcpyHostToDevice));
    RTX_HIP(hipMemset(pf.d_acc.p, 0, (3u * (size_t)nn + 4u) * 8));
    pf.cutoff = cutoff_hundredths;
    pf.flags = flags;
    pf.ms = 0.f;
    pf.launches = 0;
    pf.on = true;
    return RTX_OK;
}

int rtx_index_profile_begin(rtx_index *ix, uint32_t cutoff_hundredths, uint32_t flags) { return profile_begin(ix, cutoff_hundredths, flags, 0u); }

int rtx_index_profile_begin_samples(rtx_index *ix, uint32_t cutoff_hundredths, uint32_t flags, uint32_t n_samples) {
    if (n_samples == 0) { set_error("rtx_index_profile_begin_samples: no samples"); return RTX_ERR_INVALID; }
    return profile_begin(ix, cutoff_hundredths, flags, n_samples);
}

int rtx_index_profile_read_samples(rtx_index *ix, rtx_sample_profile_view *out) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!out) { set_error("rtx_index_profile_read_samples: null argument"); return RTX_ERR_INVALID; }
    rtx_index::Profile &pf = ix->prof;
    if (!pf.on || !pf.n_samples) { set_error("rtx_index_profile_read_samples: no profile with samples is open (rtx_index_profile_begin_samples)"); return RTX_ERR_STATE; }
    const uint32_t nn = ix->nodes.size();
    pf.h_by_sample.resize((size_t)pf.n_samples * ((size_t)nn + 4u));
    RTX_HIP(hipMemcpy(pf.h_by_sample.data(), pf.d_by_sample.p, pf.h_by_sample.size() * 8, hipMemcpyDeviceToHost));
    out->n_nodes = nn;
    out->n_samples = pf.n_samples;
    out->cutoff_hundredths = pf.cutoff;
    out->flags = pf.flags;
    out->direct = pf.h_by_sample.data();
    out->totals = out->direct + (size_t)pf.n_samples * nn;
    return RTX_OK;
}

int rtx_index_profile_read(rtx_index *ix, rtx_profile_view *out) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!out) { set_error("rtx_index_profile_read: null argument"); return RTX_ERR_INVALID; }
    rtx_index::Profile &pf = ix->prof;
    if (!pf.on) { set_error("rtx_index_profile_read: no profile is open (rtx_index_profile_begin)"); return RTX_ERR_STATE; }
    const uint32_t nn = ix->nodes.size();
    pf.h_acc.resize(3u * (size_t)nn + 4u);
    // (every download has waited for its own kernel: what has been downloaded is in the counters)
    RTX_HIP(hipMemcpy(pf.h_acc.data(), pf.d_acc.p, pf.h_acc.size() * 8, hipMemcpyDeviceToHost));
    out->n_nodes = nn;
    out->cutoff_hundredths = pf.cutoff;
    out->flags = pf.flags;
    out->clade = pf.h_acc.data();
    out->direct = out->clade + nn;
    out->conf_sum = out->direct + nn;
    for (int i = 0; i < 4; i++) out->totals[i] = pf.h_acc[3u * (size_t)nn + i];
    return RTX_OK;
}

int rtx_index_profile_reset(rtx_index *ix) {
    int rc = bind(ix);
    if (rc) return rc;
    rtx_index::Profile &pf = ix->prof;
    if (!pf.on) { set_error("rtx_index_profile_reset: no profile is open"); return RTX_ERR_STATE; }
    RTX_HIP(hipMemset(pf.d_acc.p, 0, (3u * (size_t)ix->nodes.size() + 4u) * 8));
    if (pf.n_samples) RTX_HIP(hipMemset(pf.d_by_sample.p, 0, (size_t)pf.n_samples * ((size_t)ix->nodes.size() + 4u) * 8));
    pf.ms = 0.f;
    pf.launches = 0;
    return RTX_OK;
}

int rtx_index_profile_end(rtx_index *ix) {
    int rc = bind(ix);
    if (rc) return rc;
    rtx_index::Profile &pf = ix->prof;
    if (!pf.on) { set_error("rtx_index_profile_end: no profile is open"); return RTX_ERR_STATE; }
    pf.on = false;
    pf.d_acc.release(); pf.d_parent.release(); pf.d_ref_leaf.release(); pf.d_by_sample.release();
    pf.n_samples = 0;
    std::vector<uint64_t>().swap(pf.h_acc);
    std::vector<uint64_t>().swap(pf.h_by_sample);
    for (auto &e : pf.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    return RTX_OK;
}

// Milliseconds profile_kernel took and its launches since begin or reset (RTX_OPT_STAGE_TIMING on at the downloads; else 0 and 0)
int rtx_index_profile_time(rtx_index *ix, float *ms, uint32_t *launches) {
    if (!ix || (!ms && !launches)) { set_error("rtx_index_profile_time: null argument"); return RTX_ERR_INVALID; }
    if (!ix->prof.on) { set_error("rtx_index_profile_time: no profile is open"); return RTX_ERR_STATE; }
    if (ms) *ms = ix->prof.ms;
    if (launches) *launches = ix->prof.launches;
    return RTX_OK;
}

// One weight per query for the batch that the NEXT rtx_batch_prefetch / rtx_batch_upload stages: how many reads the query stands for in the
// open profile (the host mirror under RTX_OPT_DEREP: the copies of a distinct read).  The path of rtx_batch_prefetch_labels: the input set
// beside the current one, asynchronous H2D on the transfer stream, taken or dropped at that prefetch (a count that does not match: dropped).
int rtx_batch_prefetch_weights(rtx_index *ix, uint64_t n_queries, const uint32_t *weights) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!weights && n_queries) { set_error("rtx_batch_prefetch_weights: null weights"); return RTX_ERR_INVALID; }
    rtx_index::Inputs &in = ix->in[ix->cur_in ^ 1u];
    if (!ix->h2d_stream) RTX_HIP(hipStreamCreateWithFlags(&ix->h2d_stream, hipStreamNonBlocking));
    if (!in.ready) RTX_HIP(hipEventCreateWithFlags(&in.ready, hipEventDisableTiming));
    if (in.recorded) RTX_HIP(hipEventSynchronize(in.ready));  // the last transfer out of this set's pinned buffers
    if (ix->ev_activated) RTX_HIP(hipStreamWaitEvent(ix->h2d_stream, ix->ev_activated, 0));
    if ((rc = in.h_weights.resize(n_queries + 1)) || (rc = in.d_weights.alloc(n_queries + 1))) return rc;
    if (n_queries) std::memcpy(in.h_weights.data(), weights, n_queries * 4);
    if (n_queries) RTX_HIP(hipMemcpyAsync(in.d_weights.p, in.h_weights.data(), n_queries * 4, hipMemcpyHostToDevice, ix->h2d_stream));
    RTX_HIP(hipEventRecord(in.ready, ix->h2d_stream));
    in.recorded = true;
    in.weights_pending = true;
    in.n_weights = n_queries;
    return RTX_OK;
}

// One sample per query for the batch that the NEXT rtx_batch_prefetch / rtx_batch_upload stages, for the per-sample counters of the open
// profile (rtx_index_profile_begin_samples): the path and the rules of the weights above.
int rtx_batch_prefetch_samples(rtx_index *ix, uint64_t n_queries, const uint32_t *sample) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!sample && n_queries) { set_error("rtx_batch_prefetch_samples: null samples"); return RTX_ERR_INVALID; }
    const uint32_t n_samples = ix->prof.on ? ix->prof.n_samples : 0u;
    if (!n_samples) { set_error("rtx_batch_prefetch_samples: no profile with samples is open (rtx_index_profile_begin_samples)"); return RTX_ERR_STATE; }
    for (uint64_t q = 0; q < n_queries; q++)
        if (sample[q] != RTX_DEMUX_NONE && sample[q] >= n_samples) {
            set_error("rtx_batch_prefetch_samples: query %llu has sample %u of %u", (unsigned long long)q, sample[q], n_samples);
            return RTX_ERR_INVALID;
        }
    rtx_index::Inputs &in = ix->in[ix->cur_in ^ 1u];
    if (!ix->h2d_stream) RTX_HIP(hipStreamCreateWithFlags(&ix->h2d_stream, hipStreamNonBlocking));
    if (!in.ready) RTX_HIP(hipEventCreateWithFlags(&in.ready, hipEventDisableTiming));
    if (in.recorded) RTX_HIP(hipEventSynchronize(in.ready));  // the last transfer out of this set's pinned buffers
    if (ix->ev_activated) RTX_HIP(hipStreamWaitEvent(ix->h2d_stream, ix->ev_activated, 0));
    if ((rc = in.h_samples.resize(n_queries + 1)) || (rc = in.d_samples.alloc(n_queries + 1))) return rc;
    if (n_queries) std::memcpy(in.h_samples.data(), sample, n_queries * 4);
    if (n_queries) RTX_HIP(hipMemcpyAsync(in.d_samples.p, in.h_samples.data(), n_queries * 4, hipMemcpyHostToDevice, ix->h2d_stream));
    RTX_HIP(hipEventRecord(in.ready, ix->h2d_stream));
    in.recorded = true;
    in.samples_pending = true;
    in.n_samples = n_queries;
    return RTX_OK;
}

// Distance to the nearest reference and length of every query of the last download (rtx_identity.hip)
int rtx_batch_identity(rtx_index *ix, const uint32_t **dist, const uint32_t **qlen) {
    if (!ix || (!dist && !qlen)) { set_error("rtx_batch_identity: null argument"); return RTX_ERR_INVALID; }
    const rtx_index::HostRes &hr = ix->host_res[ix->res_set];
    if (!hr.has_identity || hr.h_dist.size() < hr.n_user || hr.h_qlen.size() < hr.n_user) { set_error("rtx_batch_identity: the last download's run had RTX_OPT_IDENTITY off (or there was no download)"); return RTX_ERR_STATE; }
    if (dist) *dist = hr.h_dist.data();
    if (qlen) *qlen = hr.h_qlen.data();
    return RTX_OK;
}

int rtx_classify_batch(rtx_index *index, uint64_t n_queries, const uint8_t *bases, const uint64_t *base_off,
                       const uint32_t *exact_ids, const uint64_t *exact_off, uint32_t flags, rtx_result_view *out) {
    int rc = rtx_batch_upload(index, n_queries, bases, base_off, exact_ids, exact_off);
    if (rc) return rc;
    if ((rc = rtx_batch_run(index, flags))) return rc;
    return rtx_batch_download(index, out);
}

}  // extern "C"

// The read front of the host mirror: see host_front.hpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (host_screen.hpp -> rtx_math.hpp: __forceinline__)
#endif
#include "host_front.hpp"
#include "host_screen.hpp"

#include <chrono>
#include <cstring>
#include <tuple>
#include <utility>

namespace rtx_front {

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The sample of every read of the chunk, on the device (a stream of its own beside the handle's); then the reads without their tags, a
// read that is not assigned empty.
int run_demux(rtx_demux *stage, FrontChunk &fc, BufPool &pool, FrontTotals &tot) {
    const double t0 = now();
    const uint64_t nq = fc.given.n;
    for (auto *v : {&fc.dx_sample, &fc.dx_lo, &fc.dx_hi, &fc.dx_hit, &fc.dx_info}) v->resize(nq);
    int rc = rtx_demux_run(stage, nq, fc.given.bases, fc.given.off, fc.dx_sample.data(), fc.dx_lo.data(), fc.dx_hi.data(), fc.dx_hit.data(), fc.dx_info.data());
    if (rc) return rc;
    std::vector<uint32_t> keep_hi(nq);
    auto x = tot.demux;  // (counted in locals: the loop runs per read)
    for (uint64_t i = 0; i < nq; i++) {
        const uint32_t v = fc.dx_info[i] & 0xFFu;
        keep_hi[i] = v == RTX_DEMUX_OK ? fc.dx_hi[i] : fc.dx_lo[i];
        x.assigned += v == RTX_DEMUX_OK;
        if (v < 5u) x.reasons[v]++;
    }
    tot.demux = x;
    rc = cut(fc.given, fc.dx_lo.data(), keep_hi.data(), fc.given.quals != nullptr, fc.x, pool, "no memory for the demultiplexed reads of a chunk", fc.in);
    if (rc) return rc;
    fc.src = fc.dev = fc.in;
    tot.demux.queries += nq;
    tot.demux.busy += now() - t0;
    return RTX_OK;
}

// The primers of the chunk's reads, then the quality of the ranges they left, then the contaminants among what is still kept, on the device
// (streams of their own beside the handle's); then all three in one cut, a discarded read or a contaminant empty.
int run_trim_qual_screen(rtx_trim *trim, rtx_qual *qual, rtx_screen *screen, FrontChunk &fc, BufPool &pool, FrontTotals &tot) {
    const double t_t0 = now();
    const Reads &in = fc.in;
    const uint64_t nq = in.n;
    fc.lo.resize(nq);
    fc.hi.resize(nq);
    fc.hit.resize(nq);
    if (trim) {
        const int rc = rtx_trim_run(trim, nq, in.bases, in.off, fc.lo.data(), fc.hi.data(), fc.hit.data());
        if (rc) return rc;
        auto t = tot.trim;  // (counted in locals: the loops run per read)
        for (uint64_t i = 0; i < nq; i++) {
            t.with5 += (fc.hit[i] & 0xFFu) != RTX_TRIM_NO_PATTERN;
            t.with3 += ((fc.hit[i] >> 16) & 0xFFu) != RTX_TRIM_NO_PATTERN;
            t.emptied += in.len(i) != 0 && fc.hi[i] == fc.lo[i];
        }
        tot.trim = t;
    } else {
        for (uint64_t i = 0; i < nq; i++) {
            fc.lo[i] = 0u;
            fc.hi[i] = in.len32(i);
            fc.hit[i] = RTX_TRIM_NO_PATTERN | RTX_TRIM_NO_PATTERN << 16;
        }
    }
    const double t_q0 = now();
    if (qual) {
        fc.q_hi.resize(nq);
        fc.q_verdict.resize(nq);
        fc.q_ee.resize(nq);
        fc.keep_hi.resize(nq);
        const int rc = rtx_qual_run(qual, nq, in.bases, in.quals, in.off, fc.lo.data(), fc.hi.data(), fc.q_hi.data(), fc.q_ee.data(), fc.q_verdict.data());
        if (rc) return rc;
        auto q = tot.qual;
        for (uint64_t i = 0; i < nq; i++) {
            const uint32_t v = fc.q_verdict[i];
            fc.keep_hi[i] = v ? fc.lo[i] : fc.q_hi[i];
            q.passed += v == 0u;
            q.truncated += v == 0u && fc.q_hi[i] < fc.hi[i];
            for (uint32_t b = 0; b < 7u; b++) q.reasons[b] += (v >> b) & 1u;
        }
        tot.qual = q;
    }
    const double t_s0 = now();
    if (screen) {
        if (!qual) fc.keep_hi = fc.hi;
        for (auto *v : {&fc.s_windows, &fc.s_hits, &fc.s_first, &fc.s_source, &fc.s_verdict}) v->resize(nq);
        const int rc = rtx_screen_run(screen, nq, in.bases, in.off, fc.lo.data(), fc.keep_hi.data(), fc.s_windows.data(), fc.s_hits.data(), fc.s_first.data(),
                                      fc.s_source.data(), fc.s_verdict.data());
        if (rc) return rc;
        auto x = tot.screen;
        for (uint64_t i = 0; i < nq; i++) {
            x.screened += fc.keep_hi[i] != fc.lo[i];
            if (fc.s_verdict[i]) { x.contaminants++; fc.keep_hi[i] = fc.lo[i]; }
        }
        tot.screen = x;
    }
    const double t_c0 = now();
    const int rc = cut(in, fc.lo.data(), (qual || screen ? fc.keep_hi : fc.hi).data(), false, fc.t, pool, "no memory for the trimmed reads of a chunk", fc.src);
    if (rc) return rc;
    fc.dev = fc.src;
    const double t_end = now(), t_cut = t_end - t_c0;  // (the cut counts with the last stage that is on, as before)
    if (trim) { tot.trim.queries += nq; tot.trim.busy += t_q0 - t_t0 + (!qual && !screen ? t_end - t_q0 : 0.0); }
    if (qual) { tot.qual.queries += nq; tot.qual.busy += t_s0 - t_q0 + (!screen ? t_cut : 0.0); }
    if (screen) { tot.screen.queries += nq; tot.screen.busy += t_end - t_s0; }
    return RTX_OK;
}

// The copies of the chunk, on the device (a stream of its own beside the handle's); then the map's host side and the distinct reads.
int run_derep(rtx_derep *stage, FrontChunk &fc, BufPool &pool, unsigned nt, FrontTotals &tot) {
    const double t0 = now();
    const uint64_t nq = fc.src.n;
    std::vector<uint32_t> rep(nq);
    uint64_t nu = 0;
    int rc = rtx_derep_run(stage, nq, fc.src.bases, fc.src.off, rep.data(), &nu);
    if (!rc && nu < nq) {  // (a chunk without copies goes on as it came)
        std::vector<uint32_t> uniq(nq);
        fc.slot.resize(nq);
        fc.size.resize(nq);
        rc = rtx_derep_plan(nq, rep.data(), uniq.data(), fc.slot.data(), fc.size.data(), &nu);
        if (!rc) {
            fc.size.resize(nu);
            rc = gather(fc.src, uniq.data(), nu, fc.u, pool, nt, fc.dev);
        }
    }
    if (rc) return rc;
    tot.derep.queries += nq;
    tot.derep.distinct += fc.dev.n;
    tot.derep.busy += now() - t0;
    return RTX_OK;
}

// The reads that go to the handle, on the device (a stream of its own beside the handle's); a flagged one goes on empty.
int run_chimera(rtx_chimera *stage, FrontChunk &fc, BufPool &pool, FrontTotals &tot) {
    const double t0 = now();
    const Reads dev = fc.dev;
    fc.chim.resize(dev.n);
    int rc = rtx_chimera_run(stage, dev.n, dev.bases, dev.off, fc.chim.data());
    if (rc) return rc;
    bool any = false;
    for (uint64_t u = 0; u < dev.n && !any; u++) any = fc.chim[u].flag != 0u;
    if (any) {  // (a flagged read has at most RTX_CHIMERA_MAX_QUERY bases; a longer one is not checked and is not cut here)
        std::vector<uint32_t> lo(dev.n, 0u), hi(dev.n);
        for (uint64_t u = 0; u < dev.n; u++) {
            if (!fc.chim[u].flag && dev.len(u) > 0xFFFFFFFFull) { rtx::set_error("rtx_raxtax: a read of 2^32 bases or more with the chimera check set"); return RTX_ERR_INVALID; }
            hi[u] = fc.chim[u].flag ? 0u : (uint32_t)dev.len(u);
        }
        rc = cut(dev, lo.data(), hi.data(), false, fc.c, pool, "no memory for the checked reads of a chunk", fc.dev);
        if (rc) return rc;
    }
    tot.chim.queries += fc.given.n;
    tot.chim.checked += dev.n;
    for (uint64_t i = 0; i < fc.given.n; i++) tot.chim.flagged += fc.chim[fc.at(i)].flag != 0u;
    tot.chim.busy += now() - t0;
    return RTX_OK;
}

// The reads that go on to be classified into the handle's tally, on the device (a stream of its own beside the handle's): one entry per query
// of the caller from `src` -- an unassigned, emptied or discarded read and a contaminant are empty there and count nowhere -- with weight 0
// for a query whose representative the chimera check flagged, and the query's own sample where tags are set.
int run_tally(rtx_tally *stage, bool demux, FrontChunk &fc, FrontTotals &tot) {
    const double t0 = now();
    const Reads &src = fc.src;
    const uint64_t nq = src.n;
    std::vector<uint32_t> weight;
    uint64_t counted = 0;
    if (!fc.chim.empty()) {
        weight.resize(nq);
        for (uint64_t i = 0; i < nq; i++) weight[i] = fc.chim[fc.at(i)].flag ? 0u : 1u;
    }
    for (uint64_t i = 0; i < nq; i++) counted += src.len(i) != 0 && (weight.empty() || weight[i]);
    uint64_t before = 0, after = 0;
    int rc = rtx_tally_info(stage, &before, nullptr, nullptr, nullptr, nullptr);
    if (!rc) rc = rtx_tally_add(stage, nq, src.bases, src.off, demux ? fc.dx_sample.data() : nullptr, weight.empty() ? nullptr : weight.data());
    if (!rc) rc = rtx_tally_info(stage, &after, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    tot.tally.queries += nq;
    tot.tally.counted += counted;
    tot.tally.added += after - before;
    tot.tally.busy += now() - t0;
    return RTX_OK;
}

}  // namespace

int cut(const Reads &from, const uint32_t *lo, const uint32_t *keep_hi, bool with_quals, Cut &out, BufPool &pool, const char *oom, Reads &to) {
    bool any = false;
    for (uint64_t i = 0; i < from.n && !any; i++) any = lo[i] != 0u || keep_hi[i] != from.len(i);
    Reads r = from;
    if (any) {  // (a chunk in which nothing was cut goes on as it came, without a copy)
        uint64_t kept = 0;
        for (uint64_t i = 0; i < from.n; i++) kept += keep_hi[i] - lo[i];
        pool.take(out.bases);
        if (with_quals) pool.take(out.quals);
        if (!out.bases.reserve(kept + 1) || (with_quals && !out.quals.reserve(kept + 1))) { rtx::set_error("%s", oom); return RTX_ERR_OOM; }
        out.off.resize(from.n + 1);
        int rc = rtx_trim_apply(from.n, from.bases, from.off, lo, keep_hi, out.bases.p, out.off.data());
        if (!rc && with_quals) rc = rtx_trim_apply(from.n, from.quals, from.off, lo, keep_hi, out.quals.p, out.off.data());
        if (rc) return rc;
        r = Reads{out.bases.p, with_quals ? out.quals.p : nullptr, out.off.data(), from.n};
    }
    to = r;
    return RTX_OK;
}

int gather(const Reads &from, const uint32_t *uniq, uint64_t nu, Cut &out, BufPool &pool, unsigned nt, Reads &to) {
    out.off.assign(nu + 1, 0);
    for (uint64_t u = 0; u < nu; u++) out.off[u + 1] = out.off[u] + from.len(uniq[u]);
    pool.take(out.bases);
    if (!out.bases.reserve(out.off[nu] + 1)) { rtx::set_error("no memory for the distinct reads of a chunk"); return RTX_ERR_OOM; }
    // runs of neighbouring distinct reads that are neighbours in the input as well (most of a chunk with few copies) move in one memcpy
    const Reads src = from;
    const uint64_t *const off = out.off.data();
    uint8_t *const dst = out.bases.p;
    parallel_ranges(nu, nt, [&](uint64_t a, uint64_t b) {
        for (uint64_t u = a; u < b;) {
            uint64_t v = u + 1;
            while (v < b && uniq[v] == uniq[v - 1] + 1u) v++;
            if (off[v] > off[u]) memcpy(dst + off[u], src.bases + src.off[uniq[u]], off[v] - off[u]);
            u = v;
        }
    });
    to = Reads{dst, nullptr, off, nu};
    return RTX_OK;
}

int Front::open(rtx_index *const *indices, uint32_t n_dev, bool has_quals, bool prof) {
    // RTX_OPT_DEREP: on every handle, or on none.  One stage object (rtx_derep.hip) per distinct device for the duration of the call: the
    // lookup thread runs chunk c through the object of handle c mod n_dev's device while that handle still classifies an earlier chunk.
    derep = rtx::index_derep(indices[0]);
    int rc = agree(indices, n_dev, rtx::index_derep, "rtx_raxtax_multi: the handles disagree on RTX_OPT_DEREP");
    if (!rc && derep) rc = dereps.open(indices, n_dev, true, [&](uint32_t d, rtx_derep **out) { return rtx_derep_create(rtx::index_device(indices[d]), out); });
    if (rc) return rc;
    // Tags (rtx_index_set_tags): the same list on every handle
    const rtx::DemuxList &taglist = rtx::index_tags(indices[0]);
    demux = !taglist.empty();
    rc = agree(indices, n_dev, [](const rtx_index *ix) -> const rtx::DemuxList & { return rtx::index_tags(ix); }, "rtx_raxtax_multi: the handles disagree on their tags (rtx_index_set_tags)");
    if (rc) return rc;
    prof_samples = rtx::index_profile_samples(indices[0]);
    rc = agree(indices, n_dev, rtx::index_profile_samples, "rtx_raxtax_multi: the handles disagree on the samples of their taxon profile (rtx_index_profile_begin_samples)");
    if (rc) return rc;
    if (demux && derep && prof) {
        rtx::set_error("rtx_raxtax: tags (rtx_index_set_tags) together with RTX_OPT_DEREP and an open taxon profile: copies from different samples would be counted as one read");
        return RTX_ERR_INVALID;
    }
    if (demux) {
        std::vector<rtx_demux_tag> tags(taglist.codes.size());
        for (size_t i = 0; i < tags.size(); i++) tags[i] = {taglist.codes[i].data(), (uint32_t)taglist.codes[i].size(), taglist.end[i]};
        rc = demuxes.open(indices, n_dev, true, [&](uint32_t d, rtx_demux **out) {
            return rtx_demux_create(rtx::index_device(indices[d]), tags.data(), (uint32_t)tags.size(), taglist.pairs.data(), (uint32_t)taglist.pairs.size(), &taglist.params, out);
        });
        if (rc) return rc;
    }
    // Primers (rtx_index_set_primers): the same list on every handle
    const std::vector<rtx::TrimPrimer> &primers = rtx::index_primers(indices[0]);
    trim = !primers.empty();
    rc = agree(indices, n_dev, [](const rtx_index *ix) -> const std::vector<rtx::TrimPrimer> & { return rtx::index_primers(ix); },
               "rtx_raxtax_multi: the handles disagree on their primers (rtx_index_set_primers)");
    if (rc) return rc;
    if (trim) {
        std::vector<rtx_trim_pattern> pats(primers.size());
        for (size_t i = 0; i < primers.size(); i++) pats[i] = {primers[i].codes.data(), (uint32_t)primers[i].codes.size(), primers[i].end, primers[i].max_errors, primers[i].window};
        rc = trims.open(indices, n_dev, true, [&](uint32_t d, rtx_trim **out) { return rtx_trim_create(rtx::index_device(indices[d]), pats.data(), (uint32_t)pats.size(), out); });
        if (rc) return rc;
    }
    // Quality filter (rtx_index_set_quality): the same setting on every handle, and the call brings the quality strings
    auto quality = [](const rtx_index *ix) { std::pair<bool, rtx_qual_params> s{false, {}}; s.first = rtx::index_quality(ix, &s.second); return s; };
    const rtx_qual_params qparams = quality(indices[0]).second;
    qual = quality(indices[0]).first;
    rc = agree(indices, n_dev, quality, "rtx_raxtax_multi: the handles disagree on their quality filter (rtx_index_set_quality)",
               [](const auto &a, const auto &b) { return a.first == b.first && (!a.first || rtx::qual_params_equal(a.second, b.second)); });
    if (rc) return rc;
    if (qual && !has_quals) { rtx::set_error("rtx_raxtax: a quality filter is set (rtx_index_set_quality) and the call brings no quality strings (rtx_raxtax_multi_ex5)"); return RTX_ERR_INVALID; }
    if (qual) {
        rc = quals.open(indices, n_dev, true, [&](uint32_t d, rtx_qual **out) { return rtx_qual_create(rtx::index_device(indices[d]), &qparams, out); });
        if (rc) return rc;
    }
    // Contaminant screen (rtx_index_set_screen): the same set and parameters on every handle, by their fingerprint (0: off)
    auto screen_fp = [](const rtx_index *ix) {
        rtx_screen_params p{};
        const rtx_screen_set *set = rtx::index_screen(ix, &p);
        return set ? rtx::screen_fingerprint(*set->data, p) : 0ull;
    };
    screen = screen_fp(indices[0]) != 0ull;
    rc = agree(indices, n_dev, screen_fp, "rtx_raxtax_multi: the handles disagree on their contaminant screen (rtx_index_set_screen)");
    if (rc) return rc;
    if (screen) {
        rtx_screen_params sparams{};
        const rtx_screen_set *set = rtx::index_screen(indices[0], &sparams);
        rc = screens.open(indices, n_dev, true, [&](uint32_t d, rtx_screen **out) { return rtx_screen_create(rtx::index_device(indices[d]), set, &sparams, out); });
        if (rc) return rc;
    }
    // Chimera check (rtx_index_set_chimera): the same setting on every handle.  One stage object (rtx_chimera.hip) per HANDLE: it reads that
    // handle's bitmap.  Not with RTX_OPT_STRAND (rtx_chimera_create refuses it: a read is checked in the orientation given).
    auto chimera = [](const rtx_index *ix) { std::pair<bool, rtx_chimera_params> s{false, {}}; s.first = rtx::index_chimera(ix, &s.second); return s; };
    const rtx_chimera_params cparams = chimera(indices[0]).second;
    chim = chimera(indices[0]).first;
    rc = agree(indices, n_dev, chimera, "rtx_raxtax_multi: the handles disagree on their chimera check (rtx_index_set_chimera)",
               [](const auto &a, const auto &b) { return a.first == b.first && (!a.first || (a.second.segments == b.second.segments && a.second.mindelta == b.second.mindelta)); });
    if (rc) return rc;
    if (chim) rc = chims.open(indices, n_dev, false, [&](uint32_t d, rtx_chimera **out) { return rtx_chimera_create(indices[d], &cparams, out); });
    if (rc) return rc;
    // Distinct reads of the run (rtx_index_set_tally): on every handle or on none, an object of its own per handle (each handle's chunks go to
    // that handle's object; the caller sums them: rtx_tally_table_merge), with a column per sample of the tag list
    tally = rtx::index_tally(indices[0]) != nullptr;
    rc = agree(indices, n_dev, [](const rtx_index *ix) { return rtx::index_tally(ix) != nullptr; }, "rtx_raxtax_multi: a tally (rtx_index_set_tally) is set on some handles and not on others");
    if (rc) return rc;
    if (tally) {
        uint32_t want = 0u;  // the samples of the tag list: its highest sample + 1
        for (const rtx_demux_pair &pr : taglist.pairs) want = std::max(want, pr.sample + 1u);
        tallies.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            tallies[d] = rtx::index_tally(indices[d]);
            for (uint32_t e = 0; e < d; e++)
                if (tallies[e] == tallies[d]) { rtx::set_error("rtx_raxtax_multi: handles %u and %u share one tally (rtx_index_set_tally): every handle needs an object of its own", e, d); return RTX_ERR_INVALID; }
            if (rtx::tally_samples(tallies[d]) != want) {
                rtx::set_error("rtx_raxtax: the tally (rtx_index_set_tally) has n_samples %u; it must be %u: %s", rtx::tally_samples(tallies[d]), want,
                               demux ? "the samples of the tag list (rtx_index_set_tags)" : "0 without tags");
                return RTX_ERR_INVALID;
            }
        }
    }
    return RTX_OK;
}

int Front::run(uint32_t d, FrontChunk &fc, BufPool &pool, unsigned nt, FrontTotals &tot) const {
    int rc = RTX_OK;
    if (demux) rc = run_demux(demuxes.of[d], fc, pool, tot);
    if (!rc && (trim || qual || screen)) rc = run_trim_qual_screen(trim ? trims.of[d] : nullptr, qual ? quals.of[d] : nullptr, screen ? screens.of[d] : nullptr, fc, pool, tot);
    if (!rc && derep) rc = run_derep(dereps.of[d], fc, pool, nt, tot);
    if (!rc && chim) rc = run_chimera(chims.of[d], fc, pool, tot);
    if (!rc && tally) rc = run_tally(tallies[d], demux, fc, tot);
    return rc;
}

}  // namespace rtx_front

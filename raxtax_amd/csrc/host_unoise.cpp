// Denoising on the host: see host_unoise.hpp.
#include "host_unoise.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace rtx {

int unoise_open(const char *who, rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out, rtx_tally_view *view, rtx_unoise_params *p) {
    if (out) *out = nullptr;
    if (!table || !out) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    *p = rtx_unoise_params{};
    p->minsize = 8;
    p->alpha = 2;
    if (params) *p = *params;
    if (p->alpha < 1u || p->alpha > 8u) { set_error("%s: alpha = %u (1 .. 8)", who, p->alpha); return RTX_ERR_INVALID; }
    if (p->minsize == 0) { set_error("%s: minsize = 0 (at least 1)", who); return RTX_ERR_INVALID; }
    if (p->max_diffs > RTX_UNOISE_MAX_DIFFS) { set_error("%s: max_diffs = %u (at most %u)", who, p->max_diffs, (unsigned)RTX_UNOISE_MAX_DIFFS); return RTX_ERR_INVALID; }
    if (p->flags) { set_error("%s: flags = %u (none is defined)", who, p->flags); return RTX_ERR_INVALID; }
    if (!p->max_diffs) p->max_diffs = RTX_UNOISE_MAX_DIFFS;
    if (const int rc = rtx_tally_table_view(table, view)) return rc;
    if (view->n_entries > 0x7FFFFFFEull) { set_error("%s: %llu rows (at most 2^31 - 2)", who, (unsigned long long)view->n_entries); return RTX_ERR_INVALID; }
    return RTX_OK;
}

void unoise_lim(const rtx_tally_view &view, uint32_t alpha, std::vector<uint32_t> &lim) {
    const uint64_t n = view.n_entries;
    lim.resize(n);
    uint64_t l = 0;  // (w[e] never grows with e, so the prefix never shrinks)
    for (uint64_t e = 0; e < n; e++) {
        while (l < n && (view.sizes[l] >> (alpha + 1u)) >= view.sizes[e]) l++;
        lim[e] = (uint32_t)l;
    }
}

void unoise_tiers(const rtx_tally_view &view, uint32_t alpha, std::vector<uint64_t> &begin) {
    const uint64_t n = view.n_entries;
    begin.clear();
    for (uint64_t s0 = 0; s0 < n;) {
        begin.push_back(s0);
        uint64_t s1 = s0 + 1;
        while (s1 < n && (view.sizes[s0] >> (alpha + 1u)) < view.sizes[s1]) s1++;
        s0 = s1;
    }
    begin.push_back(n);
}

int unoise_build(const char *who, rtx_otu &o, const rtx_tally_view &view) {
    rtx_unoise_info &u = *o.unoise;
    const uint64_t n = view.n_entries;
    o.otu.assign(n, 0);
    o.long_rows = 0;
    u.weight.assign(view.sizes, view.sizes + n);
    for (int i = 0; i < 4; i++) u.n_status[i] = 0;
    uint32_t n_otus = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint8_t st = u.status[r];
        if (st > RTX_UNOISE_LONG) { set_error("%s: row %llu has the status %u", who, (unsigned long long)r, st); return RTX_ERR_HIP; }
        u.n_status[st]++;
        if (st == RTX_UNOISE_LONG) o.long_rows++;
        if (st == RTX_UNOISE_ABSORBED) {
            const uint32_t p = u.parent[r];
            if (p >= u.lim[r] || u.status[p] != RTX_UNOISE_ZOTU || u.dist[r] == 0u || u.dist[r] > u.params.max_diffs) {
                set_error("%s: row %llu is absorbed by row %u at %u differences", who, (unsigned long long)r, p, u.dist[r]);
                return RTX_ERR_HIP;
            }
            o.otu[r] = o.otu[p];  // (p < lim(r) <= r: numbered already)
        } else {
            o.otu[r] = n_otus++;
        }
    }
    otu_sums(o, view);
    o.link_a.clear();
    o.link_b.clear();
    o.rounds = 0;
    o.link_passes = 0;
    return RTX_OK;
}

namespace {

// the Levenshtein distance of two byte strings: the full table, two rows of it at a time
uint32_t levenshtein(const uint8_t *x, uint64_t nx, const uint8_t *y, uint64_t ny, std::vector<uint32_t> &prev, std::vector<uint32_t> &cur) {
    prev.resize(ny + 1);
    cur.resize(ny + 1);
    for (uint64_t j = 0; j <= ny; j++) prev[j] = (uint32_t)j;
    for (uint64_t i = 1; i <= nx; i++) {
        cur[0] = (uint32_t)i;
        for (uint64_t j = 1; j <= ny; j++) cur[j] = std::min({prev[j - 1] + (x[i - 1] != y[j - 1] ? 1u : 0u), prev[j] + 1u, cur[j - 1] + 1u});
        prev.swap(cur);
    }
    return prev[ny];
}

const char *const kStatusName[4] = {"zotu", "absorbed", "left", "long"};

}  // namespace

}  // namespace rtx

extern "C" {

int rtx_otu_unoise_host(rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_unoise_params p{};
    if (const int rc = rtx::unoise_open("rtx_otu_unoise_host", table, params, out, &v, &p)) return rc;
    auto *o = new rtx_otu();
    o->unoise.reset(new rtx_unoise_info());
    rtx_unoise_info &u = *o->unoise;
    u.params = p;
    const uint64_t n = v.n_entries;
    rtx::unoise_lim(v, p.alpha, u.lim);
    u.status.assign(n, RTX_UNOISE_LEFT);
    u.parent.assign(n, RTX_NO_REF);
    u.dist.assign(n, RTX_NO_DIST);
    std::vector<uint32_t> live, prev, cur;  // the ZOTUs so far, in rank order
    for (uint64_t e = 0; e < n; e++) {
        const uint64_t len = v.base_off[e + 1] - v.base_off[e];
        if (len > RTX_OTU_MAX_LEN) { u.status[e] = RTX_UNOISE_LONG; continue; }
        const uint64_t we = v.sizes[e];
        uint32_t best_d = RTX_NO_DIST, best_p = RTX_NO_REF;
        for (const uint32_t q : live) {
            if (q >= u.lim[e]) break;
            uint32_t k = 0;
            for (uint32_t d = 1; d <= p.max_diffs; d++) {
                const uint32_t sh = p.alpha * d + 1u;
                if (sh < 64u && (v.sizes[q] >> sh) >= we) k = d;
            }
            if (k == 0) continue;
            const uint32_t d = rtx::levenshtein(v.bases + v.base_off[e], len, v.bases + v.base_off[q], v.base_off[q + 1] - v.base_off[q], prev, cur);
            if (d <= k && d < best_d) { best_d = d; best_p = q; }  // (q ascending: the first at a distance keeps it)
        }
        if (best_p != RTX_NO_REF) {
            u.status[e] = RTX_UNOISE_ABSORBED;
            u.parent[e] = best_p;
            u.dist[e] = best_d;
        } else if (we >= p.minsize) {
            u.status[e] = RTX_UNOISE_ZOTU;
            live.push_back((uint32_t)e);
        }
    }
    if (const int rc = rtx::unoise_build("rtx_otu_unoise_host", *o, v)) { delete o; return rc; }
    *out = o;
    return RTX_OK;
}

int rtx_otu_unoise_view(rtx_otu *o, rtx_unoise_view_t *view) {
    if (!o || !view) { rtx::set_error("rtx_otu_unoise_view: null argument"); return RTX_ERR_INVALID; }
    if (!o->unoise) { rtx::set_error("rtx_otu_unoise_view: the object is no denoising result"); return RTX_ERR_INVALID; }
    const rtx_unoise_info &u = *o->unoise;
    view->n_rows = o->n_rows;
    view->status = u.status.data();
    view->parent = u.parent.data();
    view->dist = u.dist.data();
    view->lim = u.lim.data();
    view->n_zotu = u.n_status[RTX_UNOISE_ZOTU];
    view->n_absorbed = u.n_status[RTX_UNOISE_ABSORBED];
    view->n_left = u.n_status[RTX_UNOISE_LEFT];
    view->n_long = u.n_status[RTX_UNOISE_LONG];
    view->minsize = u.params.minsize;
    view->alpha = u.params.alpha;
    view->max_diffs = u.params.max_diffs;
    view->tiers = u.tiers;
    view->launches = u.launches;
    view->pairs = u.pairs;
    view->pairs_length = u.pairs_length;
    view->pairs_finished = u.pairs_finished;
    for (int i = 0; i < 4; i++) view->seconds[i] = u.seconds[i];
    return RTX_OK;
}

int64_t rtx_otu_format_unoise(rtx_otu *o, char *buf, uint64_t cap) {
    if (!o) { rtx::set_error("rtx_otu_format_unoise: null argument"); return RTX_ERR_INVALID; }
    if (!o->unoise) { rtx::set_error("rtx_otu_format_unoise: the object is no denoising result"); return RTX_ERR_INVALID; }
    const rtx_unoise_info &u = *o->unoise;
    std::string text = "#read\tsize\tstatus\tparent\tdiffs\totu\n";
    char num[200], par[32], dif[16];
    for (uint64_t r = 0; r < o->n_rows; r++) {
        if (u.status[r] == RTX_UNOISE_ABSORBED) {
            snprintf(par, sizeof par, "uniq%llu", (unsigned long long)u.parent[r] + 1);
            snprintf(dif, sizeof dif, "%u", u.dist[r]);
        } else {
            snprintf(par, sizeof par, "*");
            snprintf(dif, sizeof dif, "*");
        }
        snprintf(num, sizeof num, "uniq%llu\t%llu\t%s\t%s\t%s\totu%llu\n", (unsigned long long)r + 1, (unsigned long long)u.weight[r], rtx::kStatusName[u.status[r]], par, dif,
                 (unsigned long long)o->otu[r] + 1);
        text += num;
    }
    return rtx::hand_out("rtx_otu_format_unoise", text, buf, cap);
}

}  // extern "C"

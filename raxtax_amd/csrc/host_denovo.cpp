// The de novo chimera check of a run on the host: see host_denovo.hpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__)
#endif
#include "host_denovo.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <unordered_set>

#include "rtx_math.hpp"

namespace rtx {

int denovo_open(const char *who, rtx_tally_table *table, rtx_otu *otu, const rtx_denovo_params *params, rtx_denovo **out, rtx_tally_view *view, rtx_denovo_params *p) {
    if (out) *out = nullptr;
    if (!table || !out) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    *p = rtx_denovo_params{RTX_CHIMERA_DEFAULT_SEGMENTS, RTX_CHIMERA_DEFAULT_MINDELTA, RTX_DENOVO_DEFAULT_ABSKEW, 0u, 0u};
    if (params) *p = *params;
    if (p->segments < 2u || p->segments > RTX_CHIMERA_MAX_SEGMENTS) { set_error("%s: %u segments (2 .. %u)", who, p->segments, RTX_CHIMERA_MAX_SEGMENTS); return RTX_ERR_INVALID; }
    if (p->abskew == 0u) { set_error("%s: abskew = 0 (an integer >= 1)", who); return RTX_ERR_INVALID; }
    if (p->flags) { set_error("%s: flags = %u (none is defined)", who, p->flags); return RTX_ERR_INVALID; }
    if (p->max_parents > RTX_DENOVO_DEFAULT_MAX_PARENTS) { set_error("%s: max_parents = %u (at most %u)", who, p->max_parents, RTX_DENOVO_DEFAULT_MAX_PARENTS); return RTX_ERR_INVALID; }
    if (p->max_parents == 0u) p->max_parents = RTX_DENOVO_DEFAULT_MAX_PARENTS;
    if (const int rc = rtx_tally_table_view(table, view)) return rc;
    if (otu && otu->n_rows != view->n_entries) {
        set_error("%s: the table has %llu rows, the OTUs were made from %llu", who, (unsigned long long)view->n_entries, (unsigned long long)otu->n_rows);
        return RTX_ERR_INVALID;
    }
    const uint64_t n = otu ? otu->n_otus : view->n_entries;
    if (n > 0x7FFFFFFEull) { set_error("%s: %llu entries (at most 2^31 - 2)", who, (unsigned long long)n); return RTX_ERR_INVALID; }
    return RTX_OK;
}

rtx_chimera_rec denovo_blank(uint32_t status) { return rtx_chimera_rec{status, 0u, 0u, RTX_NO_REF, 0u, 0u, 0u, RTX_NO_REF, 0u, RTX_NO_REF, 0u, 0u}; }

void denovo_entries(rtx_denovo &d, const rtx_tally_view &view, const rtx_otu *otu, const rtx_denovo_params &p) {
    d.params = p;
    d.n_rows = view.n_entries;
    d.otu_mode = otu != nullptr;
    const uint64_t n = otu ? otu->n_otus : view.n_entries;
    d.n_entries = n;
    d.row.resize(n);
    d.weight.resize(n);
    d.lim.resize(n);
    if (otu) {
        d.otu.resize(n);
        std::iota(d.otu.begin(), d.otu.end(), 0u);  // (the OTUs are numbered in the order of their seeds' ranks: a stable sort keeps that among equals)
        std::stable_sort(d.otu.begin(), d.otu.end(), [&](uint32_t a, uint32_t b) { return otu->sizes[a] > otu->sizes[b]; });
        for (uint64_t e = 0; e < n; e++) { d.row[e] = otu->seed[d.otu[e]]; d.weight[e] = otu->sizes[d.otu[e]]; }
    } else {
        for (uint64_t e = 0; e < n; e++) { d.row[e] = (uint32_t)e; d.weight[e] = view.sizes[e]; }
    }
    // lim: w[p] >= abskew w[e] <=> floor(w[p] / abskew) >= w[e], so nothing overflows; one binary search per distinct weight
    const uint64_t a = p.abskew;
    uint64_t skew = 0;
    for (uint64_t e = 0; e < n; e++) {
        if (e == 0 || d.weight[e] != d.weight[e - 1]) {
            const uint64_t w = d.weight[e];
            skew = (uint64_t)(std::partition_point(d.weight.begin(), d.weight.end(), [&](uint64_t wp) { return wp / a >= w; }) - d.weight.begin());
        }
        d.lim[e] = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(e, skew), p.max_parents);
    }
    d.rec.assign(n, denovo_blank(RTX_DENOVO_NO_PARENT));
}

void denovo_totals(rtx_denovo &d) {
    d.n_checked = d.n_flagged = 0;
    for (const rtx_chimera_rec &r : d.rec) {
        d.n_checked += r.status == RTX_CHIM_OK ? 1u : 0u;
        d.n_flagged += r.flag ? 1u : 0u;
    }
}

namespace {

// the definition, entry by entry: the 8-mers of every parent as a set, the parents of e as an explicit list
void host_check(const rtx_tally_view &v, rtx_denovo &d) {
    const uint64_t n = d.n_entries;
    const uint32_t S = d.params.segments;
    const uint32_t n_par = n ? d.lim[n - 1] : 0u;  // (lim never decreases along the list)
    std::vector<std::unordered_set<uint32_t>> kmers(n_par);
    auto seq_of = [&](uint64_t e, uint64_t &len) {
        len = v.base_off[d.row[e] + 1u] - v.base_off[d.row[e]];
        return v.bases + v.base_off[d.row[e]];
    };
    for (uint32_t p = 0; p < n_par; p++) {
        uint64_t len;
        const uint8_t *s = seq_of(p, len);
        for (uint64_t i = 0; i + 8u <= len; i++) {
            uint32_t k;
            if (chimera_window_kmer(s, (uint32_t)i, k)) kmers[p].insert(k);
        }
    }
    std::vector<uint32_t> parents, win_k, win_seg;
    for (uint64_t e = 0; e < n; e++) {
        uint64_t len64;
        const uint8_t *s = seq_of(e, len64);
        const uint32_t len = (uint32_t)std::min<uint64_t>(len64, 0xFFFFFFFFull), n_pos = chimera_n_pos(len);
        if (len > kChimMaxQuery) { d.rec[e] = denovo_blank(RTX_CHIM_TOO_LONG); continue; }
        win_k.clear();
        win_seg.clear();
        for (uint32_t sg = 0; sg < S; sg++)
            for (uint32_t i = chimera_boundary(n_pos, S, sg); i < chimera_boundary(n_pos, S, sg + 1u); i++) {
                uint32_t k;
                if (chimera_window_kmer(s, i, k)) { win_k.push_back(k); win_seg.push_back(sg); }
            }
        const uint32_t n_valid = (uint32_t)win_k.size();
        if (n_valid == 0u) { d.rec[e] = denovo_blank(RTX_CHIM_NO_KMER); continue; }
        if (d.lim[e] == 0u) { d.rec[e] = denovo_blank(RTX_DENOVO_NO_PARENT); continue; }
        parents.clear();
        for (uint32_t p = 0; p < d.lim[e]; p++)
            if (!d.rec[p].flag) parents.push_back(p);
        uint32_t pm[kChimMaxSegments + 1] = {0}, sm[kChimMaxSegments + 1] = {0}, pr[kChimMaxSegments + 1], sr[kChimMaxSegments + 1];
        for (uint32_t sg = 0; sg <= kChimMaxSegments; sg++) pr[sg] = sr[sg] = kChimNoRef;
        for (const uint32_t p : parents) {  // ascending: a tie keeps the lower entry
            uint32_t cnt[kChimMaxSegments] = {0}, T = 0, P = 0;
            const std::unordered_set<uint32_t> &set = kmers[p];
            for (uint32_t j = 0; j < n_valid; j++)
                if (set.count(win_k[j])) { cnt[win_seg[j]]++; T++; }
            if (!T) continue;
            for (uint32_t sg = 0; sg <= S; sg++) {
                chimera_take(pm[sg], pr[sg], P, p);
                chimera_take(sm[sg], sr[sg], T - P, p);
                if (sg < S) P += cnt[sg];
            }
        }
        const ChimRec c = chimera_record(len, n_valid, S, d.params.mindelta, pm, pr, sm, sr);
        static_assert(sizeof(ChimRec) == sizeof(rtx_chimera_rec), "twelve uint32");
        std::memcpy(&d.rec[e], &c, sizeof c);
    }
}

std::string entry_name(const rtx_denovo &d, uint32_t e) {
    if (e == RTX_NO_REF) return "*";
    char num[32];
    if (d.otu_mode) snprintf(num, sizeof num, "otu%llu", (unsigned long long)d.otu[e] + 1ull);
    else snprintf(num, sizeof num, "uniq%llu", (unsigned long long)d.row[e] + 1ull);
    return num;
}

// keep[k]: OTU k (with an OTU object) or row k passes: not flagged and at least minsize
int denovo_keep(const char *who, const rtx_denovo *d, rtx_tally_table *table, const rtx_otu *otu, uint64_t minsize, rtx_tally_view *v, std::vector<uint8_t> &keep) {
    if (!d || !table) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (const int rc = rtx_tally_table_view(table, v)) return rc;
    if ((otu != nullptr) != d->otu_mode || v->n_entries != d->n_rows || (otu && (otu->n_rows != d->n_rows || otu->n_otus != d->n_entries))) {
        set_error("%s: not the table and the OTUs the check was made from", who);
        return RTX_ERR_INVALID;
    }
    keep.assign(d->n_entries, 0);
    for (uint64_t e = 0; e < d->n_entries; e++) keep[d->otu_mode ? d->otu[e] : d->row[e]] = !d->rec[e].flag && d->weight[e] >= minsize;
    return RTX_OK;
}

}  // namespace
}  // namespace rtx

extern "C" {

int rtx_denovo_check_host(rtx_tally_table *table, rtx_otu *otu, const rtx_denovo_params *params, rtx_denovo **out) {
    rtx_tally_view v{};
    rtx_denovo_params p{};
    if (const int rc = rtx::denovo_open("rtx_denovo_check_host", table, otu, params, out, &v, &p)) return rc;
    auto *d = new rtx_denovo();
    rtx::denovo_entries(*d, v, otu, p);
    rtx::host_check(v, *d);
    rtx::denovo_totals(*d);
    d->rounds = 1;
    d->scans = d->n_entries;
    *out = d;
    return RTX_OK;
}

int rtx_denovo_view(rtx_denovo *d, rtx_denovo_view_t *view) {
    if (!d || !view) { rtx::set_error("rtx_denovo_view: null argument"); return RTX_ERR_INVALID; }
    view->n_entries = d->n_entries;
    view->row = d->row.data();
    view->otu = d->otu_mode ? d->otu.data() : nullptr;
    view->weight = d->weight.data();
    view->lim = d->lim.data();
    view->rec = d->rec.data();
    view->n_checked = d->n_checked;
    view->n_flagged = d->n_flagged;
    view->rounds = d->rounds;
    view->scans = d->scans;
    return RTX_OK;
}

int rtx_denovo_times(const rtx_denovo *d, double seconds[4]) {
    if (!d || !seconds) { rtx::set_error("rtx_denovo_times: null argument"); return RTX_ERR_INVALID; }
    for (int i = 0; i < 4; i++) seconds[i] = d->seconds[i];
    return RTX_OK;
}

void rtx_denovo_destroy(rtx_denovo *d) { delete d; }

int64_t rtx_denovo_format_records(rtx_denovo *d, char *buf, uint64_t cap) {
    if (!d) { rtx::set_error("rtx_denovo_format_records: null argument"); return RTX_ERR_INVALID; }
    std::string text = "#entry\tweight\tstatus\twindows\tsingle\tparent\tseg\tpos\tleft\ta\tright\tb\tdelta\tchimera\n";
    char num[160];
    for (uint64_t e = 0; e < d->n_entries; e++) {
        const rtx_chimera_rec &r = d->rec[e];
        text += rtx::entry_name(*d, (uint32_t)e);
        snprintf(num, sizeof num, "\t%llu\t%u\t%u\t%u\t", (unsigned long long)d->weight[e], r.status, r.n_valid, r.single);
        text += num;
        text += rtx::entry_name(*d, r.parent);
        snprintf(num, sizeof num, "\t%u\t%u\t%u\t", r.seg, r.pos, r.left);
        text += num;
        text += rtx::entry_name(*d, r.parent_a);
        snprintf(num, sizeof num, "\t%u\t", r.right);
        text += num;
        text += rtx::entry_name(*d, r.parent_b);
        snprintf(num, sizeof num, "\t%u\t%c\n", r.delta, r.flag ? 'Y' : (r.status == RTX_CHIM_OK ? 'N' : '?'));
        text += num;
    }
    return rtx::hand_out("rtx_denovo_format_records", text, buf, cap);
}

int64_t rtx_denovo_format_fasta(rtx_denovo *d, rtx_tally_table *table, rtx_otu *otu, uint64_t minsize, char *buf, uint64_t cap) {
    rtx_tally_view v{};
    std::vector<uint8_t> keep;
    if (const int rc = rtx::denovo_keep("rtx_denovo_format_fasta", d, table, otu, minsize, &v, keep)) return rc;
    std::string text;
    char num[96];
    for (uint64_t k = 0; k < keep.size(); k++) {
        if (!keep[k]) continue;
        const uint64_t r = otu ? otu->seed[k] : k;
        if (otu) snprintf(num, sizeof num, ">otu%llu;size=%llu;seed=uniq%llu\n", (unsigned long long)(k + 1), (unsigned long long)otu->sizes[k], (unsigned long long)(r + 1));
        else snprintf(num, sizeof num, ">uniq%llu;size=%llu\n", (unsigned long long)(k + 1), (unsigned long long)v.sizes[k]);
        text += num;
        for (uint64_t i = v.base_off[r]; i < v.base_off[r + 1]; i++) text += rtx::text_base(v.bases[i]);
        text += '\n';
    }
    return rtx::hand_out("rtx_denovo_format_fasta", text, buf, cap);
}

int64_t rtx_denovo_format_table(rtx_denovo *d, rtx_tally_table *table, rtx_otu *otu, const char *const *names, uint64_t minsize, char *buf, uint64_t cap) {
    rtx_tally_view v{};
    std::vector<uint8_t> keep;
    if (!names) { rtx::set_error("rtx_denovo_format_table: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::denovo_keep("rtx_denovo_format_table", d, table, otu, minsize, &v, keep)) return rc;
    const uint32_t nc = v.n_columns;
    std::string text = otu ? "#otu" : "#uniq";
    for (uint32_t c = 0; c < nc; c++) {
        if (!names[c]) { rtx::set_error("rtx_denovo_format_table: name %u is null", c); return RTX_ERR_INVALID; }
        text += '\t';
        text += names[c];
    }
    text += '\n';
    char num[32];
    for (uint64_t k = 0; k < keep.size(); k++) {
        if (!keep[k]) continue;
        snprintf(num, sizeof num, otu ? "otu%llu" : "uniq%llu", (unsigned long long)(k + 1));
        text += num;
        for (uint32_t c = 0; c < nc; c++) {
            snprintf(num, sizeof num, "\t%llu", (unsigned long long)(otu ? otu->counts[k * nc + c] : v.counts[k * nc + c]));
            text += num;
        }
        text += '\n';
    }
    return rtx::hand_out("rtx_denovo_format_table", text, buf, cap);
}

}  // extern "C"

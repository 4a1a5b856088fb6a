// The OTUs of a run on the host: see host_otu.hpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__)
#endif
#include "host_otu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "rtx_math.hpp"  // text_base: the letters of the seeds

namespace rtx {

int otu_open(const char *who, rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out, rtx_tally_view *view, rtx_otu_params *p) {
    if (out) *out = nullptr;
    if (!table || !out) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    *p = rtx_otu_params{};
    if (params) *p = *params;
    if (p->differences > 1u) { set_error("%s: differences = %u (only d = 1 is built)", who, p->differences); return RTX_ERR_INVALID; }
    if (p->flags) { set_error("%s: flags = %u (none is defined)", who, p->flags); return RTX_ERR_INVALID; }
    if (const int rc = rtx_tally_table_view(table, view)) return rc;
    if (view->n_entries > 0x7FFFFFFEull) { set_error("%s: %llu rows (at most 2^31 - 2)", who, (unsigned long long)view->n_entries); return RTX_ERR_INVALID; }
    return RTX_OK;
}

void otu_sums(rtx_otu &o, const rtx_tally_view &view) {
    const uint64_t n = view.n_entries;
    o.seed.clear();
    for (uint64_t r = 0; r < n; r++)
        if (o.otu[r] == o.seed.size()) o.seed.push_back((uint32_t)r);  // (a seed is the lowest rank of its OTU, and the OTUs are numbered in seed order)
    otu_totals(o, view);
}

void otu_totals(rtx_otu &o, const rtx_tally_view &view) {
    const uint64_t n = view.n_entries;
    const uint32_t nc = view.n_columns;
    o.n_rows = n;
    o.columns = nc;
    o.n_otus = o.seed.size();
    o.members.assign(o.n_otus, 0);
    o.sizes.assign(o.n_otus, 0);
    o.counts.assign(o.n_otus * nc, 0);
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t k = o.otu[r];
        o.members[k]++;
        o.sizes[k] += view.sizes[r];
        for (uint32_t c = 0; c < nc; c++) o.counts[k * nc + c] += view.counts[r * nc + c];
    }
}

namespace {

bool plain(uint8_t c) { return c == 1u || c == 2u || c == 4u || c == 8u; }

// every pair of linked rows, from the definition: the variants of every row looked up in the table's own map
void host_links(rtx_tally_table &t, const rtx_tally_view &v, rtx_otu &o) {
    const uint64_t n = v.n_entries;
    std::vector<uint32_t> rank_of(n);
    for (uint64_t r = 0; r < n; r++) rank_of[v.first[r]] = (uint32_t)r;
    std::vector<uint64_t> pairs;
    auto look = [&](const std::string &key, uint64_t x) {
        const auto it = t.index.find(key);
        if (it == t.index.end()) return;
        const uint64_t y = rank_of[it->second];
        pairs.push_back(x < y ? x << 32 | y : y << 32 | x);
    };
    std::string sub, del;
    for (uint64_t x = 0; x < n; x++) {
        const uint8_t *s = v.bases + v.base_off[x];
        const uint64_t len = v.base_off[x + 1] - v.base_off[x];
        if (len > RTX_OTU_MAX_LEN) { o.long_rows++; continue; }
        sub.assign(reinterpret_cast<const char *>(s), len);
        for (uint64_t i = 0; i < len; i++) {  // one code replaced by A, C, G or T
            for (uint8_t c = 1; c <= 8; c <<= 1) {
                if (c == s[i]) continue;
                sub[i] = (char)c;
                look(sub, x);
            }
            sub[i] = (char)s[i];
        }
        if (len < 2) continue;  // (the table holds no empty row)
        del.assign(reinterpret_cast<const char *>(s) + 1, len - 1);  // one code deleted: s without s[i]
        for (uint64_t i = 0; i < len; i++) {
            if (i) del[i - 1] = (char)s[i - 1];
            if (i == 0 || s[i] != s[i - 1]) look(del, x);  // (inside a run of equal codes every deletion gives the same row)
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());  // (two plain bases at the one position: found from either side)
    for (const uint64_t pr : pairs) {
        o.link_a.push_back((uint32_t)(pr >> 32));
        o.link_b.push_back((uint32_t)pr);
    }
}

// the greedy growth, as the definition states it
void host_grow(const rtx_tally_view &v, rtx_otu &o) {
    const uint64_t n = v.n_entries, nl = o.link_a.size();
    std::vector<uint64_t> begin(n + 1, 0);
    for (uint64_t l = 0; l < nl; l++) { begin[o.link_a[l] + 1u]++; begin[o.link_b[l] + 1u]++; }
    for (uint64_t r = 0; r < n; r++) begin[r + 1] += begin[r];
    std::vector<uint32_t> adj(2 * nl);
    std::vector<uint64_t> fill(begin.begin(), begin.end() - 1);
    for (uint64_t l = 0; l < nl; l++) { adj[fill[o.link_a[l]]++] = o.link_b[l]; adj[fill[o.link_b[l]]++] = o.link_a[l]; }
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    o.otu.assign(n, kNone);
    std::vector<uint32_t> queue;
    uint32_t n_otus = 0;
    for (uint64_t s = 0; s < n; s++) {
        if (o.otu[s] != kNone) continue;
        o.otu[s] = n_otus;
        queue.assign(1, (uint32_t)s);
        for (size_t head = 0; head < queue.size(); head++) {
            const uint32_t x = queue[head];
            for (uint64_t k = begin[x]; k < begin[x + 1]; k++) {
                const uint32_t y = adj[k];
                if (o.otu[y] == kNone && v.sizes[y] <= v.sizes[x]) { o.otu[y] = n_otus; queue.push_back(y); }
            }
        }
        n_otus++;
    }
}

// every string of B1(s), as the definition lists them (a string that two edits give is handed over once per run of equal codes)
template <class F>
void ball(const uint8_t *s, uint64_t len, F f) {
    std::string v(reinterpret_cast<const char *>(s), len);
    f(v);
    for (uint64_t i = 0; i < len; i++) {
        for (uint8_t c = 1; c <= 8; c <<= 1) {
            if (c == s[i]) continue;
            v[i] = (char)c;
            f(v);
        }
        v[i] = (char)s[i];
    }
    if (len >= 2) {
        std::string del(reinterpret_cast<const char *>(s) + 1, len - 1);
        for (uint64_t i = 0; i < len; i++) {
            if (i) del[i - 1] = (char)s[i - 1];
            if (i == 0 || s[i] != s[i - 1]) f(del);
        }
    }
    if (len + 1 <= RTX_OTU_MAX_LEN) {
        std::string ins(1, '\0');
        ins.append(reinterpret_cast<const char *>(s), len);  // s with one place in front of s[0]
        for (uint64_t i = 0; i <= len; i++) {
            if (i) ins[i - 1] = (char)s[i - 1];
            for (uint8_t c = 1; c <= 8; c <<= 1) {
                if (i < len && s[i] == c) continue;  // (the same string as c behind s[i])
                ins[i] = (char)c;
                f(ins);
            }
        }
    }
}

}  // namespace

int graft_open(const char *who, rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out, rtx_tally_view *view, rtx_graft_params *p) {
    if (out) *out = nullptr;
    if (!table || !otu || !out) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    *p = rtx_graft_params{};
    if (params) *p = *params;
    if (p->flags) { set_error("%s: flags = %u (none is defined)", who, p->flags); return RTX_ERR_INVALID; }
    if (p->bloom_log2 && (p->bloom_log2 < 5u || p->bloom_log2 > 40u)) { set_error("%s: bloom_log2 = %u (0, or 5 .. 40)", who, p->bloom_log2); return RTX_ERR_INVALID; }
    if (!p->boundary) p->boundary = 3;
    if (!p->max_bloom_bytes) p->max_bloom_bytes = 1ull << 33;
    if (const int rc = rtx_tally_table_view(table, view)) return rc;
    if (view->n_entries != otu->n_rows || view->n_columns != otu->columns) {
        set_error("%s: the table has %llu rows, the OTUs were made from %llu", who, (unsigned long long)view->n_entries, (unsigned long long)otu->n_rows);
        return RTX_ERR_INVALID;
    }
    return RTX_OK;
}

void graft_heavy(const rtx_otu &in, uint64_t boundary, std::vector<uint8_t> &heavy, rtx_graft_info &g) {
    g.boundary = boundary;
    g.old_otus = in.n_otus;
    for (uint64_t k = 0; k < in.n_otus; k++) (in.sizes[k] >= boundary ? g.heavy_otus : g.light_otus)++;
    heavy.resize(in.n_rows);
    for (uint64_t r = 0; r < in.n_rows; r++) {
        heavy[r] = in.sizes[in.otu[r]] >= boundary;
        (heavy[r] ? g.heavy_rows : g.light_rows)++;
    }
}

void graft_build(const rtx_otu &in, const rtx_tally_view &view, const std::vector<uint8_t> &heavy, std::vector<uint32_t> parent, rtx_otu &out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    rtx_graft_info &g = *out.graft;
    const uint64_t n = in.n_rows, no = in.n_otus;
    std::vector<uint64_t> key(no, ~0ull);  // per light OTU the smallest (parent, child)
    for (uint64_t x = 0; x < n; x++)
        if (!heavy[x] && parent[x] != kNone) key[in.otu[x]] = std::min(key[in.otu[x]], (uint64_t)parent[x] << 32 | x);
    g.old_to_new.assign(no, kNone);
    out.seed.clear();
    for (uint64_t k = 0; k < no; k++)  // the survivors keep their seeds, in the order of their old numbers
        if (key[k] == ~0ull) { g.old_to_new[k] = (uint32_t)out.seed.size(); out.seed.push_back(in.seed[k]); }
    for (uint64_t k = 0; k < no; k++) {
        if (key[k] == ~0ull) continue;
        const uint32_t p = (uint32_t)(key[k] >> 32), target = in.otu[p];  // (heavy: it survives)
        g.old_to_new[k] = g.old_to_new[target];
        g.light.push_back((uint32_t)k);
        g.size.push_back(in.sizes[k]);
        g.child.push_back((uint32_t)key[k]);
        g.par.push_back(p);
        g.heavy.push_back(target);
        g.into.push_back(g.old_to_new[target]);
    }
    g.parent = std::move(parent);
    out.otu.resize(n);
    for (uint64_t r = 0; r < n; r++) out.otu[r] = g.old_to_new[in.otu[r]];
    otu_totals(out, view);
    out.link_a = in.link_a;
    out.link_b = in.link_b;
    out.rounds = in.rounds;
    out.link_passes = in.link_passes;
    out.long_rows = in.long_rows;
}

}  // namespace rtx

extern "C" {

int rtx_otu_graft_host(rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_graft_params p{};
    if (const int rc = rtx::graft_open("rtx_otu_graft_host", table, otu, params, out, &v, &p)) return rc;
    auto *o = new rtx_otu();
    o->graft.reset(new rtx_graft_info());
    std::vector<uint8_t> heavy;
    rtx::graft_heavy(*otu, p.boundary, heavy, *o->graft);
    const uint64_t n = v.n_entries;
    std::vector<uint32_t> parent(n, 0xFFFFFFFFu);
    if (o->graft->light_rows && o->graft->heavy_rows) {
        std::unordered_map<std::string, uint32_t> lowest;  // a string of a heavy row's ball -> the lowest such row (rows come in rank order)
        for (uint64_t y = 0; y < n; y++) {
            const uint64_t len = v.base_off[y + 1] - v.base_off[y];
            if (!heavy[y] || len == 0 || len > RTX_OTU_MAX_LEN) continue;
            rtx::ball(v.bases + v.base_off[y], len, [&](const std::string &s) { lowest.emplace(s, (uint32_t)y); });
        }
        for (uint64_t x = 0; x < n; x++) {
            const uint64_t len = v.base_off[x + 1] - v.base_off[x];
            if (heavy[x] || len == 0 || len > RTX_OTU_MAX_LEN) continue;
            uint32_t best = 0xFFFFFFFFu;
            rtx::ball(v.bases + v.base_off[x], len, [&](const std::string &s) {
                const auto it = lowest.find(s);
                if (it != lowest.end()) best = std::min(best, it->second);
            });
            parent[x] = best;
        }
    }
    rtx::graft_build(*otu, v, heavy, std::move(parent), *o);
    *out = o;
    return RTX_OK;
}

int rtx_otu_graft_view(rtx_otu *o, rtx_graft_view_t *view) {
    if (!o || !view) { rtx::set_error("rtx_otu_graft_view: null argument"); return RTX_ERR_INVALID; }
    if (!o->graft) { rtx::set_error("rtx_otu_graft_view: the object is no graft result"); return RTX_ERR_INVALID; }
    const rtx_graft_info &g = *o->graft;
    view->n_rows = o->n_rows;
    view->n_old_otus = g.old_otus;
    view->n_otus = o->n_otus;
    view->n_grafts = g.light.size();
    view->boundary = g.boundary;
    view->parent = g.parent.data();
    view->old_to_new = g.old_to_new.data();
    view->light = g.light.data();
    view->child = g.child.data();
    view->par = g.par.data();
    view->heavy = g.heavy.data();
    view->into = g.into.data();
    view->size = g.size.data();
    view->heavy_otus = g.heavy_otus;
    view->light_otus = g.light_otus;
    view->heavy_rows = g.heavy_rows;
    view->light_rows = g.light_rows;
    view->variants = g.variants;
    view->candidates = g.candidates;
    view->confirmed = g.confirmed;
    view->bloom_log2 = g.bloom_log2;
    view->test_passes = g.test_passes;
    for (int i = 0; i < 5; i++) view->seconds[i] = g.seconds[i];
    return RTX_OK;
}

int64_t rtx_otu_format_grafts(rtx_otu *o, char *buf, uint64_t cap) {
    if (!o) { rtx::set_error("rtx_otu_format_grafts: null argument"); return RTX_ERR_INVALID; }
    if (!o->graft) { rtx::set_error("rtx_otu_format_grafts: the object is no graft result"); return RTX_ERR_INVALID; }
    const rtx_graft_info &g = *o->graft;
    std::string text = "#light\tsize\tchild\tparent\theavy\tinto\n";
    char num[160];
    for (size_t i = 0; i < g.light.size(); i++) {
        snprintf(num, sizeof num, "otu%llu\t%llu\tuniq%llu\tuniq%llu\totu%llu\totu%llu\n", (unsigned long long)g.light[i] + 1, (unsigned long long)g.size[i],
                 (unsigned long long)g.child[i] + 1, (unsigned long long)g.par[i] + 1, (unsigned long long)g.heavy[i] + 1, (unsigned long long)g.into[i] + 1);
        text += num;
    }
    return rtx::hand_out("rtx_otu_format_grafts", text, buf, cap);
}

int rtx_otu_cluster_host(rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_otu_params p{};
    if (const int rc = rtx::otu_open("rtx_otu_cluster_host", table, params, out, &v, &p)) return rc;
    auto *o = new rtx_otu();
    rtx::host_links(*table, v, *o);
    rtx::host_grow(v, *o);
    rtx::otu_sums(*o, v);
    o->link_passes = 1;
    *out = o;
    return RTX_OK;
}

int rtx_otu_view(rtx_otu *o, rtx_otu_view_t *view) {
    if (!o || !view) { rtx::set_error("rtx_otu_view: null argument"); return RTX_ERR_INVALID; }
    view->n_rows = o->n_rows;
    view->n_otus = o->n_otus;
    view->n_columns = o->columns;
    view->otu = o->otu.data();
    view->seed = o->seed.data();
    view->members = o->members.data();
    view->sizes = o->sizes.data();
    view->counts = o->counts.data();
    view->n_links = o->link_a.size();
    view->link_a = o->link_a.data();
    view->link_b = o->link_b.data();
    view->rounds = o->rounds;
    view->link_passes = o->link_passes;
    view->long_rows = o->long_rows;
    return RTX_OK;
}

int rtx_otu_times(const rtx_otu *o, double seconds[4]) {
    if (!o || !seconds) { rtx::set_error("rtx_otu_times: null argument"); return RTX_ERR_INVALID; }
    for (int i = 0; i < 4; i++) seconds[i] = o->seconds[i];
    return RTX_OK;
}

void rtx_otu_destroy(rtx_otu *o) { delete o; }

int64_t rtx_otu_format_fasta(rtx_otu *o, rtx_tally_table *table, uint64_t minsize, char *buf, uint64_t cap) {
    if (!o || !table) { rtx::set_error("rtx_otu_format_fasta: null argument"); return RTX_ERR_INVALID; }
    rtx_tally_view v{};
    if (const int rc = rtx_tally_table_view(table, &v)) return rc;
    if (v.n_entries != o->n_rows) {
        rtx::set_error("rtx_otu_format_fasta: the table has %llu rows, the OTUs were made from %llu", (unsigned long long)v.n_entries, (unsigned long long)o->n_rows);
        return RTX_ERR_INVALID;
    }
    std::string text;
    char num[96];
    for (uint64_t k = 0; k < o->n_otus; k++) {
        if (o->sizes[k] < minsize) continue;
        const uint64_t r = o->seed[k];
        snprintf(num, sizeof num, ">otu%llu;size=%llu;seed=uniq%llu\n", (unsigned long long)(k + 1), (unsigned long long)o->sizes[k], (unsigned long long)(r + 1));
        text += num;
        for (uint64_t i = v.base_off[r]; i < v.base_off[r + 1]; i++) text += rtx::text_base(v.bases[i]);
        text += '\n';
    }
    return rtx::hand_out("rtx_otu_format_fasta", text, buf, cap);
}

int64_t rtx_otu_format_table(rtx_otu *o, const char *const *names, uint64_t minsize, char *buf, uint64_t cap) {
    if (!o || !names) { rtx::set_error("rtx_otu_format_table: null argument"); return RTX_ERR_INVALID; }
    const uint32_t nc = o->columns;
    std::string text = "#otu";
    for (uint32_t c = 0; c < nc; c++) {
        if (!names[c]) { rtx::set_error("rtx_otu_format_table: name %u is null", c); return RTX_ERR_INVALID; }
        text += '\t';
        text += names[c];
    }
    text += '\n';
    char num[32];
    for (uint64_t k = 0; k < o->n_otus; k++) {
        if (o->sizes[k] < minsize) continue;
        snprintf(num, sizeof num, "otu%llu", (unsigned long long)(k + 1));
        text += num;
        for (uint32_t c = 0; c < nc; c++) {
            snprintf(num, sizeof num, "\t%llu", (unsigned long long)o->counts[k * nc + c]);
            text += num;
        }
        text += '\n';
    }
    return rtx::hand_out("rtx_otu_format_table", text, buf, cap);
}

int64_t rtx_otu_format_map(rtx_otu *o, char *buf, uint64_t cap) {
    if (!o) { rtx::set_error("rtx_otu_format_map: null argument"); return RTX_ERR_INVALID; }
    std::string text;
    char num[64];
    for (uint64_t r = 0; r < o->n_rows; r++) {
        snprintf(num, sizeof num, "uniq%llu\totu%llu\n", (unsigned long long)(r + 1), (unsigned long long)(o->otu[r] + 1u));
        text += num;
    }
    return rtx::hand_out("rtx_otu_format_map", text, buf, cap);
}

}  // extern "C"

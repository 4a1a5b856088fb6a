// The consensus taxonomy of the OTUs on the host: see host_otutax.hpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__)
#endif
#include "host_otutax.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>

#include "host_tally.hpp"  // hand_out
#include "rtx_math.hpp"    // profile_step: the per-query step of the taxon profile

namespace rtx {

int otutax_open(const char *who, uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed, const rtx_lineage_records *rec,
                const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out, OtuTaxInput &in) {
    typedef unsigned long long ull;
    if (out) *out = nullptr;
    if (!out || !rec || !nodes || !nodes->node_parent || (n_rows && (!otu || !weight || !rec->kind || !rec->L || !rec->node || !rec->hund)) || (n_otus && !seed)) {
        set_error("%s: null argument", who);
        return RTX_ERR_INVALID;
    }
    const uint32_t pct = params && params->agree_pct ? params->agree_pct : 51u;
    if (pct < 51u || pct > 100u) { set_error("%s: an agreement of %u percent (51 .. 100: at most one child can qualify)", who, pct); return RTX_ERR_INVALID; }
    if (params && params->flags) { set_error("%s: flags = %u (none is defined)", who, params->flags); return RTX_ERR_INVALID; }
    if (n_rows >= 0xFFFFFFFFull) { set_error("%s: %llu rows (fewer than 2^32 - 1)", who, (ull)n_rows); return RTX_ERR_INVALID; }
    if (n_otus > n_rows) { set_error("%s: %llu OTUs of %llu rows", who, (ull)n_otus, (ull)n_rows); return RTX_ERR_INVALID; }
    const uint32_t nn = nodes->n_nodes;
    if (nn == 0 || nodes->node_parent[0] != kNoNode) { set_error("%s: node 0 is not the root", who); return RTX_ERR_INVALID; }
    // the depth of every node: breadth first, so a parent comes before its children
    std::vector<uint8_t> depth(nn, 0);
    for (uint32_t v = 1; v < nn; v++) {
        const uint32_t p = nodes->node_parent[v];
        if (p >= v) { set_error("%s: node %u has the parent %u (the nodes come breadth first)", who, v, p); return RTX_ERR_INVALID; }
        depth[v] = (uint8_t)std::min<uint32_t>(depth[p] + 1u, 255u);
    }
    in.n_rows = n_rows;
    in.n_otus = n_otus;
    in.otu = otu;
    in.seed = seed;
    in.weight = weight;
    in.rec = *rec;
    in.n_nodes = nn;
    in.parent = nodes->node_parent;
    in.agree_pct = pct;
    in.max_l = 1;
    uint64_t sum = 0;
    for (uint64_t r = 0; r < n_rows; r++) {
        if (otu[r] >= n_otus) { set_error("%s: row %llu is in OTU %u of %llu", who, (ull)r, otu[r], (ull)n_otus); return RTX_ERR_INVALID; }
        if (weight[r] == 0) { set_error("%s: row %llu has the weight 0", who, (ull)r); return RTX_ERR_INVALID; }
        if (weight[r] > ~0ull / 100u - sum) { set_error("%s: 100 x the sum of the weights does not fit 64 bits (at row %llu)", who, (ull)r); return RTX_ERR_INVALID; }
        sum += weight[r];
        const uint32_t kind = rec->kind[r], l = rec->L[r];
        if (kind > RTX_LIN_CLASSIFIED) { set_error("%s: row %llu has the kind %u", who, (ull)r, kind); return RTX_ERR_INVALID; }
        if ((l != 0u) != (kind == RTX_LIN_CLASSIFIED)) { set_error("%s: row %llu has the kind %u and L = %u (L != 0 on the classified rows, and on them alone)", who, (ull)r, kind, l); return RTX_ERR_INVALID; }
        if (l == 0u) continue;
        if (l > RTX_MAX_DEPTH || l > rec->hund_stride) { set_error("%s: row %llu has L = %u (RTX_MAX_DEPTH %u, hund_stride %u)", who, (ull)r, l, RTX_MAX_DEPTH, rec->hund_stride); return RTX_ERR_INVALID; }
        const uint32_t v = rec->node[r];
        if (v >= nn) { set_error("%s: row %llu ends at node %u of %u", who, (ull)r, v, nn); return RTX_ERR_INVALID; }
        if (depth[v] != l) { set_error("%s: row %llu has L = %u at node %u, which is at depth %u", who, (ull)r, l, v, depth[v]); return RTX_ERR_INVALID; }
        const uint8_t *h = rec->hund + r * rec->hund_stride;
        for (uint32_t d = 0; d < l; d++)
            if (h[d] > 100u) { set_error("%s: row %llu has %u hundredths at level %u", who, (ull)r, h[d], d); return RTX_ERR_INVALID; }
        in.max_l = std::max(in.max_l, l);
    }
    for (uint64_t k = 0; k < n_otus; k++)
        if (seed[k] >= n_rows) { set_error("%s: the seed of OTU %llu is row %u of %llu", who, (ull)k, seed[k], (ull)n_rows); return RTX_ERR_INVALID; }
    // the members of every OTU, rows in rank order: a counting sort
    in.mem_off.assign(n_otus + 1, 0);
    in.sizes.assign(n_otus, 0);
    for (uint64_t r = 0; r < n_rows; r++) { in.mem_off[otu[r] + 1u]++; in.sizes[otu[r]] += weight[r]; }
    for (uint64_t k = 0; k < n_otus; k++) in.mem_off[k + 1] += in.mem_off[k];
    for (uint64_t k = 0; k < n_otus; k++)  // (S_k would be 0, and every child would qualify)
        if (in.mem_off[k + 1] == in.mem_off[k]) { set_error("%s: OTU %llu has no row", who, (ull)k); return RTX_ERR_INVALID; }
    in.mem_row.resize(n_rows);
    std::vector<uint64_t> fill(in.mem_off.begin(), in.mem_off.end() - 1);
    for (uint64_t r = 0; r < n_rows; r++) in.mem_row[fill[otu[r]]++] = (uint32_t)r;
    return RTX_OK;
}

void otutax_init(rtx_otutax &t, const OtuTaxInput &in) {
    t.n_rows = in.n_rows;
    t.n_otus = in.n_otus;
    t.n_nodes = in.n_nodes;
    t.agree_pct = in.agree_pct;
    t.stride = in.max_l;
    t.sizes = in.sizes;
    t.members.resize(in.n_otus);
    for (uint64_t k = 0; k < in.n_otus; k++) t.members[k] = in.mem_off[k + 1] - in.mem_off[k];
    t.classified.assign(in.n_otus, 0);
    t.depth.assign(in.n_otus, 0);
    t.node.assign(in.n_otus, 0);
    t.seed_rel.assign(in.n_otus, 0);
    t.clade.assign(in.n_otus * t.stride, 0);
    t.conf.assign(in.n_otus * t.stride, 0);
}

namespace {

// the path a_0 .. a_{L-1} of a row, from its node up
void row_path(const OtuTaxInput &in, uint64_t r, uint32_t *path) {
    uint32_t d = in.rec.L[r];
    if (d == 0u) return;  // (no path: the node is not read)
    for (uint32_t v = in.rec.node[r]; d-- > 0u; v = in.parent[v]) path[d] = v;
}

// The definition, literally: the clade and conf of every node that a member's path holds, then the descent from the root
void host_consensus(const OtuTaxInput &in, rtx_otutax &t) {
    struct Sums { uint64_t clade = 0, conf = 0; };
    std::unordered_map<uint32_t, Sums> at;
    uint32_t path[RTX_MAX_DEPTH], cons[RTX_MAX_DEPTH];
    for (uint64_t k = 0; k < in.n_otus; k++) {
        at.clear();
        for (uint64_t m = in.mem_off[k]; m < in.mem_off[k + 1]; m++) {
            const uint64_t r = in.mem_row[m];
            const uint32_t l = in.rec.L[r];
            if (in.rec.kind[r] == RTX_LIN_CLASSIFIED) t.classified[k] += in.weight[r];
            row_path(in, r, path);
            for (uint32_t d = 0; d < l; d++) {
                Sums &s = at[path[d]];
                s.clade += in.weight[r];
                s.conf += in.weight[r] * in.rec.hund[r * in.rec.hund_stride + d];
            }
        }
        uint32_t cur = 0, depth = 0;
        for (bool more = true; more && depth < t.stride;) {
            more = false;
            for (const auto &e : at)  // the children of `cur` that hold a member
                if (in.parent[e.first] == cur && e.second.clade * 100u >= (uint64_t)in.agree_pct * in.sizes[k]) {
                    t.clade[k * t.stride + depth] = e.second.clade;
                    t.conf[k * t.stride + depth] = e.second.conf;
                    cons[depth++] = cur = e.first;
                    more = true;
                    break;  // (P > 50: no second one)
                }
        }
        t.depth[k] = depth;
        t.node[k] = cur;
        const uint64_t s = in.seed[k];
        const uint32_t ls = in.rec.L[s];
        row_path(in, s, path);
        uint32_t same = 0;
        while (same < ls && same < depth && path[same] == cons[same]) same++;
        t.seed_rel[k] = same < ls && same < depth ? 3u : (ls == depth ? 0u : (ls > depth ? 1u : 2u));
    }
}

}  // namespace
}  // namespace rtx

extern "C" int rtx_otu_taxonomy_host(uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed, const rtx_lineage_records *records,
                                     const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out) {
    rtx::OtuTaxInput in;
    if (const int rc = rtx::otutax_open("rtx_otu_taxonomy_host", n_rows, otu, weight, n_otus, seed, records, nodes, params, out, in)) return rc;
    auto *t = new rtx_otutax();
    rtx::otutax_init(*t, in);
    rtx::host_consensus(in, *t);
    *out = t;
    return RTX_OK;
}

extern "C" int rtx_otu_taxonomy_view(rtx_otutax *t, rtx_otu_taxonomy_view_t *v) {
    if (!t || !v) { rtx::set_error("rtx_otu_taxonomy_view: null argument"); return RTX_ERR_INVALID; }
    v->n_rows = t->n_rows;
    v->n_otus = t->n_otus;
    v->n_nodes = t->n_nodes;
    v->agree_pct = t->agree_pct;
    v->stride = t->stride;
    v->sizes = t->sizes.data();
    v->members = t->members.data();
    v->classified = t->classified.data();
    v->depth = t->depth.data();
    v->node = t->node.data();
    v->seed_rel = t->seed_rel.data();
    v->clade = t->clade.data();
    v->conf = t->conf.data();
    v->packed_waves = t->packed_waves;
    v->big_otus = t->big_otus;
    return RTX_OK;
}

extern "C" int rtx_otu_taxonomy_times(const rtx_otutax *t, double seconds[4]) {
    if (!t || !seconds) { rtx::set_error("rtx_otu_taxonomy_times: null argument"); return RTX_ERR_INVALID; }
    for (int i = 0; i < 4; i++) seconds[i] = t->seconds[i];
    return RTX_OK;
}

extern "C" void rtx_otu_taxonomy_destroy(rtx_otutax *t) { delete t; }

extern "C" int64_t rtx_otu_taxonomy_format(rtx_otutax *t, const rtx_tree *tree, uint64_t minsize, char *buf, uint64_t cap) {
    typedef unsigned long long ull;
    if (!t || !tree) { rtx::set_error("rtx_otu_taxonomy_format: null argument"); return RTX_ERR_INVALID; }
    const rtx::FlatNodes &f = tree->flat;
    if (f.size() != t->n_nodes) { rtx::set_error("rtx_otu_taxonomy_format: the tree has %u nodes, the taxonomy was made over %u", f.size(), t->n_nodes); return RTX_ERR_INVALID; }
    std::string text = "#otu\tsize\tmembers\tclassified\tdepth\ttaxon\tlineage\tsupport\tmean_conf\tseed\n";
    char num[128];
    for (uint64_t k = 0; k < t->n_otus; k++) {
        const uint64_t S = t->sizes[k];
        if (S < minsize) continue;
        const uint32_t depth = t->depth[k], v = t->node[k];
        snprintf(num, sizeof num, "otu%llu\t%llu\t%llu\t%llu\t%u\t", (ull)(k + 1), (ull)S, (ull)t->members[k], (ull)t->classified[k], depth);
        text += num;
        if (depth == 0) {
            text += "-\t-\t-\t-";
        } else {
            if (v >= f.size() || f.depth[v] != depth || f.begin[v] >= tree->lineages.size()) {
                rtx::set_error("rtx_otu_taxonomy_format: OTU %llu ends at node %u with depth %u, which this tree does not hold", (ull)k, v, depth);
                return RTX_ERR_INVALID;
            }
            const std::string &lin = tree->lineages[f.begin[v]];
            size_t end = 0, start = 0;  // the first depth levels: [0, end), the last of them [start, end) (rtx_profile_format)
            for (uint32_t d = 0; d < depth; d++) {
                start = d ? end + 1 : 0;
                const size_t c = start <= lin.size() ? lin.find(',', start) : std::string::npos;
                end = c == std::string::npos ? lin.size() : c;
            }
            start = std::min(start, lin.size());
            text.append(lin, start, end - start);
            text += '\t';
            text.append(lin, 0, end);
            text += '\t';
            for (uint32_t d = 0; d < depth; d++) {
                const uint64_t pct = (t->clade[k * t->stride + d] * 10000u + S / 2u) / S;
                snprintf(num, sizeof num, "%s%llu.%02llu", d ? "," : "", (ull)(pct / 100u), (ull)(pct % 100u));
                text += num;
            }
            text += '\t';
            for (uint32_t d = 0; d < depth; d++) {
                const uint64_t c = t->clade[k * t->stride + d], mean = (t->conf[k * t->stride + d] + c / 2u) / c;
                snprintf(num, sizeof num, "%s%llu.%02llu", d ? "," : "", (ull)(mean / 100u), (ull)(mean % 100u));
                text += num;
            }
        }
        text += '\t';
        text += "=<>x"[t->seed_rel[k] & 3u];
        text += '\n';
    }
    return rtx::hand_out("rtx_otu_taxonomy_format", text, buf, cap);
}

extern "C" int rtx_result_best_lineages(const rtx_tree *tree, const rtx_result_view *res, const uint32_t *exact_ids, const uint64_t *exact_off, uint32_t cutoff,
                                        uint32_t flags, uint8_t *kind, uint8_t *L, uint32_t *node, uint8_t *hund, uint32_t hund_stride) {
    using namespace rtx;
    const char *who = "rtx_result_best_lineages";
    if (!tree || !res || !kind || !L || !node || !hund) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (cutoff < 1u || cutoff > 100u) { set_error("%s: the cutoff is %u hundredths, not 1 .. 100", who, cutoff); return RTX_ERR_INVALID; }
    if (flags & ~(RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE)) { set_error("%s: unknown flags %#x", who, flags); return RTX_ERR_INVALID; }
    if (!exact_ids != !exact_off) { set_error("%s: exact_ids and exact_off go together (or both NULL)", who); return RTX_ERR_INVALID; }
    const FlatNodes &f = tree->flat;
    const uint32_t nn = f.size();
    if (hund_stride < f.max_depth || hund_stride == 0u) { set_error("%s: hund_stride = %u, the tree's deepest lineage has %u levels", who, hund_stride, f.max_depth); return RTX_ERR_INVALID; }
    const uint64_t nq = res->n_queries, nr = res->n_rows;
    const uint32_t D = res->row_conf_stride ? res->row_conf_stride : RTX_MAX_DEPTH;
    // the row fields as bytes: those of the view, or converted (rtx_result_pack)
    std::vector<uint8_t> depth_u8, hund_u8;
    const uint8_t *row_depth = res->row_depth_u8, *row_hund = res->row_conf_hundredths;
    if (!row_depth || !row_hund || !res->row_conf_stride) {
        depth_u8.resize(nr);
        hund_u8.assign(nr * D, 0);
        for (uint64_t r = 0; r < nr; r++) {
            if (res->row_depth[r] > D) { set_error("%s: row %llu has the depth %u (stride %u)", who, (unsigned long long)r, res->row_depth[r], D); return RTX_ERR_INVALID; }
            depth_u8[r] = (uint8_t)res->row_depth[r];
            for (uint32_t d = 0; d < res->row_depth[r]; d++) hund_u8[r * D + d] = (uint8_t)std::lrint(res->row_conf[r * D + d] * 100.0);
        }
        row_depth = depth_u8.data();
        row_hund = hund_u8.data();
    }
    std::vector<uint8_t> node_depth(nn);
    for (uint32_t v = 0; v < nn; v++) node_depth[v] = (uint8_t)f.depth[v];
    // the Taxon node of every reference: the nodes come breadth first, so the deepest Taxon node over a reference is the last one written
    const uint32_t n_refs = (uint32_t)tree->lineages.size();
    std::vector<uint32_t> leaf(n_refs ? n_refs : 1u, kNoNode);
    for (uint32_t v = 0; v < nn; v++)
        if (f.type[v] == kTaxon && f.end[v] <= n_refs && f.begin[v] <= f.end[v]) std::fill(leaf.begin() + f.begin[v], leaf.begin() + f.end[v], v);
    const ProfileSrc src{res->status, res->row_count, reinterpret_cast<const unsigned long long *>(res->row_begin), res->row_node, row_depth, row_hund, D,
                         f.parent.data(), node_depth.data(), leaf.data(), nn, n_refs};
    const bool override_ok = exact_off && !(flags & (RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE));
    for (uint64_t q = 0; q < nq; q++) {
        if (res->status[q] == RTX_Q_OK && res->row_count[q]) {
            const uint64_t row = res->row_begin[q];
            if (row >= nr || row_depth[row] > D) { set_error("%s: query %llu begins at row %llu of %llu", who, (unsigned long long)q, (unsigned long long)row, (unsigned long long)nr); return RTX_ERR_INVALID; }
        }
        const uint32_t one = override_ok && exact_off[q + 1] - exact_off[q] == 1u ? exact_ids[exact_off[q]] : kTextNoOverride;
        const ProfileStep st = profile_step(src, q, one, cutoff);
        if (st.L > hund_stride) { set_error("%s: query %llu reaches %u levels (hund_stride %u)", who, (unsigned long long)q, st.L, hund_stride); return RTX_ERR_INVALID; }
        kind[q] = (uint8_t)st.kind;
        L[q] = (uint8_t)st.L;
        node[q] = st.L ? st.node : 0u;
        uint8_t *h = hund + q * hund_stride;
        for (uint32_t d = 0; d < hund_stride; d++) h[d] = d < st.L ? (uint8_t)st.at(d) : 0u;
    }
    return RTX_OK;
}

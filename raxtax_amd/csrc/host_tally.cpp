// The table of distinct reads on the host: see host_tally.hpp.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__)
#endif
#include "host_tally.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "rtx_math.hpp"  // text_base: the letters of the `.tsv` sequence column

namespace rtx {

uint64_t tally_table_entry(rtx_tally_table &t, const uint8_t *seq, uint64_t len) {
    std::string key(reinterpret_cast<const char *>(seq), len);
    auto it = t.index.find(key);
    if (it != t.index.end()) return it->second;
    const uint64_t e = t.seqs.size();
    t.index.emplace(key, e);
    t.seqs.push_back(std::move(key));
    t.counts.resize(t.counts.size() + t.columns, 0);
    t.laid_out = false;
    return e;
}

int tally_check_chunk(const char *who, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample, const uint32_t *weight, uint32_t columns,
                      uint64_t so_far, uint64_t *counted) {
    if (const int rc = check_reads(who, n, base_off, bases, 0xFFFFFFFFull)) return rc;  // (an entry keeps its length in 32 bits)
    uint64_t sum = 0;
    for (uint64_t q = 0; q < n; q++) {
        const uint32_t w = weight ? weight[q] : 1u;
        if (w == 0u || base_off[q + 1] == base_off[q]) continue;
        if (sample && sample[q] >= columns) {
            set_error("%s: read %llu has sample %u of %u", who, (unsigned long long)q, sample[q], columns);
            return RTX_ERR_INVALID;
        }
        sum += w;
    }
    if (so_far + sum > 0xFFFFFFFFull) {
        set_error("%s: a counted weight of %llu on top of %llu: more than 2^32 - 1 in one object, a cell could wrap", who, (unsigned long long)sum, (unsigned long long)so_far);
        return RTX_ERR_INVALID;
    }
    *counted = sum;
    return RTX_OK;
}

namespace {

// the rows of the view: total size descending, then bytes ascending
void lay_out(rtx_tally_table &t) {
    if (t.laid_out) return;
    const uint64_t ne = t.seqs.size();
    const uint32_t nc = t.columns;
    std::vector<uint64_t> size(ne, 0), order(ne);
    for (uint64_t e = 0; e < ne; e++) size[e] = std::accumulate(t.counts.begin() + e * nc, t.counts.begin() + (e + 1) * nc, (uint64_t)0);
    std::iota(order.begin(), order.end(), (uint64_t)0);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return size[a] != size[b] ? size[a] > size[b] : t.seqs[a] < t.seqs[b]; });  // (codes are below 128: char order is byte order)
    t.v_bases.clear();
    t.v_off.assign(1, 0);
    t.v_counts.resize(ne * nc);
    t.v_sizes.resize(ne);
    t.v_first = order;
    for (uint64_t r = 0; r < ne; r++) {
        const uint64_t e = order[r];
        t.v_bases.insert(t.v_bases.end(), t.seqs[e].begin(), t.seqs[e].end());
        t.v_off.push_back(t.v_bases.size());
        std::copy(t.counts.begin() + e * nc, t.counts.begin() + (e + 1) * nc, t.v_counts.begin() + r * nc);
        t.v_sizes[r] = size[e];
    }
    t.laid_out = true;
}

}  // namespace

// the two-pass protocol of the formatters (rtx_profile_format)
int64_t hand_out(const char *who, const std::string &text, char *buf, uint64_t cap) {
    if (!buf) return (int64_t)text.size();
    if (cap < text.size()) {
        set_error("%s: buffer of %llu bytes, need %llu", who, (unsigned long long)cap, (unsigned long long)text.size());
        return -(int64_t)text.size() - (int64_t)RTX_NEED_BASE;
    }
    memcpy(buf, text.data(), text.size());
    return (int64_t)text.size();
}

}  // namespace rtx

extern "C" {

int rtx_tally_table_create(uint32_t n_samples, rtx_tally_table **out) {
    if (!out) { rtx::set_error("rtx_tally_table_create: null argument"); return RTX_ERR_INVALID; }
    auto *t = new rtx_tally_table();
    t->n_samples = n_samples;
    t->columns = std::max(1u, n_samples);
    *out = t;
    return RTX_OK;
}

void rtx_tally_table_destroy(rtx_tally_table *table) { delete table; }

int rtx_tally_table_add(rtx_tally_table *table, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample, const uint32_t *weight) {
    if (!table) { rtx::set_error("rtx_tally_table_add: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (!base_off) { rtx::set_error("rtx_tally_table_add: null argument"); return RTX_ERR_INVALID; }
    uint64_t counted = 0;
    if (const int rc = rtx::tally_check_chunk("rtx_tally_table_add", n, bases, base_off, sample, weight, table->columns, 0, &counted)) return rc;
    for (uint64_t q = 0; q < n; q++) {
        const uint32_t w = weight ? weight[q] : 1u;
        const uint64_t len = base_off[q + 1] - base_off[q];
        if (w == 0u || len == 0) continue;
        const uint64_t e = rtx::tally_table_entry(*table, bases + base_off[q], len);
        table->counts[e * table->columns + (sample ? sample[q] : 0u)] += w;
    }
    table->reads += counted;
    table->laid_out = false;
    return RTX_OK;
}

int rtx_tally_table_merge(rtx_tally_table *const *tables, uint32_t n, rtx_tally_table **out) {
    if (!tables || n == 0 || !out) { rtx::set_error("rtx_tally_table_merge: null argument"); return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {
        if (!tables[i]) { rtx::set_error("rtx_tally_table_merge: table %u is null", i); return RTX_ERR_INVALID; }
        if (tables[i]->columns != tables[0]->columns) {
            rtx::set_error("rtx_tally_table_merge: table %u has %u column(s), table 0 has %u", i, tables[i]->columns, tables[0]->columns);
            return RTX_ERR_INVALID;
        }
    }
    auto *t = new rtx_tally_table();
    t->n_samples = tables[0]->n_samples;
    const uint32_t nc = t->columns = tables[0]->columns;
    for (uint32_t i = 0; i < n; i++) {
        const rtx_tally_table &s = *tables[i];
        for (uint64_t e = 0; e < s.seqs.size(); e++) {
            const uint64_t d = rtx::tally_table_entry(*t, reinterpret_cast<const uint8_t *>(s.seqs[e].data()), s.seqs[e].size());
            for (uint32_t c = 0; c < nc; c++) t->counts[d * nc + c] += s.counts[e * nc + c];
        }
        t->reads += s.reads;
        t->overflow_reads += s.overflow_reads;
    }
    *out = t;
    return RTX_OK;
}

int rtx_tally_table_view(rtx_tally_table *table, rtx_tally_view *view) {
    if (!table || !view) { rtx::set_error("rtx_tally_table_view: null argument"); return RTX_ERR_INVALID; }
    rtx::lay_out(*table);
    view->n_entries = table->seqs.size();
    view->n_columns = table->columns;
    view->bases = table->v_bases.data();
    view->base_off = table->v_off.data();
    view->counts = table->v_counts.data();
    view->sizes = table->v_sizes.data();
    view->first = table->v_first.data();
    view->totals[0] = table->reads;
    view->totals[1] = table->seqs.size();
    view->totals[2] = table->overflow_reads;
    return RTX_OK;
}

int64_t rtx_tally_format_fasta(rtx_tally_table *table, uint64_t minsize, char *buf, uint64_t cap) {
    if (!table) { rtx::set_error("rtx_tally_format_fasta: null argument"); return RTX_ERR_INVALID; }
    rtx::lay_out(*table);
    std::string text;
    char num[64];
    for (uint64_t r = 0; r < table->v_sizes.size(); r++) {
        if (table->v_sizes[r] < minsize) continue;
        snprintf(num, sizeof num, ">uniq%llu;size=%llu\n", (unsigned long long)(r + 1), (unsigned long long)table->v_sizes[r]);
        text += num;
        for (uint64_t i = table->v_off[r]; i < table->v_off[r + 1]; i++) text += rtx::text_base(table->v_bases[i]);
        text += '\n';
    }
    return rtx::hand_out("rtx_tally_format_fasta", text, buf, cap);
}

int64_t rtx_tally_format_table(rtx_tally_table *table, const char *const *names, uint64_t minsize, char *buf, uint64_t cap) {
    if (!table || !names) { rtx::set_error("rtx_tally_format_table: null argument"); return RTX_ERR_INVALID; }
    rtx::lay_out(*table);
    const uint32_t nc = table->columns;
    std::string text = "#uniq";
    for (uint32_t c = 0; c < nc; c++) {
        if (!names[c]) { rtx::set_error("rtx_tally_format_table: name %u is null", c); return RTX_ERR_INVALID; }
        text += '\t';
        text += names[c];
    }
    text += '\n';
    char num[32];
    for (uint64_t r = 0; r < table->v_sizes.size(); r++) {
        if (table->v_sizes[r] < minsize) continue;
        snprintf(num, sizeof num, "uniq%llu", (unsigned long long)(r + 1));
        text += num;
        for (uint32_t c = 0; c < nc; c++) {
            snprintf(num, sizeof num, "\t%llu", (unsigned long long)table->v_counts[r * nc + c]);
            text += num;
        }
        text += '\n';
    }
    return rtx::hand_out("rtx_tally_format_table", text, buf, cap);
}

}  // extern "C"

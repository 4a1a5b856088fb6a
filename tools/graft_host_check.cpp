// A stand-alone check of the host side of the fastidious grafting (raxtax_amd/csrc/host_otu.cpp: rtx_otu_graft_host, rtx_otu_graft_view,
// rtx_otu_format_grafts) for the sanitizers: the balls are built in place over strings of the exact lengths, so they are built with
// -fsanitize=address,undefined together with this main.  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/graft_host_check.cpp \
//       raxtax_amd/csrc/host_otu.cpp raxtax_amd/csrc/host_tally.cpp -o graft_host_check && ./graft_host_check
// The parents are also held against a pair-by-pair statement written here: the Levenshtein distance of two rows over A, C, G, T.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "raxtax_hip.h"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "graft_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static size_t distance(const std::string &a, const std::string &b) {
    // the band |i - j| <= 2 of the table: what lies outside it is above 2 anyway (the callers ask "at most 2?")
    const size_t far = 1000000;
    std::vector<size_t> prev(b.size() + 1, far), cur(b.size() + 1, far);
    for (size_t j = 0; j <= std::min<size_t>(2, b.size()); j++) prev[j] = j;
    for (size_t i = 1; i <= a.size(); i++) {
        const size_t lo = i > 2 ? i - 2 : 0, hi = std::min(b.size(), i + 2);
        if (lo > 0) cur[lo - 1] = far;
        for (size_t j = lo; j <= hi; j++) cur[j] = j == 0 ? i : std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])});
        if (hi < b.size()) cur[hi + 1] = far;
        prev.swap(cur);
    }
    return prev[b.size()];
}

int main() {
    std::mt19937 rng(13);
    std::vector<std::string> pool;
    std::vector<uint32_t> weight;
    for (uint32_t len : {1u, 2u, 7u, 8u, 9u, 16u, 17u, 64u, 65u, 600u, 4095u, 4096u, 4097u}) {
        std::string base(len, '\0');
        for (char &c : base) c = (char)(1u << (rng() % 4));
        pool.push_back(base);
        weight.push_back(5);
        for (int k = 0; k < 8; k++) {  // one to three steps away, over A, C, G, T
            std::string v = base;
            for (int e = 0, ne = 1 + k % 3; e < ne; e++) {
                const size_t i = rng() % v.size();
                switch (rng() % 3) {
                    case 0: v[i] = (char)(1u << (rng() % 4)); break;
                    case 1: if (v.size() > 1) v.erase(i, 1); break;
                    default: v.insert(i + rng() % 2, 1, (char)(1u << (rng() % 4)));
                }
            }
            pool.push_back(v);
            weight.push_back(1);
        }
    }
    rtx_tally_table *table = nullptr;
    CHECK(rtx_tally_table_create(0, &table) == RTX_OK);
    {
        const uint64_t n = pool.size();
        uint64_t total = 0;
        for (const std::string &s : pool) total += s.size();
        std::unique_ptr<uint8_t[]> bases(new uint8_t[total]);  // exact lengths: a read past the end is the sanitizer's
        std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
        uint64_t at = 0;
        for (uint64_t q = 0; q < n; q++) {
            off[q] = at;
            memcpy(bases.get() + at, pool[q].data(), pool[q].size());
            at += pool[q].size();
        }
        off[n] = at;
        CHECK(rtx_tally_table_add(table, n, bases.get(), off.get(), nullptr, weight.data()) == RTX_OK);
    }
    rtx_tally_view tv{};
    CHECK(rtx_tally_table_view(table, &tv) == RTX_OK);
    rtx_otu *o = nullptr, *g = nullptr;
    CHECK(rtx_otu_cluster_host(table, nullptr, &o) == RTX_OK);
    rtx_otu_view_t ov{};
    CHECK(rtx_otu_view(o, &ov) == RTX_OK);
    rtx_graft_view_t gv{};
    CHECK(rtx_otu_graft_view(o, &gv) == RTX_ERR_INVALID && rtx_otu_format_grafts(o, nullptr, 0) == RTX_ERR_INVALID);
    rtx_graft_params bad{0, 0, 1, 0, 0};
    CHECK(rtx_otu_graft_host(table, o, &bad, &g) == RTX_ERR_INVALID && g == nullptr);
    bad = rtx_graft_params{0, 41, 0, 0, 0};
    CHECK(rtx_otu_graft_host(table, o, &bad, &g) == RTX_ERR_INVALID && g == nullptr);
    CHECK(rtx_otu_graft_host(table, o, nullptr, &g) == RTX_OK);
    CHECK(rtx_otu_graft_view(g, &gv) == RTX_OK);
    CHECK(gv.n_rows == tv.n_entries && gv.n_old_otus == ov.n_otus && gv.boundary == 3 && gv.heavy_otus + gv.light_otus == ov.n_otus && gv.n_otus + gv.n_grafts == ov.n_otus);
    std::vector<std::string> rows;
    for (uint64_t r = 0; r < tv.n_entries; r++) rows.emplace_back(reinterpret_cast<const char *>(tv.bases) + tv.base_off[r], tv.base_off[r + 1] - tv.base_off[r]);
    // the parents, pair by pair
    uint64_t with_parent = 0;
    for (uint64_t x = 0; x < rows.size(); x++) {
        uint32_t want = 0xFFFFFFFFu;
        const bool light = ov.sizes[ov.otu[x]] < 3;
        if (light && rows[x].size() <= RTX_OTU_MAX_LEN)
            for (uint64_t y = 0; y < rows.size() && want == 0xFFFFFFFFu; y++) {
                if (ov.sizes[ov.otu[y]] < 3 || rows[y].size() > RTX_OTU_MAX_LEN) continue;
                const size_t la = rows[x].size(), lb = rows[y].size();
                if ((la > lb ? la - lb : lb - la) <= 2 && distance(rows[x], rows[y]) <= 2) want = (uint32_t)y;
            }
        CHECK(gv.parent[x] == want);
        with_parent += want != 0xFFFFFFFFu;
    }
    CHECK(with_parent > 30 && gv.n_grafts > 20);
    rtx_otu_view_t nv{};
    CHECK(rtx_otu_view(g, &nv) == RTX_OK && nv.n_otus == gv.n_otus && nv.n_links == ov.n_links && nv.long_rows == ov.long_rows);
    uint64_t members = 0, size = 0;
    for (uint64_t k = 0; k < nv.n_otus; k++) {
        CHECK(nv.otu[nv.seed[k]] == k && (k == 0 || nv.seed[k] > nv.seed[k - 1]));
        members += nv.members[k];
        size += nv.sizes[k];
    }
    CHECK(members == nv.n_rows && size == tv.totals[0]);
    for (uint64_t k = 0; k < gv.n_old_otus; k++) CHECK(gv.old_to_new[k] < nv.n_otus && nv.otu[ov.seed[k]] == gv.old_to_new[k]);
    for (uint64_t i = 0; i < gv.n_grafts; i++) {
        CHECK((i == 0 || gv.light[i] > gv.light[i - 1]) && ov.otu[gv.child[i]] == gv.light[i] && gv.parent[gv.child[i]] == gv.par[i]);
        CHECK(ov.otu[gv.par[i]] == gv.heavy[i] && gv.old_to_new[gv.heavy[i]] == gv.into[i] && gv.old_to_new[gv.light[i]] == gv.into[i] && gv.size[i] == ov.sizes[gv.light[i]]);
    }
    // the formatter into buffers of exactly `need` bytes, and one byte less; the other formatters take the object
    const int64_t need = rtx_otu_format_grafts(g, nullptr, 0);
    CHECK(need > 0);
    std::unique_ptr<char[]> buf(new char[(size_t)need]);
    CHECK(rtx_otu_format_grafts(g, buf.get(), (uint64_t)need) == need && buf[(size_t)need - 1] == '\n');
    CHECK(rtx_otu_format_grafts(g, buf.get(), (uint64_t)need - 1) == -need - (int64_t)RTX_NEED_BASE);
    CHECK(rtx_otu_format_fasta(g, table, 1, nullptr, 0) > 0 && rtx_otu_format_map(g, nullptr, 0) > 0);
    // B = 1: the input's clustering
    rtx_otu *one = nullptr;
    rtx_graft_params b1{1, 0, 0, 0, 0};
    CHECK(rtx_otu_graft_host(table, o, &b1, &one) == RTX_OK && rtx_otu_graft_view(one, &gv) == RTX_OK && gv.n_grafts == 0 && gv.n_otus == ov.n_otus);
    rtx_otu_destroy(one);
    // an empty table
    rtx_tally_table *none = nullptr;
    rtx_otu *eo = nullptr, *eg = nullptr;
    CHECK(rtx_tally_table_create(0, &none) == RTX_OK && rtx_otu_cluster_host(none, nullptr, &eo) == RTX_OK && rtx_otu_graft_host(none, eo, nullptr, &eg) == RTX_OK);
    CHECK(rtx_otu_graft_host(table, eo, nullptr, &one) == RTX_ERR_INVALID);  // (another table's object)
    CHECK(rtx_otu_graft_view(eg, &gv) == RTX_OK && gv.n_rows == 0 && gv.n_grafts == 0);
    rtx_otu_destroy(eg);
    rtx_otu_destroy(eo);
    rtx_tally_table_destroy(none);
    const uint64_t n_grafts = rtx_otu_graft_view(g, &gv) == RTX_OK ? gv.n_grafts : 0;
    printf("graft_host_check: ok (%llu rows, %llu OTUs, %llu grafts, %llu left)\n", (unsigned long long)rows.size(), (unsigned long long)ov.n_otus, (unsigned long long)n_grafts,
           (unsigned long long)nv.n_otus);
    rtx_otu_destroy(g);
    rtx_otu_destroy(o);
    rtx_tally_table_destroy(table);
    return 0;
}

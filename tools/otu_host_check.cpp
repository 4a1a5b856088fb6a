// A stand-alone check of the host side of the OTUs of a run (raxtax_amd/csrc/host_otu.cpp: rtx_otu_cluster_host, rtx_otu_view and the three
// formatters) for the sanitizers: the variants are built in place over strings of the exact lengths and the growth walks index arrays, so
// they are built with -fsanitize=address,undefined together with this main.  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/otu_host_check.cpp \
//       raxtax_amd/csrc/host_otu.cpp raxtax_amd/csrc/host_tally.cpp -o otu_host_check && ./otu_host_check
// The links are also held against a pair-by-pair statement of the definition written here.
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

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "otu_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static bool plain(uint8_t c) { return c == 1 || c == 2 || c == 4 || c == 8; }

static bool linked(const std::string &a, const std::string &b) {
    if (a.size() > RTX_OTU_MAX_LEN || b.size() > RTX_OTU_MAX_LEN) return false;
    if (a.size() == b.size()) {
        size_t diff = 0, at = 0;
        for (size_t i = 0; i < a.size(); i++)
            if (a[i] != b[i]) { diff++; at = i; }
        return diff == 1 && (plain((uint8_t)a[at]) || plain((uint8_t)b[at]));
    }
    const std::string &l = a.size() > b.size() ? a : b, &s = a.size() > b.size() ? b : a;
    if (l.size() != s.size() + 1) return false;
    size_t i = 0;
    while (i < s.size() && l[i] == s[i]) i++;
    return l.compare(i + 1, std::string::npos, s, i, std::string::npos) == 0;
}

int main() {
    std::mt19937 rng(11);
    std::vector<std::string> pool;
    for (uint32_t len : {1u, 2u, 7u, 8u, 9u, 16u, 17u, 64u, 65u, 4096u, 4097u}) {
        std::string base(len, '\0');
        for (char &c : base) c = (char)(1u << (rng() % 4));
        pool.push_back(base);
        for (int k = 0; k < 6; k++) {  // one and two steps away, ambiguity codes among them
            std::string v = pool[pool.size() - 1 - (size_t)(rng() % (k + 1))];
            const size_t i = rng() % v.size();
            switch (rng() % 4) {
                case 0: v[i] = (char)(1u << (rng() % 4)); break;
                case 1: v[i] = (char)(rng() % 2 ? 15 : 5); break;
                case 2: if (v.size() > 1) v.erase(i, 1); break;
                default: v.insert(i, 1, (char)(1u << (rng() % 4)));
            }
            pool.push_back(v);
        }
    }
    const uint32_t ns = 2;
    rtx_tally_table *table = nullptr;
    CHECK(rtx_tally_table_create(ns, &table) == RTX_OK);
    {
        const uint64_t n = pool.size();
        uint64_t total = 0;
        for (const std::string &s : pool) total += s.size();
        std::unique_ptr<uint8_t[]> bases(new uint8_t[total]);  // exact lengths: a read past the end is the sanitizer's
        std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
        std::unique_ptr<uint32_t[]> sample(new uint32_t[n]), weight(new uint32_t[n]);
        uint64_t at = 0;
        for (uint64_t q = 0; q < n; q++) {
            off[q] = at;
            memcpy(bases.get() + at, pool[q].data(), pool[q].size());
            at += pool[q].size();
            sample[q] = (uint32_t)(rng() % ns);
            weight[q] = 1u + (uint32_t)(rng() % 3);  // (ties in size: the plateaus of the growth)
        }
        off[n] = at;
        CHECK(rtx_tally_table_add(table, n, bases.get(), off.get(), sample.get(), weight.get()) == RTX_OK);
    }
    rtx_tally_view tv{};
    CHECK(rtx_tally_table_view(table, &tv) == RTX_OK);
    rtx_otu *o = nullptr;
    rtx_otu_params bad{2, 0, 0};
    CHECK(rtx_otu_cluster_host(table, &bad, &o) == RTX_ERR_INVALID && o == nullptr);
    CHECK(rtx_otu_cluster_host(table, nullptr, &o) == RTX_OK);
    rtx_otu_view_t v{};
    CHECK(rtx_otu_view(o, &v) == RTX_OK);
    CHECK(v.n_rows == tv.n_entries && v.n_columns == ns && v.n_otus >= 1 && v.n_otus <= v.n_rows);
    std::vector<std::string> rows;
    for (uint64_t r = 0; r < tv.n_entries; r++) rows.emplace_back(reinterpret_cast<const char *>(tv.bases) + tv.base_off[r], tv.base_off[r + 1] - tv.base_off[r]);
    uint64_t l = 0, long_rows = 0;
    for (uint64_t a = 0; a < rows.size(); a++) {
        long_rows += rows[a].size() > RTX_OTU_MAX_LEN;
        for (uint64_t b = a + 1; b < rows.size(); b++)
            if (linked(rows[a], rows[b])) {
                CHECK(l < v.n_links && v.link_a[l] == a && v.link_b[l] == b);
                l++;
            }
    }
    CHECK(l == v.n_links && l > 20 && long_rows == v.long_rows && long_rows >= 1);
    uint64_t members = 0, size = 0;
    for (uint64_t k = 0; k < v.n_otus; k++) {
        CHECK(v.otu[v.seed[k]] == k && (k == 0 || v.seed[k] > v.seed[k - 1]));
        members += v.members[k];
        size += v.sizes[k];
        uint64_t sum = 0;
        for (uint32_t c = 0; c < ns; c++) sum += v.counts[k * ns + c];
        CHECK(sum == v.sizes[k]);
    }
    CHECK(members == v.n_rows && size == tv.totals[0]);
    const uint64_t n_otus = v.n_otus;
    for (uint64_t r = 0; r < v.n_rows; r++) CHECK(v.otu[r] < v.n_otus && v.seed[v.otu[r]] <= r);
    // the three formatters into buffers of exactly `need` bytes, and one byte less
    const char *names[ns] = {"s0", "s1"};
    for (int f = 0; f < 3; f++) {
        auto call = [&](char *buf, uint64_t cap) {
            return f == 0 ? rtx_otu_format_fasta(o, table, 2, buf, cap) : f == 1 ? rtx_otu_format_table(o, names, 2, buf, cap) : rtx_otu_format_map(o, buf, cap);
        };
        const int64_t need = call(nullptr, 0);
        CHECK(need > 0);
        std::unique_ptr<char[]> buf(new char[(size_t)need]);
        CHECK(call(buf.get(), (uint64_t)need) == need);
        CHECK(buf[(size_t)need - 1] == '\n');
        CHECK(call(buf.get(), (uint64_t)need - 1) == -need - (int64_t)RTX_NEED_BASE);
    }
    rtx_otu_destroy(o);
    // an empty table
    rtx_tally_table *none = nullptr;
    CHECK(rtx_tally_table_create(0, &none) == RTX_OK && rtx_otu_cluster_host(none, nullptr, &o) == RTX_OK);
    CHECK(rtx_otu_view(o, &v) == RTX_OK && v.n_rows == 0 && v.n_otus == 0 && v.n_links == 0 && rtx_otu_format_map(o, nullptr, 0) == 0);
    rtx_otu_destroy(o);
    rtx_tally_table_destroy(none);
    rtx_tally_table_destroy(table);
    printf("otu_host_check: ok (%llu rows, %llu links, %llu OTUs)\n", (unsigned long long)rows.size(), (unsigned long long)l, (unsigned long long)n_otus);
    return 0;
}

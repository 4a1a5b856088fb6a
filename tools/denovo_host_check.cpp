// A stand-alone check of the host side of the de novo chimera check (raxtax_amd/csrc/host_denovo.cpp: rtx_denovo_check_host, rtx_denovo_view
// and the three formatters) for the sanitizers: the entries are gathered through index arrays, the windows are read from sequences of the
// exact lengths and the parents are walked by entry index, so they are built with -fsanitize=address,undefined together with this main.
// Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/denovo_host_check.cpp \
//       raxtax_amd/csrc/host_denovo.cpp raxtax_amd/csrc/host_otu.cpp raxtax_amd/csrc/host_tally.cpp raxtax_amd/csrc/host_chimera.cpp \
//       -o denovo_host_check && ./denovo_host_check
// Every record is also held against rtx_chimera_read over the explicit list of the entry's live parents, built here.
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
int chimera_check_params(const char *, const rtx_chimera_params *p) { return p && p->segments >= 2u && p->segments <= RTX_CHIMERA_MAX_SEGMENTS ? RTX_OK : RTX_ERR_INVALID; }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "denovo_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static std::string random_seq(std::mt19937 &rng, size_t len) {
    std::string s(len, '\0');
    for (char &c : s) c = (char)(1u << (rng() % 4));
    return s;
}

static int check(rtx_tally_table *table, rtx_otu *otu, const rtx_denovo_params &prm, uint64_t *flagged) {
    rtx_tally_view tv{};
    CHECK(rtx_tally_table_view(table, &tv) == RTX_OK);
    rtx_denovo *d = nullptr;
    CHECK(rtx_denovo_check_host(table, otu, &prm, &d) == RTX_OK && d);
    rtx_denovo_view_t v{};
    CHECK(rtx_denovo_view(d, &v) == RTX_OK);
    CHECK((v.otu != nullptr) == (otu != nullptr) && v.rounds == 1 && v.scans == v.n_entries);
    const rtx_chimera_params cp{prm.segments, prm.mindelta};
    uint64_t n_flagged = 0, n_checked = 0;
    for (uint64_t e = 0; e < v.n_entries; e++) {
        CHECK(v.row[e] < tv.n_entries && v.lim[e] <= e && (e == 0 || v.weight[e] <= v.weight[e - 1]));
        uint64_t skew = 0;
        for (uint64_t p = 0; p < v.n_entries; p++) skew += (unsigned __int128)v.weight[p] >= (unsigned __int128)prm.abskew * v.weight[e];
        const uint64_t cap = prm.max_parents ? prm.max_parents : RTX_DENOVO_DEFAULT_MAX_PARENTS;
        CHECK(v.lim[e] == std::min(std::min(e, skew), cap));
        // the live parents as references of their own, exact lengths
        std::vector<uint64_t> off(1, 0);
        std::vector<uint32_t> who;
        std::string refs;
        for (uint32_t p = 0; p < v.lim[e]; p++) {
            if (v.rec[p].flag) continue;
            refs.append(reinterpret_cast<const char *>(tv.bases) + tv.base_off[v.row[p]], tv.base_off[v.row[p] + 1] - tv.base_off[v.row[p]]);
            off.push_back(refs.size());
            who.push_back(p);
        }
        const uint64_t len = tv.base_off[v.row[e] + 1] - tv.base_off[v.row[e]];
        std::unique_ptr<uint8_t[]> read(new uint8_t[len ? len : 1]), rb(new uint8_t[refs.size() ? refs.size() : 1]);
        memcpy(read.get(), tv.bases + tv.base_off[v.row[e]], len);
        memcpy(rb.get(), refs.data(), refs.size());
        rtx_chimera_rec want{};
        CHECK(rtx_chimera_read(&cp, read.get(), len, rb.get(), off.data(), who.size(), &want) == RTX_OK);
        auto entry = [&](uint32_t r) { return r == RTX_NO_REF ? RTX_NO_REF : who[r]; };
        want.parent = entry(want.parent);
        want.parent_a = entry(want.parent_a);
        want.parent_b = entry(want.parent_b);
        if (want.status == RTX_CHIM_OK && v.lim[e] == 0) want = rtx_chimera_rec{RTX_DENOVO_NO_PARENT, 0, 0, RTX_NO_REF, 0, 0, 0, RTX_NO_REF, 0, RTX_NO_REF, 0, 0};
        CHECK(memcmp(&want, &v.rec[e], sizeof want) == 0);
        n_flagged += v.rec[e].flag;
        n_checked += v.rec[e].status == RTX_CHIM_OK;
    }
    CHECK(n_flagged == v.n_flagged && n_checked == v.n_checked);
    *flagged += n_flagged;
    // the three formatters into buffers of exactly `need` bytes, and one byte less
    const char *names[2] = {"s0", "s1"};
    for (int f = 0; f < 3; f++) {
        auto call = [&](char *buf, uint64_t cap) {
            return f == 0 ? rtx_denovo_format_records(d, buf, cap) : f == 1 ? rtx_denovo_format_fasta(d, table, otu, 2, buf, cap) : rtx_denovo_format_table(d, table, otu, names, 2, buf, cap);
        };
        const int64_t need = call(nullptr, 0);
        CHECK(need > 0);
        std::unique_ptr<char[]> buf(new char[(size_t)need]);
        CHECK(call(buf.get(), (uint64_t)need) == need);
        CHECK(buf[(size_t)need - 1] == '\n');
        CHECK(call(buf.get(), (uint64_t)need - 1) == -need - (int64_t)RTX_NEED_BASE);
    }
    if (otu) CHECK(rtx_denovo_format_fasta(d, table, nullptr, 1, nullptr, 0) == RTX_ERR_INVALID);  // (made with OTUs, formatted without)
    rtx_denovo_destroy(d);
    return 0;
}

int main() {
    std::mt19937 rng(19);
    // templates, their single-substitution variants, chimeras of two templates, chimeras of chimeras' variants, and the odd lengths
    std::vector<std::string> pool;
    std::vector<uint32_t> weight;
    std::vector<std::string> templates;
    for (int t = 0; t < 12; t++) {
        templates.push_back(random_seq(rng, 150 + (size_t)(rng() % 60)));
        pool.push_back(templates.back());
        weight.push_back(1000u >> (t / 2));
        std::string v = templates.back();
        v[rng() % v.size()] = (char)15;
        pool.push_back(v);
        weight.push_back(3);
    }
    for (int c = 0; c < 10; c++) {
        const std::string &a = templates[rng() % 12], &b = templates[rng() % 12];
        const size_t bp = 40 + rng() % 70;
        std::string chim = a.substr(0, bp) + b.substr(bp);
        pool.push_back(chim);
        weight.push_back(6);
        for (int k = 0; k < 3; k++) chim[(size_t)(20 + 45 * k) % chim.size()] ^= 3;  // (1 <-> 2, 4 <-> 7: two of them become ambiguity codes)
        pool.push_back(chim);
        weight.push_back(2);
    }
    for (size_t len : {1u, 7u, 8u, 9u, 23u, 4096u, 4097u}) { pool.push_back(random_seq(rng, len)); weight.push_back(1u + (uint32_t)(len % 5)); }
    pool.push_back(pool[pool.size() - 1].substr(0, 4096));  // the head of the entry of 4097 bases: its parent holds every window
    weight.push_back(1);
    rtx_tally_table *table = nullptr;
    CHECK(rtx_tally_table_create(2, &table) == RTX_OK);
    {
        const uint64_t n = pool.size();
        uint64_t total = 0;
        for (const std::string &s : pool) total += s.size();
        std::unique_ptr<uint8_t[]> bases(new uint8_t[total]);
        std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
        std::unique_ptr<uint32_t[]> sample(new uint32_t[n]);
        uint64_t at = 0;
        for (uint64_t q = 0; q < n; q++) {
            off[q] = at;
            memcpy(bases.get() + at, pool[q].data(), pool[q].size());
            at += pool[q].size();
            sample[q] = (uint32_t)(rng() % 2);
        }
        off[n] = at;
        CHECK(rtx_tally_table_add(table, n, bases.get(), off.get(), sample.get(), weight.data()) == RTX_OK);
    }
    rtx_denovo *d = nullptr;
    for (const rtx_denovo_params bad : {rtx_denovo_params{1, 24, 2, 0, 0}, rtx_denovo_params{33, 24, 2, 0, 0}, rtx_denovo_params{16, 24, 0, 0, 0}, rtx_denovo_params{16, 24, 2, 0, 1},
                                        rtx_denovo_params{16, 24, 2, RTX_DENOVO_DEFAULT_MAX_PARENTS + 1u, 0}})
        CHECK(rtx_denovo_check_host(table, nullptr, &bad, &d) == RTX_ERR_INVALID && d == nullptr);
    rtx_otu *otu = nullptr;
    CHECK(rtx_otu_cluster_host(table, nullptr, &otu) == RTX_OK);
    uint64_t flagged = 0;
    for (const rtx_denovo_params prm : {rtx_denovo_params{16, 24, 2, 0, 0}, rtx_denovo_params{2, 0, 1, 0, 0}, rtx_denovo_params{32, 10, 3, 5, 0}, rtx_denovo_params{7, 24, 0xFFFFFFFFu, 0, 0}}) {
        if (check(table, nullptr, prm, &flagged)) return 1;
        if (check(table, otu, prm, &flagged)) return 1;
    }
    CHECK(flagged >= 20);
    // an OTU object of another table
    rtx_tally_table *none = nullptr;
    rtx_otu *o0 = nullptr;
    CHECK(rtx_tally_table_create(0, &none) == RTX_OK && rtx_otu_cluster_host(none, nullptr, &o0) == RTX_OK);
    CHECK(rtx_denovo_check_host(table, o0, nullptr, &d) == RTX_ERR_INVALID && d == nullptr);
    // an empty table
    rtx_denovo_view_t v{};
    CHECK(rtx_denovo_check_host(none, o0, nullptr, &d) == RTX_OK && rtx_denovo_view(d, &v) == RTX_OK && v.n_entries == 0 && v.n_flagged == 0);
    CHECK(rtx_denovo_format_fasta(d, none, o0, 1, nullptr, 0) == 0 && rtx_denovo_format_records(d, nullptr, 0) > 0);
    rtx_denovo_destroy(d);
    rtx_otu_destroy(o0);
    rtx_otu_destroy(otu);
    rtx_tally_table_destroy(none);
    rtx_tally_table_destroy(table);
    printf("denovo_host_check: ok (%zu sequences, %llu flags over the runs)\n", pool.size(), (unsigned long long)flagged);
    return 0;
}

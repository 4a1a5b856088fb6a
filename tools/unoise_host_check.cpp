// A stand-alone check of the host side of the denoiser (raxtax_amd/csrc/host_unoise.cpp: rtx_otu_unoise_host, rtx_otu_unoise_view,
// rtx_otu_format_unoise, lim and the tier cut) and of the distance the lanes of the pair kernel run (rtx_math.hpp: unoise_distance over bit
// rows and packed words of the exact sizes) for the sanitizers: built with -fsanitize=address,undefined together with this main.
// Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/unoise_host_check.cpp \
//       raxtax_amd/csrc/host_unoise.cpp raxtax_amd/csrc/host_otu.cpp raxtax_amd/csrc/host_tally.cpp -o unoise_host_check && ./unoise_host_check
// The third computation: the whole matrix of distances first, each from a full (m + 1) x (n + 1) table; k from a product in 128 bits instead
// of a shift; then the statuses over that matrix, a row's candidates taken from a per-row flag, not from a list.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "host_unoise.hpp"
#include "rtx_math.hpp"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "unoise_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static std::string random_seq(std::mt19937 &rng, size_t len) {
    std::string s(len, '\0');
    for (char &c : s) c = (char)(1u << (rng() % 4));
    return s;
}

static uint32_t full_table(const uint8_t *x, size_t m, const uint8_t *y, size_t n) {
    std::vector<uint32_t> d((m + 1) * (n + 1));
    for (size_t i = 0; i <= m; i++) d[i * (n + 1)] = (uint32_t)i;
    for (size_t j = 0; j <= n; j++) d[j] = (uint32_t)j;
    for (size_t i = 1; i <= m; i++)
        for (size_t j = 1; j <= n; j++)
            d[i * (n + 1) + j] = std::min({d[(i - 1) * (n + 1) + j - 1] + (x[i - 1] != y[j - 1]), d[(i - 1) * (n + 1) + j] + 1u, d[i * (n + 1) + j - 1] + 1u});
    return d[m * (n + 1) + n];
}

static uint32_t allowed128(uint64_t wp, uint64_t we, uint32_t alpha, uint32_t max_diffs) {
    uint32_t k = 0;
    for (uint32_t d = 1; d <= max_diffs && alpha * d + 1u < 64u; d++)
        if ((unsigned __int128)wp >= ((unsigned __int128)we << (alpha * d + 1u))) k = d;
    return k;
}

// the lane's distance over arrays of exactly the sizes the kernel's layout promises
static uint32_t lane_distance(const uint8_t *x, uint32_t m, const uint8_t *y, uint32_t n, uint32_t k) {
    const uint32_t nw = rtx::unoise_peq_words(m), tw = (n + 15u) / 16u;
    std::unique_ptr<uint64_t[]> peq(new uint64_t[(size_t)16 * nw]()), text(new uint64_t[tw ? tw : 1]());
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t b = rtx::unoise_peq_bit(i);
        peq[(size_t)(x[i] & 15u) * nw + (b >> 6)] |= 1ull << (b & 63u);
    }
    rtx::unoise_pack(y, n, text.get());
    bool finished = false;
    const uint64_t *pq = peq.get(), *tx = text.get();
    return rtx::unoise_distance(m, n, k, [=](uint32_t c, uint32_t j) { return rtx::unoise_eq(pq + (size_t)c * nw, j); }, [=](uint32_t t) { return tx[t]; }, finished);
}

static int check(rtx_tally_table *table, const rtx_unoise_params &prm, uint64_t *absorbed) {
    rtx_tally_view tv{};
    CHECK(rtx_tally_table_view(table, &tv) == RTX_OK);
    rtx_otu *o = nullptr;
    CHECK(rtx_otu_unoise_host(table, &prm, &o) == RTX_OK && o);
    rtx_unoise_view_t v{};
    rtx_otu_view_t ov{};
    CHECK(rtx_otu_unoise_view(o, &v) == RTX_OK && rtx_otu_view(o, &ov) == RTX_OK);
    const uint64_t n = tv.n_entries;
    const uint32_t maxd = prm.max_diffs ? prm.max_diffs : RTX_UNOISE_MAX_DIFFS;
    CHECK(v.n_rows == n && v.alpha == prm.alpha && v.minsize == prm.minsize && v.max_diffs == maxd && v.tiers == 0 && v.pairs == 0);
    auto len = [&](uint64_t r) { return tv.base_off[r + 1] - tv.base_off[r]; };
    std::vector<uint32_t> dist(n * n, 0);
    for (uint64_t a = 0; a < n; a++)
        for (uint64_t b = 0; b < a; b++) {
            if (len(a) > RTX_OTU_MAX_LEN || len(b) > RTX_OTU_MAX_LEN) continue;
            const uint32_t d = full_table(tv.bases + tv.base_off[a], len(a), tv.bases + tv.base_off[b], len(b));
            dist[a * n + b] = d;
            // the lanes' distance, both ways round, at the pair's own threshold and at the largest
            const uint32_t diff = (uint32_t)(len(a) > len(b) ? len(a) - len(b) : len(b) - len(a));
            for (const uint32_t k : {allowed128(tv.sizes[b], tv.sizes[a], prm.alpha, maxd), 16u}) {
                if (diff > k) continue;
                const uint32_t want = d <= k ? d : rtx::kUnoiseNoDist;
                CHECK(lane_distance(tv.bases + tv.base_off[a], (uint32_t)len(a), tv.bases + tv.base_off[b], (uint32_t)len(b), k) == want);
                CHECK(lane_distance(tv.bases + tv.base_off[b], (uint32_t)len(b), tv.bases + tv.base_off[a], (uint32_t)len(a), k) == want);
            }
        }
    std::vector<uint8_t> status(n, RTX_UNOISE_LEFT);
    uint64_t counts[4] = {0, 0, 0, 0}, n_otus = 0;
    for (uint64_t e = 0; e < n; e++) {
        uint64_t lim = 0;
        for (uint64_t p = 0; p < n; p++) lim += (unsigned __int128)tv.sizes[p] >= ((unsigned __int128)tv.sizes[e] << (prm.alpha + 1u));
        CHECK(v.lim[e] == lim && lim <= e);
        uint32_t bd = RTX_NO_DIST, bp = RTX_NO_REF;
        if (len(e) > RTX_OTU_MAX_LEN) {
            status[e] = RTX_UNOISE_LONG;
        } else {
            for (uint64_t p = 0; p < e; p++) {
                if (status[p] != RTX_UNOISE_ZOTU) continue;
                const uint32_t k = allowed128(tv.sizes[p], tv.sizes[e], prm.alpha, maxd);
                CHECK((k >= 1u) == (p < lim));
                if (k >= 1u && dist[e * n + p] <= k && dist[e * n + p] < bd) { bd = dist[e * n + p]; bp = (uint32_t)p; }
            }
            status[e] = bp != RTX_NO_REF ? RTX_UNOISE_ABSORBED : tv.sizes[e] >= prm.minsize ? RTX_UNOISE_ZOTU : RTX_UNOISE_LEFT;
        }
        CHECK(v.status[e] == status[e] && v.parent[e] == bp && v.dist[e] == bd);
        counts[status[e]]++;
        CHECK(ov.otu[e] == (bp != RTX_NO_REF ? ov.otu[bp] : n_otus));
        if (bp == RTX_NO_REF) { CHECK(ov.seed[n_otus] == e); n_otus++; }
    }
    CHECK(v.n_zotu == counts[0] && v.n_absorbed == counts[1] && v.n_left == counts[2] && v.n_long == counts[3] && ov.n_otus == n_otus && ov.long_rows == counts[3]);
    CHECK(ov.n_links == 0 && ov.rounds == 0 && ov.link_passes == 0);
    *absorbed += counts[1];
    // the tier cut: inside a tier nobody is below anybody's lim, and the row behind a tier has the tier's first row below its lim
    std::vector<uint64_t> tier;
    std::vector<uint32_t> lim;
    rtx::unoise_tiers(tv, prm.alpha, tier);
    rtx::unoise_lim(tv, prm.alpha, lim);
    CHECK(!tier.empty() && tier.back() == n && tier.size() - 1 <= 64u / (prm.alpha + 1u) + 1u);
    for (size_t t = 0; t + 1 < tier.size(); t++) {
        CHECK(tier[t] < tier[t + 1]);
        for (uint64_t r = tier[t]; r < tier[t + 1]; r++) CHECK(lim[r] <= tier[t] && lim[r] == v.lim[r]);
        if (tier[t + 1] < n) CHECK(lim[tier[t + 1]] > tier[t]);
    }
    // the text into a buffer of exactly `need` bytes, and one byte less; the three formatters of any rtx_otu take the object
    const int64_t need = rtx_otu_format_unoise(o, nullptr, 0);
    CHECK(need > 0);
    std::unique_ptr<char[]> buf(new char[(size_t)need]);
    CHECK(rtx_otu_format_unoise(o, buf.get(), (uint64_t)need) == need && buf[(size_t)need - 1] == '\n');
    CHECK(rtx_otu_format_unoise(o, buf.get(), (uint64_t)need - 1) == -need - (int64_t)RTX_NEED_BASE);
    const char *names[2] = {"s0", "s1"};
    CHECK(rtx_otu_format_fasta(o, table, prm.minsize, nullptr, 0) >= 0 && rtx_otu_format_map(o, nullptr, 0) > 0 && rtx_otu_format_table(o, names, 1, nullptr, 0) > 0);
    rtx_otu_destroy(o);
    return 0;
}

int main() {
    std::mt19937 rng(31);
    std::vector<std::string> pool;
    std::vector<uint32_t> weight;
    auto edit = [&](std::string s, int edits) {
        for (int e = 0; e < edits; e++) {
            const size_t at = rng() % s.size();
            switch (rng() % 3) {
                case 0: s[at] = (char)(1u << (rng() % 4)); break;
                case 1: if (s.size() > 1) s.erase(at, 1); break;
                default: s.insert(at, 1, (char)(1u << (rng() % 4)));
            }
        }
        return s;
    };
    for (int t = 0; t < 10; t++) {  // centres of geometric weights, variants 1 .. 4 edits away at weights around every threshold
        const std::string c = random_seq(rng, 60 + (size_t)(rng() % 80));
        const uint32_t wc = 40000u >> t;
        pool.push_back(c);
        weight.push_back(wc);
        for (int k = 0; k < 12; k++) {
            const int edits = 1 + (int)(rng() % 4);
            pool.push_back(edit(c, edits));
            weight.push_back((uint32_t)std::max<int64_t>(1, (int64_t)(wc >> (2 * edits + 1)) + (int64_t)(rng() % 3) - 1));
        }
    }
    for (size_t len : {1u, 2u, 15u, 16u, 17u, 63u, 64u, 65u, 4096u, 4097u}) { pool.push_back(random_seq(rng, len)); weight.push_back(1u + (uint32_t)(len % 90)); }
    pool.push_back(edit(pool[pool.size() - 2], 1));  // beside the row of 4096
    weight.push_back(2);
    pool.push_back(pool[pool.size() - 2].substr(1));  // the row of 4097 without its first code: not long, the long row is no parent
    weight.push_back(1);
    {
        std::string amb = pool[0];
        amb[5] = (char)15;
        pool.push_back(amb);
        weight.push_back(7);
    }
    for (size_t a = 0; a < pool.size(); a++)  // (equal strings would be one row with the sum of their weights: the later one is dropped)
        for (size_t b = pool.size() - 1; b > a; b--)
            if (pool[b] == pool[a]) { pool.erase(pool.begin() + (long)b); weight.erase(weight.begin() + (long)b); }
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
    rtx_otu *o = nullptr;
    for (const rtx_unoise_params bad : {rtx_unoise_params{8, 0, 0, 0}, rtx_unoise_params{8, 9, 0, 0}, rtx_unoise_params{0, 2, 0, 0}, rtx_unoise_params{8, 2, 17, 0}, rtx_unoise_params{8, 2, 0, 1}})
        CHECK(rtx_otu_unoise_host(table, &bad, &o) == RTX_ERR_INVALID && o == nullptr);
    uint64_t absorbed = 0;
    for (const rtx_unoise_params prm : {rtx_unoise_params{8, 2, 0, 0}, rtx_unoise_params{1, 1, 3, 0}, rtx_unoise_params{100, 3, 16, 0}, rtx_unoise_params{2, 8, 1, 0}})
        if (check(table, prm, &absorbed)) return 1;
    CHECK(absorbed >= 100);
    // any other rtx_otu is no denoising result; an empty table
    rtx_unoise_view_t v{};
    CHECK(rtx_otu_cluster_host(table, nullptr, &o) == RTX_OK && rtx_otu_unoise_view(o, &v) == RTX_ERR_INVALID && rtx_otu_format_unoise(o, nullptr, 0) == RTX_ERR_INVALID);
    rtx_otu_destroy(o);
    rtx_tally_table *none = nullptr;
    CHECK(rtx_tally_table_create(0, &none) == RTX_OK && rtx_otu_unoise_host(none, nullptr, &o) == RTX_OK && rtx_otu_unoise_view(o, &v) == RTX_OK);
    CHECK(v.n_rows == 0 && v.minsize == 8 && v.alpha == 2 && v.max_diffs == 16 && rtx_otu_format_unoise(o, nullptr, 0) > 0);
    rtx_otu_destroy(o);
    rtx_tally_table_destroy(none);
    rtx_tally_table_destroy(table);
    printf("unoise_host_check: ok (%zu sequences, %llu absorbed over the runs)\n", pool.size(), (unsigned long long)absorbed);
    return 0;
}

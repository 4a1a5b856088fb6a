// A stand-alone check of the host table of distinct reads (raxtax_amd/csrc/host_tally.cpp: rtx_tally_table_add, _merge, _view and the two
// formatters) for the sanitizers: accumulation, layout and text are pointer arithmetic over caller buffers, so they are built with
// -fsanitize=address,undefined together with this main and run on heap buffers of the exact lengths.  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/tally_host_check.cpp \
//       raxtax_amd/csrc/host_tally.cpp -o tally_host_check && ./tally_host_check
// Every cell is also held against a std::map written here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "raxtax_hip.h"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "tally_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main() {
    std::mt19937 rng(7);
    const uint32_t ns = 3;
    std::vector<std::string> pool;
    for (int i = 0; i < 60; i++) {
        std::string s(rng() % 40, '\0');  // (some of length 0)
        for (char &c : s) c = (char)(1u << (rng() % 4));
        pool.push_back(s);
    }
    pool[5] = pool[6].substr(0, pool[6].size() / 2);  // a prefix of another
    std::map<std::string, std::vector<uint64_t>> want;
    rtx_tally_table *tables[3] = {nullptr, nullptr, nullptr};
    uint64_t reads = 0;
    for (int k = 0; k < 3; k++) {
        CHECK(rtx_tally_table_create(ns, &tables[k]) == RTX_OK);
        for (int add = 0; add < 4; add++) {
            const uint64_t n = 1 + rng() % 200;
            std::vector<uint64_t> off(n + 1, 0);
            std::string flat;
            std::unique_ptr<uint32_t[]> sample(new uint32_t[n]), weight(new uint32_t[n]);
            for (uint64_t q = 0; q < n; q++) {
                const std::string &s = pool[rng() % pool.size()];
                flat += s;
                off[q + 1] = flat.size();
                weight[q] = (uint32_t[]){0u, 1u, 5u}[rng() % 3];
                sample[q] = weight[q] ? rng() % ns : RTX_DEMUX_NONE;
                if (weight[q] && !s.empty()) {
                    auto &row = want[s];
                    row.resize(ns);
                    row[sample[q]] += weight[q];
                    reads += weight[q];
                }
            }
            std::unique_ptr<uint8_t[]> bases(new uint8_t[flat.size() ? flat.size() : 1]);  // exactly the bases, nothing behind them
            memcpy(bases.get(), flat.data(), flat.size());
            CHECK(rtx_tally_table_add(tables[k], n, bases.get(), off.data(), sample.get(), weight.get()) == RTX_OK);
            sample[n - 1] = ns;  // out of range on a read that counts: refused, nothing counted
            weight[n - 1] = 1;
            if (off[n] != off[n - 1]) CHECK(rtx_tally_table_add(tables[k], n, bases.get(), off.data(), sample.get(), weight.get()) == RTX_ERR_INVALID);
        }
    }
    rtx_tally_table *sum = nullptr;
    CHECK(rtx_tally_table_merge(tables, 3, &sum) == RTX_OK);
    rtx_tally_view v{};
    CHECK(rtx_tally_table_view(sum, &v) == RTX_OK);
    CHECK(v.n_entries == want.size() && v.n_columns == ns && v.totals[0] == reads && v.totals[1] == want.size() && v.totals[2] == 0);
    for (uint64_t r = 0; r < v.n_entries; r++) {
        const std::string s((const char *)v.bases + v.base_off[r], v.base_off[r + 1] - v.base_off[r]);
        CHECK(want.count(s));
        uint64_t size = 0;
        for (uint32_t c = 0; c < ns; c++) { CHECK(v.counts[r * ns + c] == want[s][c]); size += want[s][c]; }
        CHECK(v.sizes[r] == size);
        if (r) {
            const std::string p((const char *)v.bases + v.base_off[r - 1], v.base_off[r] - v.base_off[r - 1]);
            CHECK(v.sizes[r - 1] > size || (v.sizes[r - 1] == size && p < s));
        }
    }
    const char *names[3] = {"a", "b", "c"};
    for (int which = 0; which < 2; which++) {
        auto fmt = [&](char *buf, uint64_t cap) { return which ? rtx_tally_format_table(sum, names, 2, buf, cap) : rtx_tally_format_fasta(sum, 2, buf, cap); };
        const int64_t need = fmt(nullptr, 0);
        CHECK(need > 0);
        std::unique_ptr<char[]> buf(new char[need]);  // exactly `need` bytes
        CHECK(fmt(buf.get(), (uint64_t)need - 1) == -need - RTX_NEED_BASE);
        CHECK(fmt(buf.get(), (uint64_t)need) == need);
        CHECK(buf[need - 1] == '\n');
    }
    rtx_tally_table_destroy(sum);
    for (rtx_tally_table *t : tables) rtx_tally_table_destroy(t);
    printf("tally_host_check: %zu entries, %llu reads: ok\n", want.size(), (unsigned long long)reads);
    return 0;
}

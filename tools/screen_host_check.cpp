// A stand-alone check of the contaminant screen's host code (raxtax_amd/csrc/host_screen.cpp: rtx_screen_set_build, rtx_screen_read) and of the
// x86 emulation of the kernel (raxtax_amd/csrc/rtx_emul.cpp: emul_screen_read) for the sanitizers: set, table and reads are pointer arithmetic
// over caller buffers, so they are built with -fsanitize=address,undefined together with this main and run on heap buffers of the exact
// lengths (a read one byte past an end is then an error).  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/screen_host_check.cpp \
//       raxtax_amd/csrc/host_screen.cpp raxtax_amd/csrc/rtx_emul.cpp -o screen_host_check && ./screen_host_check
// The set is the adversarial one of tests/test_screen_cpu.py: single-window sequences whose keys crowd the last slots of a 1024-slot table, so
// that one chain runs across the wrap.  Every lookup is also held against a std::map written here.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "raxtax_hip.h"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
}
extern "C" void emul_screen_read(const uint32_t *slots, uint32_t log2m, const uint8_t *x, uint32_t len, uint32_t *out);

static uint32_t rc_of(uint32_t w) {
    uint32_t r = 0;
    for (int j = 0; j < 16; j++) r |= (3u - ((w >> (2 * j)) & 3u)) << (2 * (15 - j));
    return r;
}
static std::vector<uint8_t> codes_of(uint32_t w) {
    std::vector<uint8_t> c(16);
    for (int j = 0; j < 16; j++) c[j] = (uint8_t)(1u << ((w >> (2 * (15 - j))) & 3u));
    return c;
}

int main() {
    std::mt19937 rng(50);
    const uint32_t inv = 0x0E8B2F51u;  // 0x9E3779B1 * inv == 1 (mod 2^32)
    if ((uint32_t)(0x9E3779B1u * inv) != 1u) { fprintf(stderr, "the inverse of the hash multiplier is wrong\n"); return 2; }
    auto homed_at = [&](uint32_t slot, size_t count, const std::map<uint32_t, uint32_t> &taken) {
        std::vector<uint32_t> out;
        while (out.size() < count) {
            const uint32_t c = (uint32_t)(((slot << 22) | (rng() & 0x3FFFFFu)) * inv);
            if (c <= rc_of(c) && !taken.count(c) && std::find(out.begin(), out.end(), c) == out.end()) out.push_back(c);
        }
        return out;
    };
    std::map<uint32_t, uint32_t> members;  // canonical value -> source
    std::vector<uint32_t> keys;
    for (auto [slot, count] : {std::pair<uint32_t, size_t>{1020u, 10}, {1022u, 3}, {1023u, 3}, {500u, 2}})
        for (uint32_t c : homed_at(slot, count, members)) { members[c] = (uint32_t)keys.size(); keys.push_back(c); }
    std::vector<uint32_t> absent;
    for (uint32_t slot : {1020u, 1021u, 1022u, 1023u, 0u, 1u, 5u, 11u})
        for (uint32_t c : homed_at(slot, 2, members)) absent.push_back(c);
    // the set: exact-size heap arrays
    const size_t n = keys.size();
    std::unique_ptr<uint8_t[]> bases(new uint8_t[16 * n]);
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    for (size_t i = 0; i < n; i++) {
        const auto c = codes_of(keys[i]);
        memcpy(bases.get() + 16 * i, c.data(), 16);
        off[i] = 16 * i;
    }
    off[n] = 16 * n;
    rtx_screen_set *set = nullptr;
    if (rtx_screen_set_build(n, bases.get(), off.get(), &set) != RTX_OK) { fprintf(stderr, "rtx_screen_set_build failed\n"); return 2; }
    uint64_t n_keys = 0, n_slots = 0, disp = 0, wrapped = 0;
    const uint32_t *slots = nullptr;
    uint32_t log2m = 0;
    if (rtx_screen_set_info(set, &n_keys, &n_slots, &disp, &wrapped, nullptr) != RTX_OK || rtx_screen_set_table(set, &slots, &log2m) != RTX_OK) return 2;
    if (n_keys != n || n_slots != 1024 || log2m != 10 || disp < 8 || wrapped < 1) {
        fprintf(stderr, "the table is not the adversarial one: %llu keys, %llu slots, displacement %llu, %llu wrapped\n", (unsigned long long)n_keys, (unsigned long long)n_slots,
                (unsigned long long)disp, (unsigned long long)wrapped);
        return 1;
    }
    // reads: every key and every absent value alone, in either orientation, and all of them in one read with a breaking code behind each;
    // lengths around the piece and the step with keys at their ends
    int bad = 0;
    const rtx_screen_params params{1u, 0u};
    auto check = [&](const std::vector<uint8_t> &read, uint32_t lo, uint32_t hi) {
        std::unique_ptr<uint8_t[]> x(new uint8_t[read.size() ? read.size() : 1]);  // (exact size)
        if (!read.empty()) memcpy(x.get(), read.data(), read.size());
        uint32_t want[4] = {0, 0, RTX_SCREEN_NONE, RTX_SCREEN_NONE};
        for (uint32_t p = lo; p + 16 <= hi; p++) {
            uint32_t w = 0;
            bool valid = true;
            for (uint32_t j = 0; j < 16; j++) {
                const uint8_t c = read[p + j];
                valid = valid && (c == 1 || c == 2 || c == 4 || c == 8);
                w = w << 2 | (c == 2 ? 1u : c == 4 ? 2u : c == 8 ? 3u : 0u);
            }
            if (!valid) continue;
            want[0]++;
            const auto it = members.find(std::min(w, rc_of(w)));
            if (it == members.end()) continue;
            want[1]++;
            if (want[2] == RTX_SCREEN_NONE) { want[2] = p - lo; want[3] = it->second; }
        }
        uint32_t got[5], emu[4];
        if (rtx_screen_read(set, &params, x.get(), read.size(), lo, hi, &got[0], &got[1], &got[2], &got[3], &got[4]) != RTX_OK) { bad++; return; }
        std::unique_ptr<uint8_t[]> y(new uint8_t[hi - lo ? hi - lo : 1]);
        if (hi > lo) memcpy(y.get(), read.data() + lo, hi - lo);
        emul_screen_read(slots, log2m, y.get(), hi - lo, emu);
        if (memcmp(got, want, 16) != 0 || memcmp(emu, want, 16) != 0 || got[4] != (want[1] >= 1u ? 1u : 0u)) {
            fprintf(stderr, "a read of %zu bases, range [%u, %u): host %u %u %u %u, emulator %u %u %u %u, expected %u %u %u %u\n", read.size(), lo, hi, got[0], got[1], got[2], got[3],
                    emu[0], emu[1], emu[2], emu[3], want[0], want[1], want[2], want[3]);
            bad++;
        }
    };
    std::vector<uint32_t> all = keys;
    all.insert(all.end(), absent.begin(), absent.end());
    std::vector<uint8_t> joined;
    for (uint32_t c : all) {
        auto f = codes_of(c), r = codes_of(rc_of(c));
        check(f, 0, 16);
        check(r, 0, 16);
        joined.insert(joined.end(), f.begin(), f.end());
        joined.push_back(15);
    }
    check(joined, 0, (uint32_t)joined.size());
    check(joined, 5, (uint32_t)joined.size() - 3);
    for (uint32_t len : {0u, 1u, 15u, 16u, 17u, 31u, 32u, 33u, 255u, 256u, 257u, 271u, 272u, 511u, 512u, 513u, 658u}) {
        std::vector<uint8_t> read(len);
        for (auto &c : read) c = (uint8_t)(1u << (rng() & 3u));
        if (len >= 16) {
            const auto k = codes_of(keys[len % keys.size()]);
            memcpy(read.data() + len - 16, k.data(), 16);  // a key in the last window
            if (len >= 48) memcpy(read.data(), codes_of(rc_of(keys[0])).data(), 16);
        }
        check(read, 0, len);
        if (len >= 4) check(read, len / 4, len);
    }
    rtx_screen_set_free(set);
    if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
    printf("screen_host_check: %zu keys, %zu absent values, all lookups agree\n", keys.size(), absent.size());
    return 0;
}

// A stand-alone check of rtx_semiglobal_distance (raxtax_amd/csrc/host_align.cpp) for the sanitizers: the host function is pointer arithmetic
// over caller buffers, so it is built with -fsanitize=address,undefined together with this main and run on heap buffers of the exact
// lengths (a read one byte past an end is then an error).  Build and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc \
//       tools/identity_host_check.cpp raxtax_amd/csrc/host_align.cpp -o identity_host_check && ./identity_host_check
// Every pair is also held against a plain O(mn) Sellers recurrence written here.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "raxtax_hip.h"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
}

static uint32_t plain(const std::vector<uint8_t> &q, const std::vector<uint8_t> &r) {
    const size_t m = q.size();
    std::vector<uint32_t> col(m + 1), nxt(m + 1);
    for (size_t i = 0; i <= m; i++) col[i] = (uint32_t)i;
    uint32_t best = (uint32_t)m;
    for (uint8_t c : r) {
        nxt[0] = 0;
        for (size_t i = 1; i <= m; i++) {
            const bool match = q[i - 1] >= 1 && q[i - 1] <= 15 && c >= 1 && c <= 15 && (q[i - 1] & c) != 0;
            nxt[i] = std::min({col[i - 1] + (match ? 0u : 1u), col[i] + 1u, nxt[i - 1] + 1u});
        }
        col.swap(nxt);
        best = std::min(best, col[m]);
    }
    return best;
}

static int check(const std::vector<uint8_t> &q, const std::vector<uint8_t> &r, const char *what) {
    // exact-size heap copies: the sanitizer sees every byte outside them
    std::unique_ptr<uint8_t[]> qb(new uint8_t[q.size() ? q.size() : 1]), rb(new uint8_t[r.size() ? r.size() : 1]);
    if (!q.empty()) std::memcpy(qb.get(), q.data(), q.size());
    if (!r.empty()) std::memcpy(rb.get(), r.data(), r.size());
    uint32_t d = 0;
    const int rc = rtx_semiglobal_distance(q.empty() ? nullptr : qb.get(), q.size(), r.empty() ? nullptr : rb.get(), r.size(), &d);
    const uint32_t want = plain(q, r);
    if (rc != RTX_OK || d != want) {
        std::fprintf(stderr, "FAIL %s: rc %d, dist %u, expected %u (qlen %zu, rlen %zu)\n", what, rc, d, want, q.size(), r.size());
        return 1;
    }
    return 0;
}

int main() {
    std::mt19937 rng(28);
    auto rnd = [&](size_t n) { std::vector<uint8_t> v(n); for (auto &b : v) b = (uint8_t)(1u << (rng() & 3u)); return v; };
    auto cat = [](std::vector<uint8_t> a, const std::vector<uint8_t> &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
    auto sub = [](const std::vector<uint8_t> &a, size_t lo, size_t hi) { return std::vector<uint8_t>(a.begin() + lo, a.begin() + hi); };
    int bad = 0, n = 0;
    auto run = [&](const std::vector<uint8_t> &q, const std::vector<uint8_t> &r, const char *what) { bad += check(q, r, what); n++; };
    const std::vector<uint8_t> ref = rnd(658);
    run(rnd(40), {}, "an empty reference");
    run({}, ref, "an empty query");
    run(ref, ref, "equal");
    run(sub(ref, 200, 400), ref, "a substring");
    run(cat(sub(ref, 0, 300), rnd(30)), sub(ref, 0, 300), "a prefix and 30 bases of overhang");
    for (size_t pos : {(size_t)0, (size_t)329, (size_t)657}) {
        std::vector<uint8_t> s = ref;
        s[pos] = (uint8_t)(s[pos] == 8 ? 1 : s[pos] << 1);
        run(s, ref, "a substitution");
        s = ref;
        s.insert(s.begin() + pos, (uint8_t)(ref[pos] == 1 ? 2 : 1));
        run(s, ref, "an insertion");
        s = ref;
        s.erase(s.begin() + pos);
        run(s, ref, "a deletion");
    }
    for (int side = 0; side < 2; side++)
        for (uint8_t byte : {(uint8_t)15, (uint8_t)3, (uint8_t)5, (uint8_t)10, (uint8_t)0, (uint8_t)0x20}) {
            std::vector<uint8_t> a = sub(ref, 100, 400), b = ref;
            if (side == 0) a[150] = a[151] = a[290] = byte;
            else b[250] = b[251] = b[390] = byte;
            run(a, b, "an ambiguity code or a byte that is no code");
        }
    for (size_t len : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)127, (size_t)128, (size_t)129, (size_t)1023, (size_t)1024, (size_t)1025,
                       (size_t)4095, (size_t)4096}) {
        std::vector<uint8_t> r = rnd(len + 50), s = sub(r, 20, 20 + len);
        for (size_t k = 0; k < std::max<size_t>(1, len / 50); k++) s[rng() % len] = (uint8_t)(1u << (rng() & 3u));
        run(s, r, "a query length at a block edge");
        run(s, sub(r, 0, len / 2 + 1), "... against a short reference");
    }
    std::printf("%d pairs, %d failed\n", n, bad);
    return bad ? 1 : 0;
}

// A stand-alone check of what the front stage objects share on the host (raxtax_amd/csrc/host_stage.hpp: parallel_ranges, check_reads,
// layout_ranges) for the sanitizers: all of it is pointer arithmetic over caller arrays, so it is built with -fsanitize=address,undefined
// together with this main and run on heap buffers of the exact lengths (a byte past an end is then an error).  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/stage_host_check.cpp \
//       -o stage_host_check && ./stage_host_check
// Every batch goes through layout_ranges and then through the copy of its ranges into 16-byte pieces as rtx_screen_run does it (on the
// thread fan, into a buffer of exactly pieces * 16 bytes), and is held against a layout computed here.  Then every rejection.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host_stage.hpp"

static std::string g_error;
namespace rtx {
void set_error(const char *fmt, ...) {  // (the library's lives in rtx_api_index.hip)
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace rtx

static int bad = 0;
static void fail(const char *what, const char *name) {
    fprintf(stderr, "%s: %s\n", name, what);
    bad++;
}

constexpr uint32_t kPiece = 16, kMaxLen = 1u << 20;

// lens: the reads; ranges: [lo, hi) per read, or empty for the whole reads; nt: the threads offered to the fan; first: the offset of read 0
static void batch(const char *name, const std::vector<uint32_t> &lens, const std::vector<std::pair<uint32_t, uint32_t>> &ranges, unsigned nt, unsigned want_threads,
                  uint64_t first = 0) {
    const uint64_t n = lens.size();
    std::unique_ptr<uint64_t[]> off(new uint64_t[n + 1]);
    off[0] = first;
    for (uint64_t r = 0; r < n; r++) off[r + 1] = off[r] + lens[r];
    const uint64_t total = off[n];  // (the array the offsets point into starts at 0)
    std::unique_ptr<uint8_t[]> bases(new uint8_t[total]);
    for (uint64_t i = 0; i < total; i++) bases[i] = (uint8_t)(1u + i % 251u);
    std::unique_ptr<uint32_t[]> lo, hi;
    if (!ranges.empty()) {
        lo.reset(new uint32_t[n]);
        hi.reset(new uint32_t[n]);
        for (uint64_t r = 0; r < n; r++) { lo[r] = ranges[r].first; hi[r] = ranges[r].second; }
    }
    if (rtx::check_reads(name, n, off.get(), bases.get(), kMaxLen) != RTX_OK) return fail("check_reads refuses the batch", name);
    std::unique_ptr<uint32_t[]> h_off(new uint32_t[n]), h_len(new uint32_t[n]);
    uint64_t pieces = ~0ull;
    if (rtx::layout_ranges(name, n, off.get(), lo.get(), hi.get(), kMaxLen, kPiece, h_off.get(), h_len.get(), &pieces) != RTX_OK) return fail("layout_ranges refuses the batch", name);
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint32_t a = lo ? lo[r] : 0u, b = hi ? hi[r] : lens[r];
        if (h_off[r] != at || h_len[r] != b - a) return fail("the layout differs", name);
        at += (b - a + kPiece - 1u) / kPiece;
    }
    if (pieces != at) return fail("the number of pieces differs", name);
    std::unique_ptr<uint8_t[]> hb(new uint8_t[pieces * kPiece]);  // (exact: the stages add 16 bytes that nothing here may need)
    memset(hb.get(), 0xEE, pieces * kPiece);
    std::atomic<unsigned> threads{0};
    std::atomic<uint64_t> covered{0};
    const uint64_t *o = off.get();
    const uint32_t *l = lo.get(), *ho = h_off.get(), *hl = h_len.get();
    const uint8_t *x = bases.get();
    uint8_t *dst = hb.get();
    rtx::parallel_ranges(n, nt, 4096, [&](unsigned k, uint64_t a, uint64_t b) {
        threads.fetch_add(1);
        covered.fetch_add(b - a);
        if (a != n * k / std::max(1u, want_threads) || b != n * (k + 1) / std::max(1u, want_threads)) covered.fetch_add(1ull << 40);
        for (uint64_t r = a; r < b; r++)
            if (hl[r]) memcpy(dst + (size_t)ho[r] * kPiece, x + o[r] + (l ? l[r] : 0u), hl[r]);
    });
    if (threads.load() != want_threads) return fail("the fan ran another number of threads", name);
    if (covered.load() != n) return fail("the ranges of the fan do not tile the batch", name);
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t src = off[r] + (lo ? lo[r] : 0u);
        if (h_len[r] && memcmp(hb.get() + (size_t)h_off[r] * kPiece, bases.get() + src, h_len[r]) != 0) return fail("a staged range differs", name);
        const uint64_t end = (size_t)h_off[r] * kPiece + h_len[r], next = r + 1 < n ? (uint64_t)h_off[r + 1] * kPiece : pieces * kPiece;
        for (uint64_t i = end; i < next; i++)
            if (hb[i] != 0xEE) return fail("the padding behind a range was written", name);
    }
}

static void refused(const char *name, int rc, const char *text) {
    if (rc != RTX_ERR_INVALID) return fail("not refused", name);
    if (g_error != text) {
        fprintf(stderr, "%s: the error text is '%s', expected '%s'\n", name, g_error.c_str(), text);
        bad++;
    }
}

int main() {
    batch("n = 1", {40}, {}, 4, 1);
    batch("n = 1, a range", {40}, {{3, 37}}, 4, 1);
    batch("all reads empty", {0, 0, 0}, {}, 4, 1);
    batch("every range empty", {20, 16, 5}, {{0, 0}, {16, 16}, {2, 2}}, 4, 1);
    batch("a range ending on the last byte of the batch", {33, 0, 47}, {{1, 30}, {0, 0}, {31, 47}}, 4, 1);
    batch("lengths 15, 16 and 17", {15, 16, 17}, {}, 4, 1);
    batch("lengths 15, 16 and 17 as ranges", {40, 40, 40}, {{25, 40}, {24, 40}, {23, 40}}, 4, 1);
    batch("offsets that do not start at 0", {15, 16, 17}, {}, 4, 1, 7);
    {
        std::vector<uint32_t> lens(8193);
        std::vector<std::pair<uint32_t, uint32_t>> ranges(lens.size());
        for (size_t r = 0; r < lens.size(); r++) {
            lens[r] = (uint32_t)(r * 7u % 41u);
            ranges[r] = {lens[r] / 3u, lens[r] - lens[r] / 5u};
        }
        batch("n = 8193", lens, {}, 4, 3);
        batch("n = 8193, ranges", lens, ranges, 4, 3);
        batch("n = 8193, two threads offered", lens, ranges, 2, 2);
        batch("n = 8193, no thread offered", lens, ranges, 0, 1);
        lens.resize(4096);
        batch("n = 4096", lens, {}, 4, 1);
        lens.resize(4097);
        batch("n = 4097", lens, {}, 4, 2);
    }
    // the rejections
    const uint8_t one[1] = {1};
    uint32_t h_off[16], h_len[16];
    uint64_t pieces = 0;
    {
        const uint64_t off[4] = {0, 10, 9, 12};
        refused("check_reads, not monotone", rtx::check_reads("who", 3, off, one, kMaxLen), "base_off not monotone at query 1");
        refused("layout_ranges, not monotone", rtx::layout_ranges("who", 3, off, nullptr, nullptr, kMaxLen, kPiece, h_off, h_len, &pieces), "base_off not monotone at query 1");
    }
    {
        const uint64_t off[3] = {0, 10, 10 + (uint64_t)kMaxLen + 1};
        refused("check_reads, over-long", rtx::check_reads("who", 2, off, one, kMaxLen), "who: read 1 has 1048577 bases (at most 1048576)");
        refused("layout_ranges, over-long", rtx::layout_ranges("who", 2, off, nullptr, nullptr, kMaxLen, kPiece, h_off, h_len, &pieces), "who: read 1 has 1048577 bases (at most 1048576)");
        const uint64_t big[2] = {5, 5 + (1ull << 32)};
        refused("check_reads, 2^32 bases", rtx::check_reads("who", 1, big, one, 0xFFFFFFFFull), "who: read 0 has 4294967296 bases (at most 2^32 - 1)");
    }
    {
        const uint64_t off[3] = {0, 10, 30};
        refused("check_reads, null bases", rtx::check_reads("who", 2, off, nullptr, kMaxLen), "who: null bases");
        const uint64_t none[3] = {4, 4, 4};
        if (rtx::check_reads("who", 2, none, nullptr, kMaxLen) != RTX_OK) fail("null bases of an empty batch refused", "check_reads");
        const uint32_t lo[2] = {0, 12}, hi[2] = {10, 11}, hi2[2] = {11, 20};
        refused("layout_ranges, lo > hi", rtx::layout_ranges("who", 2, off, lo, hi, kMaxLen, kPiece, h_off, h_len, &pieces), "who: read 1 of 20 bases has the range [12, 11)");
        refused("layout_ranges, hi > len", rtx::layout_ranges("who", 2, off, lo, hi2, kMaxLen, kPiece, h_off, h_len, &pieces), "who: read 0 of 10 bases has the range [0, 11)");
    }
    {
        uint64_t off[17];  // 16 reads of 2^28 pieces each: the 2^32nd piece is refused (only the offsets are read)
        for (int r = 0; r <= 16; r++) off[r] = (uint64_t)r << 32;
        std::vector<uint32_t> lo(16, 0u), hi(16, 0xFFFFFFF1u);
        refused("layout_ranges, 2^32 bases", rtx::layout_ranges("who", 16, off, lo.data(), hi.data(), 0xFFFFFFFFu, kPiece, h_off, h_len, &pieces),
                "who: read 0 has 4294967296 bases (at most 4294967295)");
        for (int r = 0; r <= 16; r++) off[r] = (uint64_t)r * 0xFFFFFFFFull;
        refused("layout_ranges, 2^32 pieces", rtx::layout_ranges("who", 16, off, lo.data(), hi.data(), 0xFFFFFFFFu, kPiece, h_off, h_len, &pieces),
                "who: the ranges of the batch take more than 2^36 bytes");
    }
    if (bad) { fprintf(stderr, "%d failures\n", bad); return 1; }
    printf("stage_host_check: every layout, every staged range and every rejection as expected\n");
    return 0;
}

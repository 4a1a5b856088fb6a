// Primer trimming on the host (include/raxtax_hip.h): the checks of a pattern list, rtx_primer_search -- one pattern in one read with the
// staging, the plane construction and the search trim_kernel runs (rtx_math.hpp: trim_stage_row, trim_pattern_init, trim_search) -- and
// rtx_trim_apply.  No device involved: tests pin the definition with them, the host mirror cuts its chunks with rtx_trim_apply.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "rtx_internal.hpp"
#include "rtx_math.hpp"

namespace rtx {

int trim_check_patterns(const char *who, const rtx_trim_pattern *pats, uint32_t n) {
    if (n > RTX_TRIM_MAX_PATTERNS) { set_error("%s: %u patterns (at most %d)", who, n, RTX_TRIM_MAX_PATTERNS); return RTX_ERR_INVALID; }
    if (n && !pats) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {
        const rtx_trim_pattern &p = pats[i];
        if (p.len == 0 || p.len > RTX_TRIM_MAX_PATTERN || !p.codes) { set_error("%s: pattern %u has %u codes (1 .. %d)", who, i, p.len, RTX_TRIM_MAX_PATTERN); return RTX_ERR_INVALID; }
        for (uint32_t j = 0; j < p.len; j++)
            if (p.codes[j] == 0 || p.codes[j] > 15) { set_error("%s: pattern %u holds byte %u at %u (codes are 1 .. 15)", who, i, p.codes[j], j); return RTX_ERR_INVALID; }
        if (p.max_errors >= p.len) { set_error("%s: pattern %u allows %u errors in %u codes (fewer than its codes)", who, i, p.max_errors, p.len); return RTX_ERR_INVALID; }
        if (p.window > RTX_TRIM_MAX_WINDOW) { set_error("%s: pattern %u has a window of %u bases (at most %d)", who, i, p.window, RTX_TRIM_MAX_WINDOW); return RTX_ERR_INVALID; }
        if (p.end != RTX_TRIM_5P && p.end != RTX_TRIM_3P) { set_error("%s: pattern %u has end %u (RTX_TRIM_5P or RTX_TRIM_3P)", who, i, p.end); return RTX_ERR_INVALID; }
    }
    return RTX_OK;
}

}  // namespace rtx

extern "C" int rtx_primer_search(const uint8_t *p, uint32_t m, const uint8_t *x, uint64_t n, uint32_t end, uint32_t window,
                                 uint32_t max_errors, uint32_t *cut, uint32_t *errors) {
    if (!cut || !errors || (!x && n)) { rtx::set_error("rtx_primer_search: null argument"); return RTX_ERR_INVALID; }
    *cut = 0;
    *errors = RTX_NO_DIST;
    const rtx_trim_pattern one{p, m, end, max_errors, window};
    if (const int rc = rtx::trim_check_patterns("rtx_primer_search", &one, 1)) return rc;
    rtx::TrimPattern pat;
    rtx::trim_pattern_init(pat, p, m, max_errors, window, end == RTX_TRIM_3P, 0);
    alignas(16) uint8_t row[RTX_TRIM_MAX_WINDOW / 2];
    rtx::trim_stage_row(x, n, pat.w, end == RTX_TRIM_3P, row);
    auto load = [&row](uint32_t c) { rtx::TrimWords t; memcpy(t.w, row + 16u * c, 16); return t; };
    rtx::trim_search(pat, load, (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull), *cut, *errors);
    return RTX_OK;
}

extern "C" int rtx_trim_apply(uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *lo, const uint32_t *hi,
                              uint8_t *out_bases, uint64_t *out_off) {
    if (!out_off || (n && (!base_off || !lo || !hi))) { rtx::set_error("rtx_trim_apply: null argument"); return RTX_ERR_INVALID; }
    out_off[0] = 0;
    for (uint64_t q = 0; q < n; q++) {
        if (base_off[q + 1] < base_off[q] || lo[q] > hi[q] || hi[q] > base_off[q + 1] - base_off[q]) {
            rtx::set_error("rtx_trim_apply: read %llu keeps [%u, %u) of %llu bases", (unsigned long long)q, lo[q], hi[q], (unsigned long long)(base_off[q + 1] - base_off[q]));
            return RTX_ERR_INVALID;
        }
        out_off[q + 1] = out_off[q] + (hi[q] - lo[q]);
    }
    if (out_off[n] && (!bases || !out_bases)) { rtx::set_error("rtx_trim_apply: null argument"); return RTX_ERR_INVALID; }
    auto copy = [&](uint64_t a, uint64_t b) {
        for (uint64_t q = a; q < b; q++)
            if (hi[q] > lo[q]) memcpy(out_bases + out_off[q], bases + base_off[q] + lo[q], hi[q] - lo[q]);
    };
    const unsigned nt = (unsigned)std::min<uint64_t>(rtx::host_threads(4u), (n + 4095) / 4096);
    if (nt <= 1) { copy(0, n); return RTX_OK; }
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; i++) th.emplace_back(copy, n * i / nt, n * (i + 1) / nt);
    for (auto &t : th) t.join();
    return RTX_OK;
}

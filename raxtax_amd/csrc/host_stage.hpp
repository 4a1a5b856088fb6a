// What the front stage objects (rtx_stage.hpp; rtx_trim.hip, rtx_demux.hip, rtx_qual.hip, rtx_screen.hip, rtx_merge.hip, rtx_derep.hip,
// rtx_chimera.hip) and the host mirror (host_front.hpp) do on the host alike: the thread fan, the checks of a batch's offsets and the layout of
// its ranges in 16-byte pieces.  Plain C++ over caller pointers, no HIP: tools/stage_host_check.cpp runs it under the sanitizers on the CPU.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <thread>
#include <vector>

#include "rtx_internal.hpp"

namespace rtx {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Runs fn(k, a, b) over contiguous ranges [a, b) of [0, n): range k on thread k of up to `nt`, one thread per `grain` items at the most;
// inline (k = 0) when one thread suffices.
template <class F>
void parallel_ranges(uint64_t n, unsigned nt, uint64_t grain, F fn) {
    nt = (unsigned)std::min<uint64_t>(nt, (n + grain - 1) / grain);
    if (nt <= 1) { fn(0u, (uint64_t)0, n); return; }
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; k++) th.emplace_back(fn, k, n * k / nt, n * (k + 1) / nt);
    for (auto &t : th) t.join();
}

// The n reads bases[base_off[q] .. base_off[q + 1]) of a batch: RTX_ERR_INVALID (with the error text set, `who` in front) unless the offsets
// are monotone, no read is longer than max_len and `bases` is there for a batch that holds a base.
inline int check_reads(const char *who, uint64_t n, const uint64_t *base_off, const uint8_t *bases, uint64_t max_len) {
    for (uint64_t q = 0; q < n; q++) {
        if (base_off[q + 1] < base_off[q]) { set_error("base_off not monotone at query %llu", (unsigned long long)q); return RTX_ERR_INVALID; }
        const uint64_t len = base_off[q + 1] - base_off[q];
        if (len > max_len) {
            if (max_len == 0xFFFFFFFFull) set_error("%s: read %llu has %llu bases (at most 2^32 - 1)", who, (unsigned long long)q, (unsigned long long)len);
            else set_error("%s: read %llu has %llu bases (at most %llu)", who, (unsigned long long)q, (unsigned long long)len, (unsigned long long)max_len);
            return RTX_ERR_INVALID;
        }
    }
    if (base_off[n] != base_off[0] && !bases) { set_error("%s: null bases", who); return RTX_ERR_INVALID; }
    return RTX_OK;
}

// The ranges [lo[r], hi[r]) of the reads of a batch (both null: the whole reads) laid out back to back, each from a multiple of `piece`
// bytes on: h_off[r] its first piece, h_len[r] its length, *pieces what the batch takes.  RTX_ERR_INVALID (error text set) unless the offsets
// are monotone, no read is longer than max_len, every range lies inside its read and the pieces of the batch number less than 2^32.
inline int layout_ranges(const char *who, uint64_t n, const uint64_t *base_off, const uint32_t *lo_in, const uint32_t *hi_in, uint32_t max_len,
                         uint32_t piece, uint32_t *h_off, uint32_t *h_len, uint64_t *pieces_out) {
    uint64_t pieces = 0;
    for (uint64_t r = 0; r < n; r++) {
        if (base_off[r + 1] < base_off[r]) { set_error("base_off not monotone at query %llu", (unsigned long long)r); return RTX_ERR_INVALID; }
        const uint64_t len = base_off[r + 1] - base_off[r];
        if (len > max_len) { set_error("%s: read %llu has %llu bases (at most %u)", who, (unsigned long long)r, (unsigned long long)len, max_len); return RTX_ERR_INVALID; }
        const uint32_t lo = lo_in ? lo_in[r] : 0u, hi = hi_in ? hi_in[r] : (uint32_t)len;
        if (lo > hi || hi > len) { set_error("%s: read %llu of %llu bases has the range [%u, %u)", who, (unsigned long long)r, (unsigned long long)len, lo, hi); return RTX_ERR_INVALID; }
        h_off[r] = (uint32_t)pieces;
        h_len[r] = hi - lo;
        pieces += ((uint64_t)(hi - lo) + piece - 1u) / piece;
        if (pieces > 0xFFFFFFFFull) { set_error("%s: the ranges of the batch take more than 2^36 bytes", who); return RTX_ERR_INVALID; }
    }
    *pieces_out = pieces;
    return RTX_OK;
}

}  // namespace rtx

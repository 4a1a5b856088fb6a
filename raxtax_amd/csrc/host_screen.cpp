// Contaminant screen on the host (include/raxtax_hip.h): the set -- the canonical 16-mers of the contaminant sequences, sorted once and laid
// out as the table the kernel probes -- the checks of a parameter struct, and rtx_screen_read: one read with the piece and probe functions
// screen_kernel runs (rtx_math.hpp: screen_piece, screen_probe, screen_verdict).  No device involved: tests pin the definition with it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "host_screen.hpp"
#include "rtx_internal.hpp"
#include "rtx_math.hpp"

namespace rtx {

int screen_check_params(const char *who, const rtx_screen_params *p) {
    if (!p) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (p->min_hits < 1u) { set_error("%s: min_hits %u (at least 1)", who, p->min_hits); return RTX_ERR_INVALID; }
    if (p->min_pct > 100u) { set_error("%s: min_pct %u (0 .. 100)", who, p->min_pct); return RTX_ERR_INVALID; }
    return RTX_OK;
}

static uint64_t screen_mix(uint64_t h, uint64_t v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ h >> 29;
}

uint64_t screen_fingerprint(const ScreenSetData &set, const rtx_screen_params &p) {
    const uint64_t h = screen_mix(screen_mix(set.fingerprint, p.min_hits), p.min_pct);
    return h ? h : 1ull;
}

}  // namespace rtx

extern "C" int rtx_screen_set_build(uint64_t n_seqs, const uint8_t *bases, const uint64_t *base_off, rtx_screen_set **out) {
    using namespace rtx;
    if (!out) { set_error("rtx_screen_set_build: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (!base_off || n_seqs == 0) { set_error("rtx_screen_set_build: no sequences"); return RTX_ERR_INVALID; }
    if (n_seqs >= kScreenNone) { set_error("rtx_screen_set_build: %llu sequences (fewer than 2^32 - 1)", (unsigned long long)n_seqs); return RTX_ERR_INVALID; }
    for (uint64_t s = 0; s < n_seqs; s++)
        if (base_off[s + 1] < base_off[s]) { set_error("rtx_screen_set_build: base_off not monotone at sequence %llu", (unsigned long long)s); return RTX_ERR_INVALID; }
    const uint64_t total = base_off[n_seqs] - base_off[0];
    if (total > RTX_SCREEN_MAX_BASES) { set_error("rtx_screen_set_build: %llu bases (at most 2^26)", (unsigned long long)total); return RTX_ERR_INVALID; }
    if (total && !bases) { set_error("rtx_screen_set_build: null bases"); return RTX_ERR_INVALID; }
    try {
        std::vector<uint64_t> keys;  // c << 32 | src: sorted, the lowest source of a value comes first
        keys.reserve(total);
        for (uint64_t s = 0; s < n_seqs; s++) {
            uint32_t fw = 0u, rc = 0u, run = 0u;
            for (uint64_t i = base_off[s]; i < base_off[s + 1]; i++) {
                const uint32_t code = bases[i];
                const bool acgt = code == 1u || code == 2u || code == 4u || code == 8u;
                const uint32_t two = (code >> 1 & 1u) | (code >> 2 & 1u) << 1 | (code >> 3 & 1u) * 3u;
                fw = fw << 2 | two;
                rc = rc >> 2 | (3u - two) << 30;
                run = acgt ? run + 1u : 0u;
                if (run >= kScreenK) keys.push_back((uint64_t)std::min(fw, rc) << 32 | s);
            }
        }
        if (keys.empty()) { set_error("rtx_screen_set_build: the sequences hold no valid window of 16 bases"); return RTX_ERR_INVALID; }
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a >> 32 == b >> 32; }), keys.end());
        auto data = std::make_shared<ScreenSetData>();
        data->n_keys = keys.size();
        uint32_t log2m = 10u;  // kScreenMinSlots
        while ((1ull << log2m) < 2ull * keys.size()) log2m++;
        data->log2m = log2m;
        const uint32_t mask = (1u << log2m) - 1u;
        data->slots.assign((size_t)mask + 1u, ScreenSlot{kScreenNone, kScreenNone});
        uint64_t fp = 0xCBF29CE484222325ull;
        for (const uint64_t k : keys) {
            const uint32_t c = (uint32_t)(k >> 32), home = screen_home(c, log2m);
            uint32_t h = home;
            while (data->slots[h].key != kScreenNone) h = (h + 1u) & mask;
            data->slots[h] = ScreenSlot{c, (uint32_t)k};
            data->max_disp = std::max<uint64_t>(data->max_disp, (h - home) & mask);
            data->n_wrapped += h < home;
            fp = (fp ^ k) * 0x9E3779B97F4A7C15ull;
            fp ^= fp >> 29;
        }
        data->fingerprint = fp;
        auto *set = new rtx_screen_set();
        set->data = std::move(data);
        *out = set;
    } catch (const std::bad_alloc &) {
        set_error("rtx_screen_set_build: no memory for the keys of %llu bases", (unsigned long long)total);
        return RTX_ERR_OOM;
    }
    return RTX_OK;
}

extern "C" void rtx_screen_set_free(rtx_screen_set *set) { delete set; }

extern "C" int rtx_screen_set_info(const rtx_screen_set *set, uint64_t *n_keys, uint64_t *n_slots, uint64_t *max_displacement, uint64_t *n_wrapped,
                                   uint64_t *fingerprint) {
    if (!set || !set->data) { rtx::set_error("rtx_screen_set_info: null argument"); return RTX_ERR_INVALID; }
    if (n_keys) *n_keys = set->data->n_keys;
    if (n_slots) *n_slots = set->data->slots.size();
    if (max_displacement) *max_displacement = set->data->max_disp;
    if (n_wrapped) *n_wrapped = set->data->n_wrapped;
    if (fingerprint) *fingerprint = set->data->fingerprint;
    return RTX_OK;
}

extern "C" int rtx_screen_set_table(const rtx_screen_set *set, const uint32_t **slots, uint32_t *log2m) {
    if (!set || !set->data || !slots || !log2m) { rtx::set_error("rtx_screen_set_table: null argument"); return RTX_ERR_INVALID; }
    static_assert(sizeof(rtx::ScreenSlot) == 8, "a slot is two words");
    *slots = &set->data->slots.data()->key;
    *log2m = set->data->log2m;
    return RTX_OK;
}

extern "C" int rtx_screen_read(const rtx_screen_set *set, const rtx_screen_params *params, const uint8_t *bases, uint64_t len, uint32_t lo, uint32_t hi,
                               uint32_t *windows, uint32_t *hits, uint32_t *first, uint32_t *source, uint32_t *verdict) {
    using namespace rtx;
    if (!set || !set->data || !windows || !hits || !first || !source || !verdict || (len && !bases)) { set_error("rtx_screen_read: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = screen_check_params("rtx_screen_read", params)) return rc;
    if (len > RTX_SCREEN_MAX_READ) { set_error("rtx_screen_read: a read of %llu bases (at most %u)", (unsigned long long)len, RTX_SCREEN_MAX_READ); return RTX_ERR_INVALID; }
    if (lo > hi || hi > len) { set_error("rtx_screen_read: the range [%u, %u) of a read of %llu bases", lo, hi, (unsigned long long)len); return RTX_ERR_INVALID; }
    const uint32_t n = hi - lo;
    std::vector<uint8_t> row((size_t)(n + 15u) / 16u * 16u + 16u, 0);
    if (n) memcpy(row.data(), bases + lo, n);
    const ScreenTable t = set->data->table();
    ScreenAcc acc{0u, 0u, kScreenNone, kScreenNone};
    for (uint32_t pos = 0; pos < n; pos += kScreenPiece) {  // (the pieces one after the other: the first hit seen is the lowest)
        ScreenWords a, b;
        memcpy(a.w, row.data() + pos, 16);
        memcpy(b.w, row.data() + pos + 16u, 16);
        screen_piece(t, a, b, pos, n, acc);
    }
    *windows = acc.windows;
    *hits = acc.hits;
    *first = acc.first;
    *source = acc.source;
    *verdict = screen_verdict(acc.hits, acc.windows, params->min_hits, params->min_pct);
    return RTX_OK;
}

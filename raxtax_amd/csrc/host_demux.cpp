// Sample demultiplexing on the host (include/raxtax_hip.h): the checks of a tag list and its pair table, the list as the kernel takes it
// (rtx_math.hpp: demux_tag_init; rtx_demux.hip uploads it) and rtx_demux_read -- one read with the staging and the function demux_kernel
// runs (trim_stage_row, demux_read).  No device involved: tests pin the definition with it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <algorithm>
#include <cstring>

#include "host_demux.hpp"

namespace rtx {

uint32_t DemuxSet::sample_of(uint32_t i5, uint32_t i3) const {
    const uint32_t slot = (uint32_t)demux_table_slot(n3, i5, i3);
    const auto it = std::lower_bound(pairs.begin(), pairs.end(), std::make_pair(slot, 0u));
    return it != pairs.end() && it->first == slot ? it->second : kDemuxNone;
}

std::vector<uint32_t> DemuxSet::dense_table() const {
    std::vector<uint32_t> t(demux_table_size(n5, n3), kDemuxNone);
    for (const auto &p : pairs) t[p.first] = p.second;
    return t;
}

int demux_build(const char *who, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                const rtx_demux_params *params, DemuxSet &out) {
    if (!tags || !params || (n_pairs && !pairs)) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (n_tags == 0) { set_error("%s: no tags", who); return RTX_ERR_INVALID; }
    uint32_t per_end[2] = {0u, 0u};
    for (uint32_t i = 0; i < n_tags; i++)
        if (tags[i].end <= 1u) per_end[tags[i].end]++;
    for (uint32_t e = 0; e < 2u; e++)
        if (per_end[e] > RTX_DEMUX_MAX_TAGS) { set_error("%s: %u tags at the %s end (at most %d)", who, per_end[e], e ? "3'" : "5'", RTX_DEMUX_MAX_TAGS); return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n_tags; i++) {
        const rtx_demux_tag &t = tags[i];
        if (t.len == 0 || t.len > RTX_DEMUX_MAX_TAG || !t.codes) { set_error("%s: tag %u has %u codes (1 .. %d)", who, i, t.len, RTX_DEMUX_MAX_TAG); return RTX_ERR_INVALID; }
        for (uint32_t j = 0; j < t.len; j++)
            if (t.codes[j] == 0 || t.codes[j] > 15) { set_error("%s: tag %u holds byte %u at %u (codes are 1 .. 15)", who, i, t.codes[j], j); return RTX_ERR_INVALID; }
        if (t.end != RTX_TRIM_5P && t.end != RTX_TRIM_3P) { set_error("%s: tag %u has end %u (RTX_TRIM_5P or RTX_TRIM_3P)", who, i, t.end); return RTX_ERR_INVALID; }
    }
    if (params->max_mismatches > RTX_DEMUX_MAX_MISMATCHES) { set_error("%s: max_mismatches %u (at most %d)", who, params->max_mismatches, RTX_DEMUX_MAX_MISMATCHES); return RTX_ERR_INVALID; }
    if (params->max_offset > RTX_DEMUX_MAX_OFFSET) { set_error("%s: max_offset %u (at most %d)", who, params->max_offset, RTX_DEMUX_MAX_OFFSET); return RTX_ERR_INVALID; }
    DemuxSet s;
    s.n5 = per_end[0];
    s.n3 = per_end[1];
    s.max_mismatches = params->max_mismatches;
    s.max_offset = params->max_offset;
    std::vector<uint32_t> rank(n_tags);  // the place of a tag within its end
    for (uint32_t e = 0; e < 2u; e++)
        for (uint32_t i = 0, r = 0; i < n_tags; i++) {
            if (tags[i].end != e) continue;
            DemuxTag t;
            demux_tag_init(t, tags[i].codes, tags[i].len, e == RTX_TRIM_3P, i);
            s.tags.push_back(t);
            rank[i] = r++;
        }
    s.pairs.reserve(n_pairs);
    for (uint32_t i = 0; i < n_pairs; i++) {
        const rtx_demux_pair &p = pairs[i];
        const bool none5 = p.tag5 == RTX_DEMUX_NO_TAG, none3 = p.tag3 == RTX_DEMUX_NO_TAG;
        if ((!none5 && (p.tag5 >= n_tags || tags[p.tag5].end != RTX_TRIM_5P)) || (!none3 && (p.tag3 >= n_tags || tags[p.tag3].end != RTX_TRIM_3P))) {
            set_error("%s: pair %u names tags %u / %u (a 5' and a 3' tag of the %u given, or RTX_DEMUX_NO_TAG)", who, i, p.tag5, p.tag3, n_tags);
            return RTX_ERR_INVALID;
        }
        if (none5 && none3) { set_error("%s: pair %u names no tag", who, i); return RTX_ERR_INVALID; }
        if (p.sample == RTX_DEMUX_NONE) { set_error("%s: pair %u has the sample RTX_DEMUX_NONE", who, i); return RTX_ERR_INVALID; }
        s.pairs.emplace_back((uint32_t)demux_table_slot(s.n3, none5 ? s.n5 : rank[p.tag5], none3 ? s.n3 : rank[p.tag3]), p.sample);
    }
    std::stable_sort(s.pairs.begin(), s.pairs.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t i = 1; i < s.pairs.size(); i++)
        if (s.pairs[i].first == s.pairs[i - 1].first) {
            const uint32_t i5 = s.pairs[i].first / (s.n3 + 1u), i3 = s.pairs[i].first % (s.n3 + 1u);
            set_error("%s: the pair of 5' tag %u and 3' tag %u is given twice", who, i5 < s.n5 ? s.tags[i5].index : RTX_DEMUX_NO_TAG,
                      i3 < s.n3 ? s.tags[s.n5 + i3].index : RTX_DEMUX_NO_TAG);
            return RTX_ERR_INVALID;
        }
    out = std::move(s);
    return RTX_OK;
}

}  // namespace rtx

extern "C" int rtx_demux_read(const rtx_demux_params *params, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs,
                              uint32_t n_pairs, const uint8_t *read, uint64_t len, uint32_t *sample, uint32_t *lo, uint32_t *hi, uint32_t *hit,
                              uint32_t *info) {
    if (!sample || !lo || !hi || !hit || !info || (!read && len)) { rtx::set_error("rtx_demux_read: null argument"); return RTX_ERR_INVALID; }
    rtx::DemuxSet s;
    if (const int rc = rtx::demux_build("rtx_demux_read", tags, n_tags, pairs, n_pairs, params, s)) return rc;
    if (len > 0xFFFFFFFFull) { rtx::set_error("rtx_demux_read: the read has %llu bases (at most 2^32 - 1)", (unsigned long long)len); return RTX_ERR_INVALID; }
    const uint32_t w = rtx::demux_window(s.max_offset), stride = rtx::trim_row_stride(w);
    alignas(16) uint8_t row5[32], row3[32];
    rtx::trim_stage_row(read, len, w, false, row5);
    rtx::trim_stage_row(read, len, w, true, row3);
    auto pair = [&s](uint32_t i5, uint32_t i3) { return s.sample_of(i5, i3); };
    rtx::demux_read(s.tags.data(), s.n5, s.n3, pair, s.max_mismatches, s.max_offset, rtx::demux_window_of(row5, stride),
                    rtx::demux_window_of(row3, stride), (uint32_t)len, *sample, *lo, *hi, *hit, *info);
    return RTX_OK;
}

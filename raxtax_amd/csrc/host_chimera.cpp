// Chimera check on the host (include/raxtax_hip.h): rtx_chimera_read -- one read against the reference SEQUENCES, no device and no
// index involved: the per-reference prefix counts are summed position by position and only the record is built by the function the
// device runs (rtx_math.hpp: chimera_record).  Tests pin the definition with it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <cstring>
#include <vector>

#include "rtx_internal.hpp"
#include "rtx_math.hpp"

extern "C" int rtx_chimera_read(const rtx_chimera_params *params, const uint8_t *read, uint64_t len, const uint8_t *ref_bases, const uint64_t *ref_off,
                                uint64_t n_refs, rtx_chimera_rec *rec) {
    using namespace rtx;
    if (!rec || (len && !read) || (n_refs && !ref_off)) { set_error("rtx_chimera_read: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = chimera_check_params("rtx_chimera_read", params)) return rc;
    if (n_refs >= kChimNoRef) { set_error("rtx_chimera_read: %llu references (fewer than 2^32 - 1)", (unsigned long long)n_refs); return RTX_ERR_INVALID; }
    for (uint64_t r = 0; r < n_refs; r++)
        if (ref_off[r + 1] < ref_off[r]) { set_error("ref_off not monotone at reference %llu", (unsigned long long)r); return RTX_ERR_INVALID; }
    if (n_refs && ref_off[n_refs] > ref_off[0] && !ref_bases) { set_error("rtx_chimera_read: null ref_bases"); return RTX_ERR_INVALID; }
    const uint32_t S = params->segments;
    const uint32_t len32 = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
    const uint32_t n_pos = chimera_n_pos(len32);
    uint32_t pm[kChimMaxSegments + 1] = {0}, sm[kChimMaxSegments + 1] = {0}, pr[kChimMaxSegments + 1], sr[kChimMaxSegments + 1];
    for (uint32_t s = 0; s <= kChimMaxSegments; s++) pr[s] = sr[s] = kChimNoRef;
    // the windows of the read by k-mer: head[k] -> the first position with it, next[i] -> the next one; seg_of[i]: the segment of window i
    std::vector<uint32_t> head(RTX_NUM_KMERS, kChimNoRef), next(n_pos, kChimNoRef), seg_of(n_pos, 0u);
    uint32_t n_valid = 0;
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t i = chimera_boundary(n_pos, S, s); i < chimera_boundary(n_pos, S, s + 1u); i++) seg_of[i] = s;
    for (uint32_t i = n_pos; i-- > 0u;) {
        uint32_t k;
        if (!chimera_window_kmer(read, i, k)) continue;
        n_valid++;
        next[i] = head[k];
        head[k] = i;
    }
    if (n_valid) {
        std::vector<uint32_t> seen(RTX_NUM_KMERS, kChimNoRef);  // the last reference that counted the k-mer
        for (uint64_t r = 0; r < n_refs; r++) {
            const uint8_t *seq = ref_bases + ref_off[r];
            const uint64_t rl = ref_off[r + 1] - ref_off[r];
            uint32_t cnt[kChimMaxSegments] = {0};
            bool any = false;
            for (uint64_t w = 0; w + 8u <= rl; w++) {
                uint32_t k = 0;
                bool ok = true;
                for (uint32_t j = 0; j < 8u; j++) {
                    const uint32_t c = seq[w + j];
                    ok = ok && (c == 1u || c == 2u || c == 4u || c == 8u);
                    k = (k << 2) | (c == 2u ? 1u : (c == 4u ? 2u : (c == 8u ? 3u : 0u)));
                }
                if (!ok || seen[k] == (uint32_t)r) continue;
                seen[k] = (uint32_t)r;
                for (uint32_t i = head[k]; i != kChimNoRef; i = next[i]) { cnt[seg_of[i]]++; any = true; }
            }
            if (!any) continue;
            uint32_t T = 0, P = 0;
            for (uint32_t s = 0; s < S; s++) T += cnt[s];
            for (uint32_t s = 0; s <= S; s++) {  // P_r[s] and Suf_r[s]; references ascend, so a tie keeps the lower one
                chimera_take(pm[s], pr[s], P, (uint32_t)r);
                chimera_take(sm[s], sr[s], T - P, (uint32_t)r);
                if (s < S) P += cnt[s];
            }
        }
    }
    const ChimRec c = chimera_record(len32, n_valid, S, params->mindelta, pm, pr, sm, sr);
    static_assert(sizeof(ChimRec) == sizeof(rtx_chimera_rec), "twelve uint32");
    std::memcpy(rec, &c, sizeof c);
    return RTX_OK;
}

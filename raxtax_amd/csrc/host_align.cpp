// rtx_semiglobal_distance: the distance of RTX_OPT_IDENTITY on the host (include/raxtax_hip.h) -- the block step and the plane
// construction identity_kernel runs (rtx_math.hpp), column by column and block by block.  No device involved: tests pin the definition
// with it, callers spot-check the device's figures.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <vector>

#include "rtx_internal.hpp"
#include "rtx_math.hpp"

extern "C" int rtx_semiglobal_distance(const uint8_t *q, uint64_t qlen, const uint8_t *r, uint64_t rlen, uint32_t *dist) {
    if (!dist || (!q && qlen) || (!r && rlen)) { rtx::set_error("rtx_semiglobal_distance: null argument"); return RTX_ERR_INVALID; }
    if (qlen >= 0xFFFFFFFFull) { rtx::set_error("rtx_semiglobal_distance: query of %llu bases", (unsigned long long)qlen); return RTX_ERR_INVALID; }
    const uint32_t m = (uint32_t)qlen;
    if (m == 0) { *dist = 0; return RTX_OK; }
    const uint32_t nb = (m + 63u) / 64u;
    std::vector<rtx::IdentityBlock> blk(nb);
    auto fetch = [q](uint32_t j) { return (uint32_t)q[j]; };
    for (uint32_t b = 0; b < nb; b++) rtx::identity_block_init(blk[b], fetch, m, b, false);
    uint32_t score = m, best = m;
    for (uint64_t j = 0; j < rlen; j++) {
        const uint32_t code = rtx::identity_code(r[j]);
        int h = 0;
        for (uint32_t b = 0; b < nb; b++) h = rtx::identity_step(blk[b], code, h, rtx::identity_out_mask(m, b));
        score += (uint32_t)h;
        if (score < best) best = score;
    }
    *dist = best;
    return RTX_OK;
}

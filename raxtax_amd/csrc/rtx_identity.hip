// Alignment identity (RTX_OPT_IDENTITY): the semi-global edit distance of every query of the caller, in the orientation that was classified,
// to its nearest reference (rtx_nearest.hip) -- Myers' bit-vector algorithm in its block form, the blocks of a query spread over the lanes of a
// lane group and run as a systolic array (rtx_math.hpp: identity_block_init, identity_step; rtx_semiglobal_distance is the same on the host).
//
//   lane b of a group owns block b of the query (bases 64 b .. 64 b + 63): Pv, Mv and the four bit planes, twelve 32-bit registers;
//   at step s it runs text column s - b; what it hands to lane b + 1 for the next step -- the text code and its horizontal delta, one
//   register -- moves one lane down per step (a DPP row shift in a group of 16, a shuffle in the whole wave);
//   lane 0 takes the next text code from a chunk of W codes the group loads coalesced every W steps, one chunk ahead of its use
//   (in a group of 16 the chunk rotates one lane per step, so that lane 0 always holds the code that is due);
//   the lane of the last block keeps the score of the query's last row and its minimum: qlen before the first column (the empty substring).
// A pair takes len(r) + blocks - 1 steps.  Two launches: groups of 16 lanes (queries up to 1024 bases, four per wave -- a barcode of 658 bases
// fills 11 of 16 lanes) and whole waves (up to RTX_IDENTITY_MAX_QUERY); the first also writes qlen of every query and RTX_NO_DIST where no
// alignment is due.  The query's bytes come from the batch's INPUT SET (two per byte, or raw) and not from the unpacked bases, which the
// next activation overwrites under RTX_OPT_RUN_AHEAD while this run's back halves are still on the device; a minus-strand query is
// reverse-complemented while its planes are built.
#include <hip/hip_runtime.h>

#include "rtx_kernels.hpp"
#include "rtx_math.hpp"

namespace rtx {

// ids of group g -> group of every id (the device has only group -> ids): once per handle, when the option is switched on
__global__ __launch_bounds__(256) void ref_group_kernel(const uint32_t *goff, const uint32_t *gids, uint32_t n_groups, uint32_t n_refs, uint32_t *ref_grp) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    for (uint32_t i = goff[g]; i < goff[g + 1]; i++)
        if (gids[i] < n_refs) ref_grp[gids[i]] = g;
}

void launch_ref_group(hipStream_t s, const uint32_t *goff, const uint32_t *gids, uint32_t n_groups, uint32_t n_refs, uint32_t *ref_grp) {
    if (n_groups) hipLaunchKernelGGL(ref_group_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, s, goff, gids, n_groups, n_refs, ref_grp);
}

constexpr uint32_t kIdentitySmall = 16u * 64u;  // longest query of a group of 16 lanes

template <uint32_t W>
__global__ __launch_bounds__(256) void identity_kernel(IdentityParams p) {
    static_assert(W == 16u || W == 64u, "a DPP row or the whole wave");
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (W - 1u);
    const uint32_t q = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (64u / W) + lane / W;
    uint32_t qlen = 0, rlen = 0, nb = 0;
    const uint8_t *r = nullptr;
    uint64_t b0 = 0;
    bool mine = false, minus = false;
    if (q < p.n) {
        b0 = p.qoff[q];
        const uint64_t len = p.qoff[q + 1] - b0;
        qlen = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
        const uint32_t ref = p.nearest[q];
        const bool due = ref < p.n_refs && qlen >= 1u && qlen <= RTX_IDENTITY_MAX_QUERY;  // (RTX_NO_REF is no id)
        mine = due && (qlen <= kIdentitySmall) == (W == 16u);
        if (W == 16u && gl == 0u) {
            p.qlen[q] = qlen;
            if (!due) p.dist[q] = RTX_NO_DIST;
        }
        if (mine) {
            const uint32_t g = p.ref_grp[ref];
            const uint64_t r0 = p.rep_off[g];
            rlen = (uint32_t)(p.rep_off[g + 1] - r0);
            r = p.rep_bytes + r0;
            minus = p.strand[q] != 0u;
            nb = (qlen + 63u) >> 6;
        }
    }
    if (__ballot(mine) == 0ull) return;  // (wave-uniform)
    const bool owner = mine && gl < nb;
    IdentityBlock blk{};
    if (owner) {
        const uint8_t *const bytes = p.qbytes;
        if (p.packed) identity_block_init(blk, [=](uint32_t j) { const uint64_t k = b0 + j; return (uint32_t)((bytes[k >> 1] >> ((k & 1u) * 4u)) & 15u); }, qlen, gl, minus);
        else identity_block_init(blk, [=](uint32_t j) { return (uint32_t)bytes[b0 + j]; }, qlen, gl, minus);
    }
    const bool last = owner && gl + 1u == nb;
    const uint64_t out_mask = owner ? identity_out_mask(qlen, gl) : 0ull;
    uint32_t steps = mine && rlen ? rlen + nb - 1u : 0u;
    if (W == 16u) {  // the groups of a wave run in step: as long as its longest pair
        steps = max(steps, (uint32_t)__shfl_xor((int)steps, 16, 64));
        steps = max(steps, (uint32_t)__shfl_xor((int)steps, 32, 64));
    }
    // bytes i W + gl of the text (0 behind its end: never run, a lane's column stays below rlen); taken as they are -- the load is not
    // waited for before the chunk is due, W steps later
    auto load = [&](uint32_t chunk) -> uint32_t {
        const uint32_t i = chunk * W + gl;
        return mine && i < rlen ? (uint32_t)r[i] : 0u;
    };
    uint32_t cur = identity_code(load(0)), nxt = load(1);
    uint32_t hand = 0;  // to the lane below: code | (horizontal delta + 1) << 4
    uint32_t score = qlen, best = qlen;
    for (uint32_t s = 0; s < steps; s++) {  // (wave-uniform)
        const uint32_t k = s & (W - 1u);
        if (s != 0u && k == 0u) {
            cur = identity_code(nxt);
            nxt = load(s / W + 1u);
        }
        uint32_t in, code0;
        if (W == 16u) {
            in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hand, 0x111, 0xF, 0xF, true);  // row_shr:1
            code0 = cur;                                                                       // (lane 0 of the group reads its own)
        } else {
            in = (uint32_t)__shfl_up((int)hand, 1, 64);
            code0 = (uint32_t)__shfl((int)cur, (int)k, 64);
        }
        if (gl == 0u) in = code0 | (1u << 4);  // the first block: the next code of the text, horizontal delta 0
        const uint32_t col = s - gl;
        if (owner && s >= gl && col < rlen) {
            const int h = identity_step(blk, in & 15u, (int)(in >> 4) - 1, out_mask);
            hand = (in & 15u) | ((uint32_t)(h + 1) << 4);
            if (last) {
                score += (uint32_t)h;
                best = min(best, score);
            }
        }
        if (W == 16u) cur = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x12F, 0xF, 0xF, true);  // row_ror:15: lane i takes lane i + 1's
    }
    if (last) p.dist[q] = best;  // (the owner of the last block exists whenever the query is due)
}

void launch_identity(hipStream_t s, const IdentityParams &p) {
    if (!p.n) return;
    const uint32_t waves16 = (p.n + 3u) / 4u;
    hipLaunchKernelGGL(identity_kernel<16u>, dim3((waves16 + 3u) / 4u), dim3(256), 0, s, p);
    if (p.max_len > kIdentitySmall) hipLaunchKernelGGL(identity_kernel<64u>, dim3((p.n + 3u) / 4u), dim3(256), 0, s, p);
}

}  // namespace rtx

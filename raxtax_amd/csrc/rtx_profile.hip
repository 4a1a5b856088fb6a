// The taxon profile of a run (rtx_index_profile_*): per node of the taxonomy the queries whose best lineage reaches it with a confidence at
// or above the cutoff (clade), those that end there (direct) and the sum of their hundredths (conf_sum), accumulated on the device from the
// final rows of every accepted batch (rtx_finalise.hip) -- the per-query step is rtx_math.hpp's profile_step, which the x86 emulation runs
// as well (tests/test_profile_cpu.py).
//
// A lane per position of the processing order (related queries share a wave: few distinct nodes per wave), levels walked from the deepest
// one of the wave up to level 0 so that lanes on one node meet in the same step.  Per level a wave-level group-by: the first lane still to
// be served names its node, a ballot finds the lanes that hold the same one, their count and hundredths are reduced over the wave and the
// leader adds them with one 64-bit integer atomic each -- a million queries under one phylum reach memory as one add per wave.  Integer
// adds: the result does not depend on the order.  (No LDS table per workgroup on top of it: not tried.)
#include <hip/hip_runtime.h>

#include "rtx_kernels.hpp"
#include "rtx_math.hpp"
#include "rtx_wave.hpp"

namespace rtx {

// Sum over the 64 lanes, in every lane; all 64 lanes must be active (DPP inside the rows of 16, the four row totals through v_readlane)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    return ((uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16)) +
           ((uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
}

// ... of 64-bit values (weighted queries: a weight times 64 lanes times 100 hundredths does not fit 32 bits); all 64 lanes active
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

constexpr uint32_t kProfileThreads = 256;

// (no lane leaves early: the reductions run over whole waves)
// W: every query counts with its weight (ProfileParams::weight: the reads it stands for; 0 = not at all) -- wave sums in the place of the
// popcounts, 64-bit throughout; without weights the kernel is the one it was.
template <bool W>
__global__ __launch_bounds__(kProfileThreads) void profile_kernel(ProfileParams p) {
    const uint32_t lane = lane_id();
    const uint64_t pos = (uint64_t)blockIdx.x * kProfileThreads + threadIdx.x;
    bool active = pos < p.n_pos;
    uint64_t q = 0;
    if (active) {
        q = p.perm[pos];
        active = q < p.n_user;  // (both strands: the twins' positions carry nothing of their own)
    }
    ProfileStep st{kProfUnclassifiable, 0u, 0u, nullptr};
    if (active) {
        // the exact matches of the orientation that was chosen: those of the twin for a minus-strand query
        const uint64_t qx = p.strand && p.strand[q] ? q + p.n_user : q;
        st = profile_step(p.src, q, p.override_ok ? exact_only(p.exact, qx) : kTextNoOverride, p.cutoff);
    }
    const unsigned long long w = W && active ? p.weight[q] : 0ull;
    if constexpr (W) {
        const unsigned long long n_act = wave_sum_u64(w);
        const unsigned long long n_cls = wave_sum_u64(st.kind == kProfClassified ? w : 0ull);
        const unsigned long long n_unc = wave_sum_u64(st.kind == kProfUnclassified ? w : 0ull);
        if (lane == 0 && n_act) {
            atomicAdd(p.totals + 0, n_act);
            if (n_cls) atomicAdd(p.totals + 1, n_cls);
            if (n_unc) atomicAdd(p.totals + 2, n_unc);
            if (n_act - n_cls - n_unc) atomicAdd(p.totals + 3, n_act - n_cls - n_unc);
        }
    } else {
        // totals: queries, classified, unclassified, unclassifiable
        const uint32_t n_act = (uint32_t)__popcll(__ballot(active));
        const uint32_t n_cls = (uint32_t)__popcll(__ballot(active && st.kind == kProfClassified));
        const uint32_t n_unc = (uint32_t)__popcll(__ballot(active && st.kind == kProfUnclassified));
        if (lane == 0 && n_act) {
            atomicAdd(p.totals + 0, (unsigned long long)n_act);
            if (n_cls) atomicAdd(p.totals + 1, (unsigned long long)n_cls);
            if (n_unc) atomicAdd(p.totals + 2, (unsigned long long)n_unc);
            if (n_act - n_cls - n_unc) atomicAdd(p.totals + 3, (unsigned long long)(n_act - n_cls - n_unc));
        }
    }
    const uint32_t L = active ? st.L : 0u;
    const uint32_t max_l = wave_max_u32(L);
    uint32_t node = st.node;  // a_{L-1}; walks up as the levels go by
    for (uint32_t d = max_l; d-- > 0u;) {
        const bool part = L > d;  // this lane's path has level d, and `node` is a_d
        const uint32_t h = part ? st.at(d) : 0u;
        const bool direct = part && d + 1u == L;
        unsigned long long todo = __ballot(part);
        while (todo) {  // (wave-uniform)
            const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t key = (uint32_t)__shfl((int)node, (int)lead, 64);
            const bool mine = part && node == key;
            const unsigned long long m = __ballot(mine);
            if constexpr (W) {
                const unsigned long long n_mine = wave_sum_u64(mine ? w : 0ull);
                const unsigned long long n_dir = wave_sum_u64(mine && direct ? w : 0ull);
                const unsigned long long sum_h = wave_sum_u64(mine ? w * h : 0ull);
                if (lane == lead && key < p.n_nodes && n_mine) {
                    atomicAdd(p.clade + key, n_mine);
                    atomicAdd(p.conf_sum + key, sum_h);
                    if (n_dir) atomicAdd(p.direct + key, n_dir);
                }
            } else {
                const uint32_t n_dir = (uint32_t)__popcll(__ballot(mine && direct));
                const uint32_t sum_h = wave_sum_u32(mine ? h : 0u);
                if (lane == lead && key < p.n_nodes) {  // (a node id outside the table: never from a well-formed result)
                    atomicAdd(p.clade + key, (unsigned long long)__popcll(m));
                    atomicAdd(p.conf_sum + key, (unsigned long long)sum_h);
                    if (n_dir) atomicAdd(p.direct + key, (unsigned long long)n_dir);
                }
            }
            todo &= ~m;
        }
        if (part && node < p.n_nodes) node = p.src.parent[node];
    }
}

// The per-sample counters (rtx_index_profile_begin_samples): a lane per position like profile_kernel, the same profile_step, and the same
// wave-level group-by -- once on the sample for the totals, once on (sample, node) for the direct counts of the classified queries: the
// first lane still to be served names its key, a ballot finds the lanes that hold it, their weights are summed over the wave and the
// leader adds them with one 64-bit integer atomic.  No lane leaves early; a query without a sample takes part in nothing.
__global__ __launch_bounds__(kProfileThreads) void profile_samples_kernel(SampleProfileParams sp) {
    const ProfileParams &p = sp.p;
    const uint32_t lane = lane_id();
    const uint64_t pos = (uint64_t)blockIdx.x * kProfileThreads + threadIdx.x;
    bool active = pos < p.n_pos;
    uint64_t q = 0;
    if (active) {
        q = p.perm[pos];
        active = q < p.n_user;
    }
    const uint32_t smp = active ? sp.sample[q] : sp.n_samples;
    active = active && smp < sp.n_samples;
    ProfileStep st{kProfUnclassifiable, 0u, 0u, nullptr};
    if (active) {
        const uint64_t qx = p.strand && p.strand[q] ? q + p.n_user : q;
        st = profile_step(p.src, q, p.override_ok ? exact_only(p.exact, qx) : kTextNoOverride, p.cutoff);
    }
    const unsigned long long w = active ? (p.weight ? p.weight[q] : 1ull) : 0ull;
    unsigned long long todo = __ballot(active);
    while (todo) {  // (wave-uniform) the totals, by sample
        const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t key = (uint32_t)__shfl((int)smp, (int)lead, 64);
        const bool mine = active && smp == key;
        const unsigned long long n_act = wave_sum_u64(mine ? w : 0ull);
        const unsigned long long n_cls = wave_sum_u64(mine && st.kind == kProfClassified ? w : 0ull);
        const unsigned long long n_unc = wave_sum_u64(mine && st.kind == kProfUnclassified ? w : 0ull);
        if (lane == lead && n_act) {
            unsigned long long *t = sp.totals + (size_t)key * 4u;
            atomicAdd(t + 0, n_act);
            if (n_cls) atomicAdd(t + 1, n_cls);
            if (n_unc) atomicAdd(t + 2, n_unc);
            if (n_act - n_cls - n_unc) atomicAdd(t + 3, n_act - n_cls - n_unc);
        }
        todo &= ~__ballot(mine);
    }
    const bool part = active && st.kind == kProfClassified && st.node < p.n_nodes;  // (a node id outside the table: never from a well-formed result)
    const uint64_t slot = (uint64_t)smp * p.n_nodes + st.node;
    todo = __ballot(part);
    while (todo) {  // the direct counts, by (sample, node)
        const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint64_t key = (uint64_t)__shfl((unsigned long long)slot, (int)lead, 64);
        const bool mine = part && slot == key;
        const unsigned long long n_dir = wave_sum_u64(mine ? w : 0ull);
        if (lane == lead && n_dir) atomicAdd(sp.direct + key, n_dir);
        todo &= ~__ballot(mine);
    }
}

void launch_profile_samples(hipStream_t s, const SampleProfileParams &p) {
    if (p.p.n_pos == 0) return;
    const dim3 grid((unsigned)((p.p.n_pos + kProfileThreads - 1u) / kProfileThreads));
    hipLaunchKernelGGL(profile_samples_kernel, grid, dim3(kProfileThreads), 0, s, p);
}

void launch_profile(hipStream_t s, const ProfileParams &p) {
    if (p.n_pos == 0) return;
    const dim3 grid((unsigned)((p.n_pos + kProfileThreads - 1u) / kProfileThreads));
    if (p.weight) hipLaunchKernelGGL(profile_kernel<true>, grid, dim3(kProfileThreads), 0, s, p);
    else hipLaunchKernelGGL(profile_kernel<false>, grid, dim3(kProfileThreads), 0, s, p);
}

}  // namespace rtx

// The device helpers that rtx_otu.hip and rtx_graft.hip share: what a plain code is, the wave scan of 64-bit word mixes, the word of a row
// shifted down by one byte, and the block scan of the three numbering kernels.  Not part of the ABI.
#pragma once

#include "rtx_index.hpp"
#include "rtx_wave.hpp"

namespace rtxi {

__device__ __forceinline__ bool plain(uint32_t c) { return c == 1u || c == 2u || c == 4u || c == 8u; }

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

// word j of the row X (nw words, zero-padded) shifted down by one byte: what word j holds once a code in front of it is deleted
__device__ __forceinline__ uint64_t shifted_word(const uint64_t *X, uint32_t nw, uint32_t j) {
    return (X[j] >> 8) | (j + 1u < nw ? X[j + 1u] << 56 : 0ull);
}

// Inclusive scan of v over the 256 threads of the block (every thread calls); *total = the block's sum.  lds: 4 words.
__device__ __forceinline__ uint32_t block_scan_incl_u32(uint32_t v, uint32_t *lds, uint32_t *total) {
    const uint32_t w = threadIdx.x >> 6;
    v = wave_incl_scan_u32(v);
    if ((threadIdx.x & 63u) == 63u) lds[w] = v;
    __syncthreads();
    uint32_t add = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t s = lds[k];
        if (k < w) add += s;
        tot += s;
    }
    __syncthreads();  // (lds may be written again)
    *total = tot;
    return v + add;
}

}  // namespace rtxi

// The device code that rtx_derep.hip and rtx_tally.hip share: the hash of a read and the chunk-local insert / resolve that finds, among the
// reads of one chunk, the lowest index with every read's sequence (rtx_derep.hip describes the three steps and why no wave waits).  One wave
// per read in the first two, one thread per read in the third; the callers' kernels decide which reads take part.  Not part of the ABI.
#pragma once

#include "rtx_index.hpp"

namespace rtxi {

struct DerepParams {
    const uint8_t *bases;      // one byte per base, padded behind the end (em_load_word)
    const uint64_t *base_off;  // [n + 1]
    uint32_t n;
    uint64_t *hash;            // [n]
    uint32_t *table;           // [2^bits] query + 1; 0: empty
    uint32_t bits;
    uint64_t hash_mask;
    uint32_t *owner;           // [n] the query that holds the slot of q's sequence
    uint32_t *cluster_min;     // [n] at an owner: the lowest query of its cluster (preset to all ones)
    uint32_t *rep;             // [n] | [1] the number of q with rep[q] == q
};

// the 64-bit hash of rtx_exact.hip over the 8-byte words of a sequence, before any mask; the same value in every lane of the wave
__device__ __forceinline__ uint64_t derep_hash_read(const uint8_t *seq, uint64_t len, uint32_t lane) {
    const uint64_t nw = (len + 7u) >> 3;
    uint64_t sum = 0;
    for (uint64_t j = lane; j < nw; j += 64) sum += em_mix_word(em_load_word(seq, len, j), j);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return em_finish(sum, len);
}

// the `len` bytes at a and at b differ (the whole wave asks, the whole wave is answered)
__device__ __forceinline__ bool derep_bytes_differ(const uint8_t *a, const uint8_t *b, uint64_t len, uint32_t lane) {
    const uint64_t nw = (len + 7u) >> 3;
    bool differ = false;
    for (uint64_t j = lane; j < nw; j += 64) differ = differ || em_load_word(a, len, j) != em_load_word(b, len, j);
    return __ballot(differ) != 0ull;
}

// Query q (the whole wave) into the chunk's table: it claims an empty slot and owns itself, or meets an occupant with its bytes, its owner.
__device__ __forceinline__ void derep_insert_read(const DerepParams &p, uint32_t q, uint32_t lane) {
    const uint64_t b0 = p.base_off[q], len = p.base_off[q + 1] - b0;
    const uint8_t *seq = p.bases + b0;
    const uint64_t h = p.hash[q];
    const uint32_t mask = (uint32_t)((1ull << p.bits) - 1ull);
    uint32_t slot = em_slot(h, p.bits);
    uint32_t own = q;
    for (uint64_t probe = 0; probe <= mask; probe++) {  // wave-uniform; the table is at most half full: an empty slot comes
        uint32_t e = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p.table + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (e == 0u) {
            uint32_t old = 0u;
            if (lane == 0) old = atomicCAS(p.table + slot, 0u, q + 1u);
            e = __builtin_amdgcn_readfirstlane(old);
            if (e == 0u) break;  // the slot is this query's: it owns itself
        }
        const uint32_t o = e - 1u;  // an occupant (found, or the winner of the compare-and-swap)
        if (p.hash[o] == h) {
            const uint64_t o0 = p.base_off[o], olen = p.base_off[o + 1] - o0;
            if (olen == len && !derep_bytes_differ(seq, p.bases + o0, len, lane)) { own = o; break; }
        }
        slot = (slot + 1u) & mask;
    }
    if (lane == 0) {
        p.owner[q] = own;
        atomicMin(p.cluster_min + own, q);
    }
}

// the lowest index with q's sequence, whatever the scheduling of the inserts was
__device__ __forceinline__ uint32_t derep_resolve_read(const DerepParams &p, uint32_t q) { return p.cluster_min[p.owner[q]]; }

}  // namespace rtxi

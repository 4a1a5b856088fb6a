// The OTUs of a run on the device (rtx_otu_cluster; raxtax_hip.h, "OTUs of a run"): Swarm's d = 1 clustering of the rows of an rtx_tally_table.
// No alignment: every single-difference variant of a row is looked up in a table of all rows, and the hash of a variant follows from the
// hash of the row in O(1), since the hash is a SUM of position-keyed word mixes (em_mix_word(word, j), em_finish(sum, len)).
//   rows     the arena of rtx_tally.hip: one byte per code, every row from a multiple of 8 bytes on and zero-padded to one, 64 zero bytes behind
//            the end; r_off, r_len, r_size (the total of a row: rows are sorted by it, descending)
//   table    open addressing, 2^tbits >= 2 x rows slots of {tag, row + 1} in 64 bits (0: empty), at most half full.  The 32-bit tag (em_tag)
//            beside the id saves the dependent load of anything of the occupant on a miss; a hit in the tag goes on to the length and then
//            to the bytes: a hash picks the candidates, the bytes decide, always.  Rows above RTX_OTU_MAX_LEN are not in it: nothing links to them.
//   1 insert one wave per row: hash, lane 0 claims the first empty slot with one compare-and-swap (rows are distinct: no compare)
//   2 link   one wave per row x, read-only on the table.  Per wave in LDS: P[j] = the sum of the mixes of x's words in front of word j, and
//            PT[j] = the same over the words of x shifted down by one byte (what lies behind a deleted code).  A lane takes a position i:
//              substitution by c in A, C, G, T (c != x[i]):  sum = P[nw] - mix(w, j) + mix(w with byte i replaced, j), length len
//              deletion (one per run of equal codes):        sum = P[j] + mix(recomposed word j, j) + PT[nwd] - PT[j + 1], length len - 1;
//                the recomposed word takes its low bytes from x's word j and the rest from the shifted word j; nwd, the words of len - 1
//                codes, may be one less than nw -- then the last word is gone (em_mix_word(0, j) is not 0: it must not be added).
//            A candidate is confirmed word by word, the edited word first.  Every undirected link is emitted once: a deletion from the longer
//            row; a substitution from x iff x's code there is not one of A, C, G, T (then y cannot generate x) or x > y.  Links are
//            appended through a counter that goes on counting past the capacity while the writes stay inside it: the host grows the
//            buffer to the count and runs the pass once more.
//   3 label  label[y] = y; one thread per link (a, b), a < b, hence size[a] >= size[b]: atomicMin(label[b], label[a]), and the other way
//            round when the sizes are equal.  kLabelRounds launches per read-back of their flags, to the fixed point: a round without a
//            change.  No wave waits for another: a round reads what it finds and the next one picks up the rest.
//   4 number the seeds (label[y] == y) are numbered in rank order by a scan; otu[y] = the number of label[y]; members by atomicAdd.
#include <atomic>

#include "host_otu.hpp"
#include "rtx_derep_dev.hpp"
#include "rtx_otu_dev.hpp"  // plain, wave_incl_scan_u64, shifted_word, block_scan_incl_u32: shared with rtx_graft.hip
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"

namespace {

std::atomic<uint64_t> g_otu_hash_mask{~0ull};  // RTX_DEFAULT_OTU_HASH_MASK (tests: a hash of two bits, so that every probe ends in the byte compare)

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLabelRounds = 8;  // launches per read-back of the changed flags

struct OtuParams {
    const uint8_t *arena;
    const uint64_t *r_off;   // [n] (multiples of 8)
    const uint32_t *r_len;   // [n]
    const uint64_t *r_size;  // [n]
    uint32_t n;
    unsigned long long *table;  // [2^tbits] tag | (row + 1) << 32
    uint32_t tbits;
    uint64_t hash_mask;
    uint32_t lds_words;      // per array and wave: the most words of a row that takes part, + 1
    uint2 *links;            // [link_cap] (a, b), a < b
    uint64_t link_cap;
    unsigned long long *link_count;
    uint32_t *label;         // [n]
    uint32_t *changed;       // [kLabelRounds]
    uint32_t *seed_no;       // [n] at a seed: its OTU
    uint32_t *otu;           // [n]
    uint32_t *block_sum;     // [ceil(n / 256)]
    uint32_t *members;       // [n] (the first n_otus in use)
    uint32_t *n_otus;        // [1]
};

__global__ __launch_bounds__(256) void otu_insert_kernel(OtuParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (x >= p.n) return;  // wave-uniform
    const uint32_t len = p.r_len[x];
    if (len == 0u || len > RTX_OTU_MAX_LEN) return;  // wave-uniform
    const uint64_t h = derep_hash_read(p.arena + p.r_off[x], len, lane) & p.hash_mask;
    if (lane != 0u) return;
    const uint32_t mask = (uint32_t)((1ull << p.tbits) - 1ull);
    const unsigned long long mine = (unsigned long long)em_tag(h) | (unsigned long long)(x + 1u) << 32;
    uint32_t slot = em_slot(h, p.tbits);
    for (uint64_t probe = 0; probe <= mask; probe++) {  // the table is at most half full: an empty slot comes
        if (atomicCAS(p.table + slot, 0ull, mine) == 0ull) return;
        slot = (slot + 1u) & mask;
    }
}

// The row of `len` codes whose word sum is `sum`: its rank, or kNone.  same(y): the bytes of row y (of that length) are the variant's.
template <class Same>
__device__ __forceinline__ uint32_t otu_probe(const OtuParams &p, uint64_t sum, uint32_t len, Same same) {
    const uint64_t h = em_finish(sum, len) & p.hash_mask;
    const uint32_t tag = em_tag(h), mask = (uint32_t)((1ull << p.tbits) - 1ull);
    uint32_t slot = em_slot(h, p.tbits);
    for (uint64_t probe = 0; probe <= mask; probe++) {  // read-only; bounded by the table
        const unsigned long long s = p.table[slot];
        if (s == 0ull) break;
        if ((uint32_t)s == tag) {
            const uint32_t y = (uint32_t)(s >> 32) - 1u;
            if (p.r_len[y] == len && same(y)) return y;
        }
        slot = (slot + 1u) & mask;
    }
    return kNone;
}

__device__ __forceinline__ void otu_emit(const OtuParams &p, uint32_t x, uint32_t y) {
    const unsigned long long at = atomicAdd(p.link_count, 1ull);  // (counts on past the capacity: the host sees what the pass needs)
    if (at < p.link_cap) p.links[at] = x < y ? make_uint2(x, y) : make_uint2(y, x);
}

// (no thread leaves early: the block meets at the barrier between the sums and the probes)
__global__ __launch_bounds__(256) void otu_link_kernel(OtuParams p) {
    extern __shared__ uint64_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * 4u + wv;
    const uint32_t len = x < p.n ? p.r_len[x] : 0u;
    const bool active = len != 0u && len <= RTX_OTU_MAX_LEN;            // wave-uniform
    const uint32_t nw = (len + 7u) >> 3, nwd = (len + 6u) >> 3;         // the words of len and of len - 1 codes
    const uint64_t *X = reinterpret_cast<const uint64_t *>(p.arena + (active ? p.r_off[x] : 0ull));
    uint64_t *P = lds + (size_t)wv * 2u * p.lds_words, *PT = P + p.lds_words;  // P[0 .. nw], PT[0 .. nwd]: nw + 1 <= lds_words
    if (active) {
        uint64_t carry = 0, carry_t = 0;
        if (lane == 0u) { P[0] = 0; PT[0] = 0; }
        for (uint32_t base = 0; base < nw; base += 64u) {  // wave-uniform
            const uint32_t j = base + lane;
            const uint64_t v = wave_incl_scan_u64(j < nw ? em_mix_word(X[j], j) : 0ull, lane);
            const uint64_t t = wave_incl_scan_u64(j < nwd ? em_mix_word(shifted_word(X, nw, j), j) : 0ull, lane);
            if (j < nw) P[j + 1u] = carry + v;
            if (j < nwd) PT[j + 1u] = carry_t + t;
            carry += __shfl(v, 63, 64);
            carry_t += __shfl(t, 63, 64);
        }
    }
    __syncthreads();
    if (!active) return;
    const uint64_t S = P[nw], ST = PT[nwd];
    for (uint32_t i = lane; i < len; i += 64u) {
        const uint32_t j = i >> 3, k8 = (i & 7u) * 8u;
        const uint64_t w = X[j], low = (1ull << k8) - 1ull;
        const uint32_t a = (uint32_t)(w >> k8) & 0xFFu;
        const uint64_t rest = S - em_mix_word(w, j);
#pragma unroll
        for (uint32_t c = 1u; c <= 8u; c <<= 1) {  // x[i] replaced by c
            if (c == a) continue;
            const uint64_t w2 = (w & ~(0xFFull << k8)) | (uint64_t)c << k8;
            const uint32_t y = otu_probe(p, rest + em_mix_word(w2, j), len, [&](uint32_t o) {
                const uint64_t *Y = reinterpret_cast<const uint64_t *>(p.arena + p.r_off[o]);
                if (Y[j] != w2) return false;
                for (uint32_t m = 0; m < nw; m++)
                    if (m != j && Y[m] != X[m]) return false;
                return true;
            });
            if (y != kNone && (!plain(a) || x > y)) otu_emit(p, x, y);
        }
        if (len < 2u) continue;  // (the table holds no empty row)
        const uint64_t t = shifted_word(X, nw, j);
        if (i + 1u < len && ((uint32_t)(t >> k8) & 0xFFu) == a) continue;  // inside a run of equal codes: the last one of the run is deleted
        const bool gone = j >= nwd;                                         // x[i] was the only code of the last word
        const uint64_t w2 = (w & low) | (t & ~low);
        const uint64_t sum = gone ? P[j] : P[j] + em_mix_word(w2, j) + (ST - PT[j + 1u]);
        const uint32_t y = otu_probe(p, sum, len - 1u, [&](uint32_t o) {
            const uint64_t *Y = reinterpret_cast<const uint64_t *>(p.arena + p.r_off[o]);
            if (!gone && Y[j] != w2) return false;
            for (uint32_t m = 0; m < nwd; m++)
                if (m != j && Y[m] != (m < j ? X[m] : shifted_word(X, nw, m))) return false;
            return true;
        });
        if (y != kNone) otu_emit(p, x, y);
    }
}

__global__ __launch_bounds__(256) void otu_label_init_kernel(OtuParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < p.n) p.label[i] = i;
}

__global__ __launch_bounds__(256) void otu_label_kernel(OtuParams p, uint64_t n_links, uint32_t round) {
    const uint64_t l = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (l >= n_links) return;
    const uint2 e = p.links[l];  // a < b: size[a] >= size[b]
    const uint32_t la = __hip_atomic_load(p.label + e.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t lb = __hip_atomic_load(p.label + e.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (la < lb) {
        atomicMin(p.label + e.y, la);
        p.changed[round] = 1u;
    } else if (lb < la && p.r_size[e.x] == p.r_size[e.y]) {
        atomicMin(p.label + e.x, lb);
        p.changed[round] = 1u;
    }
}

// (no thread leaves early in the three kernels of the scan: the block scans as a whole)
__global__ __launch_bounds__(256) void otu_seed_count_kernel(OtuParams p) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t tot;
    (void)block_scan_incl_u32(i < p.n && p.label[i] == i ? 1u : 0u, lds, &tot);
    if (threadIdx.x == 0) p.block_sum[blockIdx.x] = tot;
}

// one block: the block sums become their exclusive scan, their total the number of OTUs
__global__ __launch_bounds__(256) void otu_scan_blocks_kernel(OtuParams p, uint32_t n_blocks) {
    __shared__ uint32_t lds[4];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 256u) {  // block-uniform
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? p.block_sum[i] : 0u;
        uint32_t tot;
        const uint32_t inc = block_scan_incl_u32(v, lds, &tot);
        if (i < n_blocks) p.block_sum[i] = carry + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *p.n_otus = carry;
}

__global__ __launch_bounds__(256) void otu_seed_number_kernel(OtuParams p) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool seed = i < p.n && p.label[i] == i;
    uint32_t tot;
    const uint32_t inc = block_scan_incl_u32(seed ? 1u : 0u, lds, &tot);
    if (seed) p.seed_no[i] = p.block_sum[blockIdx.x] + inc - 1u;
}

__global__ __launch_bounds__(256) void otu_assign_kernel(OtuParams p) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t k = p.seed_no[p.label[i]];  // (label[i] <= i is a seed: a label is the lowest rank that reaches the row, and that row reaches itself first)
    p.otu[i] = k;
    if (k < p.n) atomicAdd(p.members + k, 1u);  // (seed_no is preset to all ones: a label that is no seed shows on the host, and writes nowhere)
}

struct OtuStage : StageShell {
    DevBuf<uint8_t> d_arena;
    DevBuf<uint64_t> d_off, d_size;
    DevBuf<uint32_t> d_len, d_label, d_changed, d_seed_no, d_otu, d_block_sum, d_members, d_n_otus;
    DevBuf<unsigned long long> d_table, d_link_count;
    DevBuf<uint2> d_links;
    PinBuf<uint8_t> h_arena;
    PinBuf<uint64_t> h_off, h_size, h_count;
    PinBuf<uint32_t> h_len, h_changed, h_otu, h_members, h_n_otus;
    PinBuf<uint2> h_links;
};

int cluster(OtuStage *st, const rtx_tally_view &v, const rtx_otu_params &prm, rtx_otu &o) {
    const uint64_t n = v.n_entries;
    hipStream_t s = st->stream;
    int rc;
    double t0 = now_s();
    // the rows as the arena of rtx_tally.hip: every row from a multiple of 8 bytes on, zero-padded
    if ((rc = st->h_off.resize(n + 1)) || (rc = st->h_len.resize(n)) || (rc = st->h_size.resize(n))) return rc;
    uint64_t total = 0;
    uint32_t max_nw = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = v.base_off[r + 1] - v.base_off[r];
        st->h_off[r] = total;
        st->h_len[r] = (uint32_t)len;  // (a row of the table keeps its length in 32 bits)
        st->h_size[r] = v.sizes[r];
        total += (len + 7u) & ~7ull;
        if (len > RTX_OTU_MAX_LEN) o.long_rows++;
        else max_nw = std::max(max_nw, (uint32_t)((len + 7u) >> 3));
    }
    st->h_off[n] = total;
    if ((rc = st->h_arena.resize(total + 64))) return rc;
    {
        uint8_t *arena = st->h_arena.data();
        const uint64_t *off = st->h_off.data();
        parallel_ranges(n, rtx::host_threads(4u), 4096, [=](unsigned, uint64_t a, uint64_t b) {
            for (uint64_t r = a; r < b; r++) {
                const uint64_t len = v.base_off[r + 1] - v.base_off[r];
                std::memcpy(arena + off[r], v.bases + v.base_off[r], len);
                std::memset(arena + off[r] + len, 0, off[r + 1] - off[r] - len);
            }
        });
        std::memset(arena + total, 0, 64);
    }
    uint32_t tbits = 3;
    while ((1ull << tbits) < 2ull * n) tbits++;
    const size_t slots = (size_t)1 << tbits;
    const uint32_t n_blocks = (uint32_t)((n + 255u) / 256u);
    uint64_t link_cap = prm.initial_links ? prm.initial_links : std::max<uint64_t>(1024, 4 * n);
    if ((rc = st->d_arena.alloc(total + 64)) || (rc = st->d_off.alloc(n + 1)) || (rc = st->d_len.alloc(n)) || (rc = st->d_size.alloc(n)) || (rc = st->d_table.alloc(slots)) ||
        (rc = st->d_links.alloc(link_cap)) || (rc = st->d_link_count.alloc(1)) || (rc = st->d_label.alloc(n)) || (rc = st->d_changed.alloc(kLabelRounds)) ||
        (rc = st->d_seed_no.alloc(n)) || (rc = st->d_otu.alloc(n)) || (rc = st->d_block_sum.alloc(n_blocks)) || (rc = st->d_members.alloc(n)) || (rc = st->d_n_otus.alloc(1)) ||
        (rc = st->h_count.resize(1)) || (rc = st->h_changed.resize(kLabelRounds)) || (rc = st->h_otu.resize(n)) || (rc = st->h_members.resize(n)) || (rc = st->h_n_otus.resize(1)))
        return rc;
    RTX_HIP(hipMemcpyAsync(st->d_arena.p, st->h_arena.data(), total + 64, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_off.p, st->h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_len.p, st->h_len.data(), n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_size.p, st->h_size.data(), n * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemsetAsync(st->d_table.p, 0, slots * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_members.p, 0, n * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_seed_no.p, 0xFF, n * 4, s));
    OtuParams p{};
    p.arena = st->d_arena.p;
    p.r_off = st->d_off.p;
    p.r_len = st->d_len.p;
    p.r_size = st->d_size.p;
    p.n = (uint32_t)n;
    p.table = st->d_table.p;
    p.tbits = tbits;
    p.hash_mask = g_otu_hash_mask.load();
    p.lds_words = max_nw + 1u;
    p.links = st->d_links.p;
    p.link_cap = link_cap;
    p.link_count = st->d_link_count.p;
    p.label = st->d_label.p;
    p.changed = st->d_changed.p;
    p.seed_no = st->d_seed_no.p;
    p.otu = st->d_otu.p;
    p.block_sum = st->d_block_sum.p;
    p.members = st->d_members.p;
    p.n_otus = st->d_n_otus.p;
    const dim3 waves((unsigned)((n + 3u) / 4u)), threads(n_blocks);
    hipLaunchKernelGGL(otu_insert_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(otu_label_init_kernel, threads, dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(s));
    double t1 = now_s();
    o.seconds[0] = t1 - t0;

    // the links: a pass, and once more when the buffer was too small for what it counted
    const size_t lds_bytes = (size_t)4 * 2 * p.lds_words * sizeof(uint64_t);  // at most 4 x 2 x 513 x 8 = 32 832 bytes
    uint64_t n_links = 0;
    for (o.link_passes = 0;;) {
        RTX_HIP(hipMemsetAsync(st->d_link_count.p, 0, 8, s));
        hipLaunchKernelGGL(otu_link_kernel, waves, dim3(256), lds_bytes, s, p);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipMemcpyAsync(st->h_count.data(), st->d_link_count.p, 8, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipStreamSynchronize(s));
        o.link_passes++;
        n_links = st->h_count[0];
        if (n_links <= link_cap) break;
        if (o.link_passes >= 2u) { set_error("rtx_otu_cluster: the second link pass counts %llu links, the first one counted %llu", (unsigned long long)n_links, (unsigned long long)link_cap); return RTX_ERR_HIP; }
        link_cap = n_links;  // (the count does not depend on the scheduling: the second pass fits)
        st->d_links.release();
        if ((rc = st->d_links.alloc(link_cap))) return rc;
        p.links = st->d_links.p;
        p.link_cap = link_cap;
    }
    double t2 = now_s();
    o.seconds[1] = t2 - t1;

    // the labels, to the fixed point
    if (n_links) {
        const dim3 per_link((unsigned)((n_links + 255u) / 256u));
        for (bool done = false; !done;) {
            RTX_HIP(hipMemsetAsync(st->d_changed.p, 0, kLabelRounds * 4, s));
            for (uint32_t r = 0; r < kLabelRounds; r++) hipLaunchKernelGGL(otu_label_kernel, per_link, dim3(256), 0, s, p, n_links, r);
            RTX_HIP(hipGetLastError());
            RTX_HIP(hipMemcpyAsync(st->h_changed.data(), st->d_changed.p, kLabelRounds * 4, hipMemcpyDeviceToHost, s));
            RTX_HIP(hipStreamSynchronize(s));
            for (uint32_t r = 0; r < kLabelRounds && !done; r++) {
                o.rounds++;
                done = st->h_changed[r] == 0u;  // a round that changed nothing: nothing was written while it read
            }
        }
    }
    hipLaunchKernelGGL(otu_seed_count_kernel, threads, dim3(256), 0, s, p);
    hipLaunchKernelGGL(otu_scan_blocks_kernel, dim3(1), dim3(256), 0, s, p, n_blocks);
    hipLaunchKernelGGL(otu_seed_number_kernel, threads, dim3(256), 0, s, p);
    hipLaunchKernelGGL(otu_assign_kernel, threads, dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipMemcpyAsync(st->h_n_otus.data(), st->d_n_otus.p, 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    double t3 = now_s();
    o.seconds[2] = t3 - t2;

    const uint64_t n_otus = st->h_n_otus[0];
    if (n_otus == 0 || n_otus > n) { set_error("rtx_otu_cluster: %llu OTUs of %llu rows", (unsigned long long)n_otus, (unsigned long long)n); return RTX_ERR_HIP; }
    if ((rc = st->h_links.resize(std::max<uint64_t>(1, n_links)))) return rc;
    RTX_HIP(hipMemcpyAsync(st->h_otu.data(), st->d_otu.p, n * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_members.data(), st->d_members.p, n_otus * 4, hipMemcpyDeviceToHost, s));
    if (n_links) RTX_HIP(hipMemcpyAsync(st->h_links.data(), st->d_links.p, n_links * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    std::vector<uint64_t> keys(n_links);
    for (uint64_t l = 0; l < n_links; l++) {
        const uint2 e = st->h_links[l];
        if (e.x >= e.y || e.y >= n) { set_error("rtx_otu_cluster: link %llu is (%u, %u) of %llu rows", (unsigned long long)l, e.x, e.y, (unsigned long long)n); return RTX_ERR_HIP; }
        keys[l] = (uint64_t)e.x << 32 | e.y;
    }
    std::sort(keys.begin(), keys.end());  // the order of the appends is the scheduling's, the set is not
    o.link_a.resize(n_links);
    o.link_b.resize(n_links);
    for (uint64_t l = 0; l < n_links; l++) { o.link_a[l] = (uint32_t)(keys[l] >> 32); o.link_b[l] = (uint32_t)keys[l]; }
    o.otu.assign(st->h_otu.data(), st->h_otu.data() + n);
    for (uint64_t r = 0; r < n; r++)
        if (o.otu[r] >= n_otus) { set_error("rtx_otu_cluster: row %llu is in OTU %u of %llu", (unsigned long long)r, o.otu[r], (unsigned long long)n_otus); return RTX_ERR_HIP; }
    rtx::otu_sums(o, v);
    bool same = o.n_otus == n_otus;
    for (uint64_t k = 0; same && k < n_otus; k++) same = o.members[k] == st->h_members[k];
    if (!same) { set_error("rtx_otu_cluster: the members the device counted are not those of its map"); return RTX_ERR_HIP; }
    o.seconds[3] = now_s() - t3;
    return RTX_OK;
}

}  // namespace

namespace rtxi {
void set_otu_hash_mask(uint64_t mask) { g_otu_hash_mask.store(mask); }
uint64_t otu_hash_mask() { return g_otu_hash_mask.load(); }  // (rtx_graft.hip hashes under the same mask)
}  // namespace rtxi

extern "C" int rtx_otu_cluster(int device, rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_otu_params prm{};
    if (const int rc = rtx::otu_open("rtx_otu_cluster", table, params, out, &v, &prm)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto *o = new rtx_otu();
    int rc = RTX_OK;
    if (v.n_entries == 0) {
        rtx::otu_sums(*o, v);  // (no row: nothing to upload)
    } else {
        auto *st = new OtuStage();
        rc = st->open(device);
        if (!rc) rc = cluster(st, v, prm, *o);
        destroy(st);
    }
    if (rc) { delete o; return rc; }
    *out = o;
    return RTX_OK;
}

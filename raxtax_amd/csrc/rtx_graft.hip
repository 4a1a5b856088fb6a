// Fastidious grafting on the device (rtx_otu_graft; raxtax_hip.h, "Fastidious grafting"): the light OTUs of a d = 1 clustering grafted onto a
// heavy OTU that holds a row at most two differences away.  No alignment and no pair of rows is ever compared that a hash did not pick: rows
// x and y are near iff their balls B1 share a string, so the strings of the heavy rows' balls go into a Bloom filter, the strings of the
// light rows' balls are tested against it, and what passes is verified against the table of all rows -- the bytes decide, always.
//   rows     arena, offsets, lengths and the {tag, row + 1} table as rtx_otu.hip lays them out (the table is filled on the host here: the
//            stage inserts nothing), one heavy flag per row, the OTU of every row
//   sums     per wave in LDS, for a row of nw words: P[j] = the sum of the mixes of the words in front of word j; PT[j] = the same over the
//            words shifted DOWN by one byte (what lies behind a deleted code); PU[j] = the same over the words shifted UP by one byte,
//            u_j = w_j << 8 | w_{j-1} >> 56 (what lies behind an inserted code), nwi = the words of len + 1 codes of them.  Then
//              substitution of x[i] by c:  P[nw] - mix(w, j) + mix(w with byte i replaced, j), length len
//              deletion of x[i]:           P[j] + mix(low bytes of w | high bytes of the shifted-down word, j) + PT[nwd] - PT[j + 1], len - 1
//                                          (P[j] alone when x[i] was the only code of the last word: em_mix_word(0, j) is not 0)
//              insertion of c in front of x[i] (i = len: behind the end):
//                                          P[j] + mix(low bytes of w | c | the other bytes of w one up, j) + PU[nwi] - PU[j + 1], len + 1
//            Out of a run of equal codes one deletion is taken (the last code of the run), and c is not inserted in front of an equal
//            code (behind it gives the same string): every string of a ball is enumerated once, for the cost and for the counters.
//   1 bloom  one wave per heavy row, lanes over positions: every string of B1(x) sets k = 4 bits with atomicOr.  OR commutes.
//   2 test   one wave per light row, the same enumeration, read-only on the filter: a string whose 4 bits are set is appended as the
//            candidate (row, kind, position, code) through a counter that goes on counting past the capacity.
//   3 verify one wave per candidate: the string v is built as words in LDS with its own P / PT / PU, and every row y with v in B1(y) is
//            looked up: v; v with a plain code replaced by any other code of the list; v with a code of the list inserted; v with a plain
//            code deleted.  The list is A, C, G, T and whatever other byte occurs in a heavy row, so for rows over A, C, G, T this is
//            B1(v).  (B1(v) alone would miss it when y holds an ambiguity code where v holds the base that replaced it.)  A heavy y found
//            lowers parent[x] with atomicMin.
//   4 resolve key[otu[x]] = min (parent[x] << 32 | x) over the light rows with a parent; the OTUs without a key survive and are numbered by
//            a scan in the order of their old numbers; a grafted OTU takes the number of otu[parent]; otu'[r] follows, members by atomicAdd.
#include <atomic>

#include "host_otu.hpp"
#include "rtx_otu_dev.hpp"
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"

namespace rtxi {
uint64_t otu_hash_mask();  // (rtx_otu.hip) RTX_DEFAULT_OTU_HASH_MASK as it stands now
}

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kBloomK = 4;
enum : uint32_t { kSelf = 0, kSub = 1, kDel = 2, kIns = 3 };

struct GraftParams {
    const uint8_t *arena;
    const uint64_t *r_off;   // [n] (multiples of 8)
    const uint32_t *r_len;   // [n]
    const uint8_t *heavy;    // [n]
    const uint32_t *otu;     // [n]
    uint32_t n, n_otus;
    const unsigned long long *table;  // [2^tbits] tag | (row + 1) << 32
    uint32_t tbits;
    uint64_t hash_mask;
    uint32_t lds_words;      // per array and wave: the most words of a row that takes part, + 2
    uint32_t *bloom;         // [2^bloom_log2 / 32]
    uint64_t bloom_mask;     // 2^bloom_log2 - 1
    const uint8_t *codes;    // [n_codes] 1, 2, 4, 8, then every other byte of the heavy rows
    uint32_t n_codes;
    uint2 *cand;             // [cand_cap] (row, kind | code << 2 | position << 16)
    uint64_t cand_cap;
    unsigned long long *counters;  // variants, candidates, confirmed
    uint32_t *parent;        // [n]
    unsigned long long *key; // [n_otus]
    uint32_t *new_no;        // [n_otus] old_to_new
    uint32_t *block_sum;     // [ceil(n_otus / 256)]
    uint32_t *otu_new;       // [n]
    uint32_t *members;       // [n_otus] (the first n_new in use)
    uint32_t *n_new;         // [1]
};

__device__ __forceinline__ uint64_t word_at(const uint64_t *X, uint32_t nw, uint32_t m) { return m < nw ? X[m] : 0ull; }

// word m <= nw of the row shifted up by one byte: what word m holds once a code in front of it is inserted
__device__ __forceinline__ uint64_t up_word(const uint64_t *X, uint32_t nw, uint32_t m) {
    return (word_at(X, nw, m) << 8) | (m ? X[m - 1u] >> 56 : 0ull);
}

// word m of the string that the edit (kind, i, c) makes of the row X; m is a word of that string
__device__ __forceinline__ uint64_t variant_word(const uint64_t *X, uint32_t nw, uint32_t kind, uint32_t i, uint32_t c, uint32_t m) {
    const uint32_t j = i >> 3, k8 = (i & 7u) * 8u;
    if (kind == kSelf || m < j) return word_at(X, nw, m);
    const uint64_t low = (1ull << k8) - 1ull;
    if (kind == kSub) return m == j ? (X[j] & ~(0xFFull << k8)) | (uint64_t)c << k8 : word_at(X, nw, m);
    if (kind == kDel) return m == j ? (X[j] & low) | (shifted_word(X, nw, j) & ~low) : shifted_word(X, nw, m);
    const uint64_t w = word_at(X, nw, j);
    return m == j ? (w & low) | (uint64_t)c << k8 | ((w & ~low) << 8) : up_word(X, nw, m);
}

// P[0 .. nw], PT[0 .. nwd], PU[0 .. nwi] of the row X of len >= 1 codes; the whole wave calls
__device__ __forceinline__ void build_sums(const uint64_t *X, uint32_t len, uint32_t nw, uint64_t *P, uint64_t *PT, uint64_t *PU, uint32_t lane) {
    const uint32_t nwd = (len + 6u) >> 3, nwi = (len + 8u) >> 3;
    uint64_t carry = 0, carry_t = 0, carry_u = 0;
    if (lane == 0u) { P[0] = 0; PT[0] = 0; PU[0] = 0; }
    for (uint32_t base = 0; base < nwi; base += 64u) {  // wave-uniform
        const uint32_t j = base + lane;
        const uint64_t v = wave_incl_scan_u64(j < nw ? em_mix_word(X[j], j) : 0ull, lane);
        const uint64_t t = wave_incl_scan_u64(j < nwd ? em_mix_word(shifted_word(X, nw, j), j) : 0ull, lane);
        const uint64_t u = wave_incl_scan_u64(j < nwi ? em_mix_word(up_word(X, nw, j), j) : 0ull, lane);
        if (j < nw) P[j + 1u] = carry + v;
        if (j < nwd) PT[j + 1u] = carry_t + t;
        if (j < nwi) PU[j + 1u] = carry_u + u;
        carry += __shfl(v, 63, 64);
        carry_t += __shfl(t, 63, 64);
        carry_u += __shfl(u, 63, 64);
    }
}

// Every string of the ball of X, once: f(sum of its word mixes, its length, kind, position, code).  Inverse = false: B1(X), the codes are
// A, C, G, T.  Inverse = true: the rows that have X in THEIR ball -- a plain code replaced by another code of the list, a code of the list
// inserted, a plain code deleted.  Lanes take positions; the sums are in LDS.
template <bool Inverse, class F>
__device__ __forceinline__ void for_ball(const uint64_t *X, uint32_t len, uint32_t nw, const uint64_t *P, const uint64_t *PT, const uint64_t *PU, uint32_t lane,
                                         const uint8_t *codes, uint32_t n_codes, F f) {
    const uint32_t nwd = (len + 6u) >> 3, nwi = (len + 8u) >> 3;
    const uint64_t S = P[nw], ST = PT[nwd], SU = PU[nwi];
    const uint32_t nc = Inverse ? n_codes : 4u;
    if (lane == 0u) f(S, len, (uint32_t)kSelf, 0u, 0u);
    for (uint32_t i = lane; i <= len; i += 64u) {
        const uint32_t j = i >> 3, k8 = (i & 7u) * 8u;
        const uint64_t w = word_at(X, nw, j), low = (1ull << k8) - 1ull;
        const uint32_t a = i < len ? (uint32_t)(w >> k8) & 0xFFu : kNone;  // (behind the end: no code)
        if (i < len && (!Inverse || plain(a))) {
            const uint64_t rest = S - em_mix_word(w, j);
            for (uint32_t q = 0; q < nc; q++) {
                const uint32_t c = Inverse ? codes[q] : 1u << q;
                if (c == a) continue;
                f(rest + em_mix_word((w & ~(0xFFull << k8)) | (uint64_t)c << k8, j), len, (uint32_t)kSub, i, c);
            }
            const uint64_t t = shifted_word(X, nw, j);
            if (len >= 2u && !(i + 1u < len && ((uint32_t)(t >> k8) & 0xFFu) == a)) {  // the last code of a run of equal codes
                const uint64_t w2 = (w & low) | (t & ~low);
                f(j >= nwd ? P[j] : P[j] + em_mix_word(w2, j) + (ST - PT[j + 1u]), len - 1u, (uint32_t)kDel, i, 0u);
            }
        }
        if (len + 1u <= RTX_OTU_MAX_LEN) {
            for (uint32_t q = 0; q < nc; q++) {
                const uint32_t c = Inverse ? codes[q] : 1u << q;
                if (c == a) continue;  // (behind x[i] it gives the same string)
                f(P[j] + em_mix_word((w & low) | (uint64_t)c << k8 | ((w & ~low) << 8), j) + (SU - PU[j + 1u]), len + 1u, (uint32_t)kIns, i, c);
            }
        }
    }
}

// bit q of the k = 4 of a hash in the filter
__device__ __forceinline__ uint64_t bloom_bit(const GraftParams &p, uint64_t h, uint32_t q) { return em_mix_word(h, q) & p.bloom_mask; }

// The rows of one kind (heavy: into the filter; light: tested against it), one wave each.
// (no thread leaves early: the block meets at the barrier between the sums and the enumeration)
template <bool Test>
__global__ __launch_bounds__(256) void graft_ball_kernel(GraftParams p) {
    extern __shared__ uint64_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * 4u + wv;
    const uint32_t len = x < p.n ? p.r_len[x] : 0u;
    const bool active = len != 0u && len <= RTX_OTU_MAX_LEN && (p.heavy[x] != 0u) == !Test;  // wave-uniform
    const uint32_t nw = (len + 7u) >> 3;
    const uint64_t *X = reinterpret_cast<const uint64_t *>(p.arena + (active ? p.r_off[x] : 0ull));
    uint64_t *P = lds + (size_t)wv * 3u * p.lds_words, *PT = P + p.lds_words, *PU = PT + p.lds_words;  // nw + 2 <= lds_words
    if (active) build_sums(X, len, nw, P, PT, PU, lane);
    __syncthreads();
    if (!active) return;
    uint32_t mine = 0;
    for_ball<false>(X, len, nw, P, PT, PU, lane, nullptr, 0u, [&](uint64_t sum, uint32_t vlen, uint32_t kind, uint32_t i, uint32_t c) {
        const uint64_t h = em_finish(sum, vlen) & p.hash_mask;
        if (!Test) {
            mine++;
#pragma unroll
            for (uint32_t q = 0; q < kBloomK; q++) {
                const uint64_t bit = bloom_bit(p, h, q);
                atomicOr(p.bloom + (bit >> 5), 1u << (bit & 31u));
            }
        } else {
            bool all = true;
#pragma unroll
            for (uint32_t q = 0; q < kBloomK; q++) {
                const uint64_t bit = bloom_bit(p, h, q);
                all = all && (p.bloom[bit >> 5] >> (bit & 31u) & 1u);
            }
            if (all) {
                const unsigned long long at = atomicAdd(p.counters + 1, 1ull);  // (counts on past the capacity: the host sees what the pass needs)
                if (at < p.cand_cap) p.cand[at] = make_uint2(x, kind | c << 2 | i << 16);
            }
        }
    });
    if (!Test) {
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0u) atomicAdd(p.counters + 0, (unsigned long long)mine);
    }
}

// One wave per candidate; blockDim.x / 64 waves per block, as many as the LDS of the longest row allows.
// (no thread leaves early: the block meets at two barriers)
__global__ __launch_bounds__(256) void graft_verify_kernel(GraftParams p, uint64_t n_cand) {
    extern __shared__ uint64_t lds[];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t e = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const bool active = e < n_cand;  // wave-uniform
    const uint2 cd = active ? p.cand[e] : make_uint2(0u, 0u);
    const uint32_t x = cd.x, kind = cd.y & 3u, c = cd.y >> 2 & 0xFFu, i = cd.y >> 16;
    const uint32_t len = active ? p.r_len[x] : 0u, nw = (len + 7u) >> 3;
    const uint32_t vlen = len + (kind == kIns ? 1u : 0u) - (kind == kDel ? 1u : 0u), nv = (vlen + 7u) >> 3;  // 1 .. RTX_OTU_MAX_LEN: the test kernel forms no other
    const uint64_t *X = reinterpret_cast<const uint64_t *>(p.arena + (active ? p.r_off[x] : 0ull));
    uint64_t *V = lds + (size_t)wv * 4u * p.lds_words, *P = V + p.lds_words, *PT = P + p.lds_words, *PU = PT + p.lds_words;  // nv + 2 <= lds_words
    if (active)
        for (uint32_t m = lane; m < nv; m += 64u) V[m] = variant_word(X, nw, kind, i, c, m);
    __syncthreads();
    if (active) build_sums(V, vlen, nv, P, PT, PU, lane);
    __syncthreads();
    if (!active) return;
    const uint32_t mask = (uint32_t)((1ull << p.tbits) - 1ull);
    bool found = false;
    for_ball<true>(V, vlen, nv, P, PT, PU, lane, p.codes, p.n_codes, [&](uint64_t sum, uint32_t ylen, uint32_t k2, uint32_t i2, uint32_t c2) {
        const uint64_t h = em_finish(sum, ylen) & p.hash_mask;
        const uint32_t tag = em_tag(h), nwy = (ylen + 7u) >> 3, j2 = i2 >> 3;
        uint32_t slot = em_slot(h, p.tbits);
        for (uint64_t probe = 0; probe <= mask; probe++) {  // read-only; bounded by the table
            const unsigned long long s = p.table[slot];
            if (s == 0ull) break;
            if ((uint32_t)s == tag) {
                const uint32_t y = (uint32_t)(s >> 32) - 1u;
                if (y < p.n && p.r_len[y] == ylen) {
                    const uint64_t *Y = reinterpret_cast<const uint64_t *>(p.arena + p.r_off[y]);
                    bool same = j2 >= nwy || Y[j2] == variant_word(V, nv, k2, i2, c2, j2);  // the edited word first
                    for (uint32_t m = 0; same && m < nwy; m++) same = Y[m] == variant_word(V, nv, k2, i2, c2, m);
                    if (same) {  // (the rows are distinct: no other row holds these bytes)
                        if (p.heavy[y]) { atomicMin(p.parent + x, y); found = true; }
                        break;
                    }
                }
            }
            slot = (slot + 1u) & mask;
        }
    });
    if (__ballot(found) != 0ull && lane == 0u) atomicAdd(p.counters + 2, 1ull);
}

__global__ __launch_bounds__(256) void graft_key_kernel(GraftParams p) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= p.n || p.heavy[x]) return;
    const uint32_t par = p.parent[x];
    if (par != kNone) atomicMin(p.key + p.otu[x], (unsigned long long)par << 32 | x);
}

// (no thread leaves early in the three kernels of the scan: the block scans as a whole)
__global__ __launch_bounds__(256) void graft_keep_count_kernel(GraftParams p) {
    __shared__ uint32_t lds[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    uint32_t tot;
    (void)block_scan_incl_u32(k < p.n_otus && p.key[k] == ~0ull ? 1u : 0u, lds, &tot);
    if (threadIdx.x == 0) p.block_sum[blockIdx.x] = tot;
}

// one block: the block sums become their exclusive scan, their total the number of OTUs left
__global__ __launch_bounds__(256) void graft_scan_blocks_kernel(GraftParams p, uint32_t n_blocks) {
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
    if (threadIdx.x == 0) *p.n_new = carry;
}

__global__ __launch_bounds__(256) void graft_keep_number_kernel(GraftParams p) {
    __shared__ uint32_t lds[4];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool keep = k < p.n_otus && p.key[k] == ~0ull;
    uint32_t tot;
    const uint32_t inc = block_scan_incl_u32(keep ? 1u : 0u, lds, &tot);
    if (keep) p.new_no[k] = p.block_sum[blockIdx.x] + inc - 1u;
}

// a grafted OTU takes the number of its target (heavy, hence numbered by the kernel before this one; only grafted entries are written)
__global__ __launch_bounds__(256) void graft_map_kernel(GraftParams p) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= p.n_otus) return;
    const unsigned long long key = p.key[k];
    if (key == ~0ull) return;
    const uint32_t par = (uint32_t)(key >> 32);
    if (par < p.n) p.new_no[k] = p.new_no[p.otu[par]];
}

__global__ __launch_bounds__(256) void graft_assign_kernel(GraftParams p) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= p.n) return;
    const uint32_t k = p.new_no[p.otu[r]];
    p.otu_new[r] = k;
    if (k < p.n_otus) atomicAdd(p.members + k, 1u);  // (new_no is preset to all ones: an OTU without a number shows on the host, and writes nowhere)
}

struct GraftStage : StageShell {
    DevBuf<uint8_t> d_arena, d_heavy, d_codes;
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_len, d_otu, d_bloom, d_parent, d_new_no, d_block_sum, d_otu_new, d_members, d_n_new;
    DevBuf<unsigned long long> d_table, d_counters, d_key;
    DevBuf<uint2> d_cand;
    PinBuf<uint8_t> h_arena, h_heavy;
    PinBuf<uint64_t> h_off;
    PinBuf<unsigned long long> h_table, h_counters;
    PinBuf<uint32_t> h_len, h_parent, h_new_no, h_otu_new, h_members, h_n_new;
};

int graft(GraftStage *st, const rtx_tally_view &v, const rtx_otu &in, const rtx_graft_params &prm, const std::vector<uint8_t> &heavy, std::vector<uint32_t> &parent, rtx_otu &o) {
    rtx_graft_info &g = *o.graft;
    const uint64_t n = v.n_entries, no = in.n_otus;
    hipStream_t s = st->stream;
    int rc;
    double t0 = now_s();
    // the rows as the arena of rtx_otu.hip, and what the enumeration will cost
    if ((rc = st->h_off.resize(n + 1)) || (rc = st->h_len.resize(n)) || (rc = st->h_heavy.resize(n))) return rc;
    uint64_t total = 0, strings = 0;
    uint32_t max_nw = 0;
    bool seen[256] = {};
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = v.base_off[r + 1] - v.base_off[r];
        st->h_off[r] = total;
        st->h_len[r] = (uint32_t)len;
        st->h_heavy[r] = heavy[r];
        total += (len + 7u) & ~7ull;
        if (len == 0 || len > RTX_OTU_MAX_LEN) continue;
        max_nw = std::max(max_nw, (uint32_t)((len + 7u) >> 3));
        if (!heavy[r]) continue;
        strings += 1 + 4 * len + len + 4 * (len + 1);  // an upper bound of |B1|: itself, substitutions, deletions, insertions
        for (uint64_t i = v.base_off[r]; i < v.base_off[r + 1]; i++) seen[v.bases[i]] = true;
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
    // the table of all rows, filled here: {tag, row + 1}, at most half full
    uint32_t tbits = 3;
    while ((1ull << tbits) < 2ull * n) tbits++;
    const size_t slots = (size_t)1 << tbits;
    const uint64_t hash_mask = rtxi::otu_hash_mask();
    if ((rc = st->h_table.resize(slots))) return rc;
    std::memset(st->h_table.data(), 0, slots * 8);
    for (uint64_t r = 0; r < n; r++) {
        const uint32_t len = st->h_len[r];
        if (len == 0u || v.base_off[r + 1] - v.base_off[r] > RTX_OTU_MAX_LEN) continue;
        const uint64_t *X = reinterpret_cast<const uint64_t *>(st->h_arena.data() + st->h_off[r]);
        uint64_t sum = 0;
        for (uint32_t j = 0; j < (len + 7u) >> 3; j++) sum += em_mix_word(X[j], j);
        const uint64_t h = em_finish(sum, len) & hash_mask;
        size_t slot = em_slot(h, tbits);
        while (st->h_table[slot]) slot = (slot + 1) & (slots - 1);
        st->h_table[slot] = (unsigned long long)em_tag(h) | (unsigned long long)(r + 1) << 32;
    }
    std::vector<uint8_t> codes = {1, 2, 4, 8};
    for (uint32_t b = 0; b < 256u; b++)
        if (seen[b] && b != 1u && b != 2u && b != 4u && b != 8u) codes.push_back((uint8_t)b);
    // the filter: 16 bits per string, a power of two, under the cap
    uint32_t bloom_log2 = prm.bloom_log2;
    if (!bloom_log2) {
        bloom_log2 = 5;
        while (bloom_log2 < 40u && (1ull << bloom_log2) < 16 * strings) bloom_log2++;
    }
    while (bloom_log2 > 5u && (1ull << bloom_log2) / 8 > prm.max_bloom_bytes) bloom_log2--;
    const size_t bloom_words = (size_t)1 << (bloom_log2 - 5u);
    g.bloom_log2 = bloom_log2;
    const uint32_t row_blocks = (uint32_t)((n + 255u) / 256u), otu_blocks = (uint32_t)((no + 255u) / 256u);
    uint64_t cand_cap = prm.initial_candidates ? prm.initial_candidates : std::max<uint64_t>(1024, 4 * g.light_rows);
    if ((rc = st->d_arena.alloc(total + 64)) || (rc = st->d_off.alloc(n + 1)) || (rc = st->d_len.alloc(n)) || (rc = st->d_heavy.alloc(n)) || (rc = st->d_otu.alloc(n)) ||
        (rc = st->d_table.alloc(slots)) || (rc = st->d_codes.alloc(codes.size())) || (rc = st->d_bloom.alloc(bloom_words)) || (rc = st->d_cand.alloc(cand_cap)) ||
        (rc = st->d_counters.alloc(3)) || (rc = st->d_parent.alloc(n)) || (rc = st->d_key.alloc(no)) || (rc = st->d_new_no.alloc(no)) || (rc = st->d_block_sum.alloc(otu_blocks)) ||
        (rc = st->d_otu_new.alloc(n)) || (rc = st->d_members.alloc(no)) || (rc = st->d_n_new.alloc(1)) || (rc = st->h_counters.resize(3)) || (rc = st->h_parent.resize(n)) ||
        (rc = st->h_new_no.resize(no)) || (rc = st->h_otu_new.resize(n)) || (rc = st->h_members.resize(no)) || (rc = st->h_n_new.resize(1)))
        return rc;
    RTX_HIP(hipMemcpyAsync(st->d_arena.p, st->h_arena.data(), total + 64, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_off.p, st->h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_len.p, st->h_len.data(), n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_heavy.p, st->h_heavy.data(), n, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_table.p, st->h_table.data(), slots * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_otu.p, in.otu.data(), n * 4, hipMemcpyHostToDevice, s));            // (pageable: the copy is staged before the call returns)
    RTX_HIP(hipMemcpyAsync(st->d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, s));  // (likewise)
    RTX_HIP(hipMemsetAsync(st->d_bloom.p, 0, bloom_words * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_counters.p, 0, 3 * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_parent.p, 0xFF, n * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_key.p, 0xFF, no * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_new_no.p, 0xFF, no * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_members.p, 0, no * 4, s));
    GraftParams p{};
    p.arena = st->d_arena.p;
    p.r_off = st->d_off.p;
    p.r_len = st->d_len.p;
    p.heavy = st->d_heavy.p;
    p.otu = st->d_otu.p;
    p.n = (uint32_t)n;
    p.n_otus = (uint32_t)no;
    p.table = st->d_table.p;
    p.tbits = tbits;
    p.hash_mask = hash_mask;
    p.lds_words = max_nw + 2u;
    p.bloom = st->d_bloom.p;
    p.bloom_mask = (1ull << bloom_log2) - 1ull;
    p.codes = st->d_codes.p;
    p.n_codes = (uint32_t)codes.size();
    p.cand = st->d_cand.p;
    p.cand_cap = cand_cap;
    p.counters = st->d_counters.p;
    p.parent = st->d_parent.p;
    p.key = st->d_key.p;
    p.new_no = st->d_new_no.p;
    p.block_sum = st->d_block_sum.p;
    p.otu_new = st->d_otu_new.p;
    p.members = st->d_members.p;
    p.n_new = st->d_n_new.p;
    RTX_HIP(hipStreamSynchronize(s));
    double t1 = now_s();
    g.seconds[0] = t1 - t0;

    const dim3 waves((unsigned)((n + 3u) / 4u));
    const size_t ball_lds = (size_t)4 * 3 * p.lds_words * sizeof(uint64_t);  // at most 4 x 3 x 514 x 8 = 49 344 bytes
    hipLaunchKernelGGL(graft_ball_kernel<false>, waves, dim3(256), ball_lds, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(s));
    double t2 = now_s();
    g.seconds[1] = t2 - t1;

    // the candidates: a pass, and once more when the buffer was too small for what it counted
    uint64_t n_cand = 0;
    for (g.test_passes = 0;;) {
        RTX_HIP(hipMemsetAsync(st->d_counters.p + 1, 0, 8, s));
        hipLaunchKernelGGL(graft_ball_kernel<true>, waves, dim3(256), ball_lds, s, p);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipMemcpyAsync(st->h_counters.data(), st->d_counters.p, 3 * 8, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipStreamSynchronize(s));
        g.test_passes++;
        n_cand = st->h_counters[1];
        if (n_cand <= cand_cap) break;
        if (g.test_passes >= 2u) { set_error("rtx_otu_graft: the second test pass counts %llu candidates, the first one counted %llu", (unsigned long long)n_cand, (unsigned long long)cand_cap); return RTX_ERR_HIP; }
        cand_cap = n_cand;  // (the count depends on the filter, not on the scheduling: the second pass fits)
        st->d_cand.release();
        if ((rc = st->d_cand.alloc(cand_cap))) return rc;
        p.cand = st->d_cand.p;
        p.cand_cap = cand_cap;
    }
    g.variants = st->h_counters[0];
    g.candidates = n_cand;
    double t3 = now_s();
    g.seconds[2] = t3 - t2;

    if (n_cand) {
        // four arrays per wave: four waves of the longest rows pass 64 KiB, so those run two to a block
        const uint32_t wpb = (size_t)4 * 4 * p.lds_words * sizeof(uint64_t) <= 65536u ? 4u : 2u;
        const size_t verify_lds = (size_t)wpb * 4 * p.lds_words * sizeof(uint64_t);  // at most 2 x 4 x 514 x 8 = 32 896 bytes
        hipLaunchKernelGGL(graft_verify_kernel, dim3((unsigned)((n_cand + wpb - 1u) / wpb)), dim3(64u * wpb), verify_lds, s, p, n_cand);
        RTX_HIP(hipGetLastError());
    }
    RTX_HIP(hipMemcpyAsync(st->h_counters.data(), st->d_counters.p, 3 * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    g.confirmed = st->h_counters[2];
    double t4 = now_s();
    g.seconds[3] = t4 - t3;

    hipLaunchKernelGGL(graft_key_kernel, dim3(row_blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(graft_keep_count_kernel, dim3(otu_blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(graft_scan_blocks_kernel, dim3(1), dim3(256), 0, s, p, otu_blocks);
    hipLaunchKernelGGL(graft_keep_number_kernel, dim3(otu_blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(graft_map_kernel, dim3(otu_blocks), dim3(256), 0, s, p);
    hipLaunchKernelGGL(graft_assign_kernel, dim3(row_blocks), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipMemcpyAsync(st->h_parent.data(), st->d_parent.p, n * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_new_no.data(), st->d_new_no.p, no * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_otu_new.data(), st->d_otu_new.p, n * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_members.data(), st->d_members.p, no * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_n_new.data(), st->d_n_new.p, 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    parent.assign(st->h_parent.data(), st->h_parent.data() + n);
    for (uint64_t x = 0; x < n; x++)
        if (parent[x] != kNone && (parent[x] >= n || !heavy[parent[x]] || heavy[x])) { set_error("rtx_otu_graft: row %llu has the parent %u", (unsigned long long)x, parent[x]); return RTX_ERR_HIP; }
    rtx::graft_build(in, v, heavy, parent, o);
    // the numbering, the map and the members the device made are those of the host's sums
    bool same = o.n_otus == st->h_n_new[0];
    for (uint64_t k = 0; same && k < no; k++) same = g.old_to_new[k] == st->h_new_no[k];
    for (uint64_t r = 0; same && r < n; r++) same = o.otu[r] == st->h_otu_new[r];
    for (uint64_t k = 0; same && k < o.n_otus; k++) same = o.members[k] == st->h_members[k];
    if (!same) { set_error("rtx_otu_graft: the numbering and the members the device made are not those of its parents"); return RTX_ERR_HIP; }
    g.seconds[4] = now_s() - t4;
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_otu_graft(int device, rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_graft_params prm{};
    if (const int rc = rtx::graft_open("rtx_otu_graft", table, otu, params, out, &v, &prm)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto *o = new rtx_otu();
    o->graft.reset(new rtx_graft_info());
    std::vector<uint8_t> heavy;
    rtx::graft_heavy(*otu, prm.boundary, heavy, *o->graft);
    std::vector<uint32_t> parent(v.n_entries, kNone);
    int rc = RTX_OK;
    if (o->graft->heavy_rows == 0 || o->graft->light_rows == 0) {
        rtx::graft_build(*otu, v, heavy, parent, *o);  // (nothing to graft, or nothing to graft onto: nothing to upload)
    } else {
        auto *st = new GraftStage();
        rc = st->open(device);
        if (!rc) rc = graft(st, v, *otu, prm, heavy, parent, *o);
        destroy(st);
    }
    if (rc) { delete o; return rc; }
    *out = o;
    return RTX_OK;
}

// Denoising on the device (rtx_otu_unoise; raxtax_hip.h, "Denoising (UNOISE)"): the distinct reads of a run into ZOTUs by the UNOISE rule.
//   tiers    the host cuts the table into tiers [s0, s1), s1 the first row with (w[s0] >> (alpha + 1)) >= w[s1].  Inside a tier no row can
//            be another's parent (w[p] <= w[s0] < 2^(alpha + 1) w[e]), so the statuses of a tier depend on earlier tiers only: one pass
//            per tier, no edge list, no fixed point.
//   rows     4-bit codes, sixteen to a 64-bit word, row after row (r_off in words); length, weight and lim per row.
//   centroids  the live parents (ZOTUs) in rank order: c_rank / c_w / c_len per slot, and their words interleaved by 64 slots --
//            word t of slot s lies at ((s / 64) W + t) 64 + s % 64, W the most words of any row -- so that the 64 lanes of a wave, one
//            centroid each, load word t of their centroids as one run of 512 bytes.
//   1 pair   one wave per (row of the tier, group of centroid tiles).  The row is the pattern: its sixteen bit rows (one per code, rtx_math.hpp
//            "Denoising") are built once per wave into LDS from ballots, 64 positions at a time.  Then tile after tile of 64 centroids, one
//            per lane as the text: k from the two weights; a pair whose lengths differ by more than k is dropped and counted (d >= the
//            difference of the lengths); the others run unoise_distance, which gives the exact d when d <= k and leaves the loop at the
//            first column that proves d > k -- the wave leaves a tile when its last lane has.  The list is in rank order, so the tiles of
//            a row end at the first slot at or above lim(row).  (d << 32 | rank) is folded over the lanes and into best[row] with a 64-bit
//            atomicMin: the minimum does not depend on the order.
//   2 decide one thread per row of the tier: long, absorbed (best is set), a ZOTU (w >= minsize) or left.
//   3 append one block scans the tier's ZOTU flags in rank order and appends them to the list; 4 scatter copies their words into the
//            interleaved layout.  The host reads the length of the list back: the next tier's launches are sized from it.
#include <atomic>

#include "host_unoise.hpp"
#include "rtx_otu_dev.hpp"
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"

using namespace rtxi;

namespace {

std::atomic<uint64_t> g_unoise_slice{~0ull};  // RTX_DEFAULT_UNOISE_SLICE (tests: a small table in many launches)

constexpr uint64_t kPairBudget = 1ull << 32;      // (row, centroid) pairs of one launch at the most
constexpr uint64_t kCentroidBudget = 1ull << 22;  // centroids of one launch at the most
constexpr uint64_t kArenaBudget = 1ull << 34;     // bytes of the interleaved centroid words: beyond, RTX_ERR_OOM before anything is allocated

struct UnoiseParams {
    const uint64_t *words;   // the rows' packed codes
    const uint64_t *r_off;   // [n] in words
    const uint32_t *r_len;   // [n] (above RTX_OTU_MAX_LEN: a long row, no words)
    const uint64_t *r_w;     // [n]
    const uint32_t *lim;     // [n]
    uint32_t n;
    uint32_t alpha, max_diffs;
    uint64_t minsize;
    uint32_t W;              // words per centroid in the interleaved layout
    uint32_t peq_stride;     // 64-bit words per bit row in LDS (odd)
    uint32_t *c_rank;        // [c_cap]
    uint64_t *c_w;           // [c_cap]
    uint32_t *c_len;         // [c_cap]
    uint64_t *c_words;       // [c_cap / 64 x W x 64]
    uint32_t c_cap;          // a multiple of 64
    uint32_t *n_cent;        // [1]
    unsigned long long *best;      // [n] (d << 32 | rank), all ones: none
    uint8_t *status;         // [n]
    uint32_t *slot_of;       // [n] the slot of a row that became a centroid
    unsigned long long *counters;  // pairs, dropped by the length test, reached the last column
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// rows [row_begin, row_begin + gridDim.x) against the slots [slot_begin, slot_end) of the list; gridDim.y groups share a row's tiles
__global__ __launch_bounds__(64) void unoise_pair_kernel(UnoiseParams p, uint32_t row_begin, uint32_t slot_begin, uint32_t slot_end) {
    extern __shared__ uint64_t peq[];  // [16][peq_stride]
    const uint32_t lane = threadIdx.x;
    const uint32_t e = row_begin + blockIdx.x;
    const uint32_t m = p.r_len[e];
    const uint32_t lim = p.lim[e];
    if (m > RTX_OTU_MAX_LEN || slot_begin + blockIdx.y * 64u >= slot_end || p.c_rank[slot_begin + blockIdx.y * 64u] >= lim) return;  // (wave-uniform)
    const uint64_t we = p.r_w[e];
    const uint64_t *X = p.words + p.r_off[e];
    const uint32_t stride = p.peq_stride, nwq = unoise_peq_words(m);
    uint32_t *peq32 = reinterpret_cast<uint32_t *>(peq);
    // the bit rows: bit i + 32 of row c <- (x[i] == c).  64 positions are one ballot per code; lane c keeps the ballot of code c
    for (uint32_t c = 0; c < 16u; c++)
        for (uint32_t w = lane; w < nwq; w += 64u) peq[c * stride + w] = 0ull;
    __syncthreads();
    for (uint32_t base = 0; base < m; base += 64u) {  // wave-uniform
        const uint32_t i = base + lane;
        const uint32_t code = i < m ? (uint32_t)(X[i >> 4] >> (4u * (i & 15u))) & 15u : 16u;
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t c = 0; c < 16u; c++) {
            const uint64_t b = __ballot(code == c);
            mine = lane == c ? b : mine;
        }
        if (lane < 16u) {  // bits base + 32 .. base + 95: the high half of word base / 64 and the low half of the next
            const uint32_t at = lane * stride * 2u + (base >> 5) + 1u;
            peq32[at] = (uint32_t)mine;
            peq32[at + 1u] = (uint32_t)(mine >> 32);
        }
    }
    __syncthreads();

    unsigned long long best = ~0ull;
    uint32_t n_pairs = 0, n_length = 0, n_finished = 0;
    for (uint32_t base = slot_begin + blockIdx.y * 64u; base < slot_end; base += gridDim.y * 64u) {  // wave-uniform
        if (p.c_rank[base] >= lim) break;  // (the list is in rank order: so is every later tile)
        const uint32_t slot = base + lane;
        uint32_t rank = 0xFFFFFFFFu, n = 0, k = 0;
        if (slot < slot_end) {
            rank = p.c_rank[slot];
            if (rank < lim) {
                n = p.c_len[slot];
                k = unoise_allowed(p.c_w[slot], we, p.alpha, p.max_diffs);
            }
        }
        const bool pair = rank < lim;
        const bool run = k > 0u && (m > n ? m - n : n - m) <= k;
        n_pairs += (uint32_t)__popcll(__ballot(pair));
        n_length += (uint32_t)__popcll(__ballot(pair && !run));
        bool finished = false;
        if (run) {
            const uint64_t *T = p.c_words + ((size_t)(slot >> 6) * p.W) * 64u + (slot & 63u);
            const uint32_t d = unoise_distance(
                m, n, k, [&](uint32_t c, uint32_t j) { return unoise_eq(peq + c * stride, j); }, [&](uint32_t t) { return T[(size_t)t * 64u]; }, finished);
            if (d != kUnoiseNoDist) {
                const unsigned long long key = (unsigned long long)d << 32 | rank;
                best = key < best ? key : best;
            }
        }
        n_finished += (uint32_t)__popcll(__ballot(finished));
    }
    best = wave_min_u64(best);
    if (lane == 0u) {
        if (best != ~0ull) atomicMin(p.best + e, best);
        atomicAdd(p.counters + 0, (unsigned long long)n_pairs);
        atomicAdd(p.counters + 1, (unsigned long long)n_length);
        atomicAdd(p.counters + 2, (unsigned long long)n_finished);
    }
}

__global__ __launch_bounds__(256) void unoise_decide_kernel(UnoiseParams p, uint32_t s0, uint32_t s1) {
    const uint32_t r = s0 + blockIdx.x * 256u + threadIdx.x;
    if (r >= s1) return;
    uint8_t st;
    if (p.r_len[r] > RTX_OTU_MAX_LEN) st = RTX_UNOISE_LONG;
    else if (p.best[r] != ~0ull) st = RTX_UNOISE_ABSORBED;
    else st = p.r_w[r] >= p.minsize ? RTX_UNOISE_ZOTU : RTX_UNOISE_LEFT;
    p.status[r] = st;
}

// one block: the ZOTUs of [s0, s1) behind the list, in rank order
__global__ __launch_bounds__(256) void unoise_append_kernel(UnoiseParams p, uint32_t s0, uint32_t s1) {
    __shared__ uint32_t lds[4];
    uint32_t running = p.n_cent[0];
    for (uint32_t base = s0; base < s1; base += 256u) {  // block-uniform
        const uint32_t r = base + threadIdx.x;
        const bool take = r < s1 && p.status[r] == RTX_UNOISE_ZOTU;
        uint32_t tot;
        const uint32_t inc = block_scan_incl_u32(take ? 1u : 0u, lds, &tot);
        const uint32_t slot = running + inc - 1u;
        if (take && slot < p.c_cap) {  // (the capacity is the count of rows that can become a ZOTU at all)
            p.c_rank[slot] = r;
            p.c_w[slot] = p.r_w[r];
            p.c_len[slot] = p.r_len[r];
            p.slot_of[r] = slot;
        }
        running += tot;
    }
    if (threadIdx.x == 0u) p.n_cent[0] = running < p.c_cap ? running : p.c_cap;
}

// one wave per row of [s0, s1): the words of a new centroid into the interleaved layout
__global__ __launch_bounds__(256) void unoise_scatter_kernel(UnoiseParams p, uint32_t s0, uint32_t s1) {
    const uint32_t r = s0 + blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= s1 || p.status[r] != RTX_UNOISE_ZOTU) return;
    const uint32_t slot = p.slot_of[r];
    if (slot >= p.c_cap) return;
    const uint32_t nw = (p.r_len[r] + 15u) >> 4;  // (<= W)
    const uint64_t *X = p.words + p.r_off[r];
    uint64_t *T = p.c_words + ((size_t)(slot >> 6) * p.W) * 64u + (slot & 63u);
    for (uint32_t t = lane; t < nw; t += 64u) T[(size_t)t * 64u] = X[t];
}

struct UnoiseStage : StageShell {
    DevBuf<uint64_t> d_words, d_off, d_w, d_c_w, d_c_words;
    DevBuf<uint32_t> d_len, d_lim, d_c_rank, d_c_len, d_n_cent, d_slot_of;
    DevBuf<unsigned long long> d_best, d_counters;
    DevBuf<uint8_t> d_status;
    PinBuf<uint64_t> h_words, h_off;
    PinBuf<uint32_t> h_len, h_n_cent;
    PinBuf<unsigned long long> h_best, h_counters;
    PinBuf<uint8_t> h_status;
};

int unoise(UnoiseStage *st, const rtx_tally_view &v, rtx_otu &o) {
    rtx_unoise_info &u = *o.unoise;
    const rtx_unoise_params &prm = u.params;
    const uint64_t n = v.n_entries;
    hipStream_t s = st->stream;
    int rc;
    double t0 = now_s();
    // the rows as packed words; what can become a centroid at all
    if ((rc = st->h_off.resize(n + 1)) || (rc = st->h_len.resize(n))) return rc;
    uint64_t total = 0, eligible = 0;
    uint32_t max_len = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = v.base_off[r + 1] - v.base_off[r];
        st->h_off[r] = total;
        st->h_len[r] = (uint32_t)std::min<uint64_t>(len, 0xFFFFFFFFull);
        if (len > RTX_OTU_MAX_LEN) continue;
        total += (len + 15u) >> 4;
        max_len = std::max(max_len, (uint32_t)len);
        if (v.sizes[r] >= prm.minsize) eligible++;
    }
    st->h_off[n] = total;
    for (uint64_t i = 0; i < v.base_off[n]; i++)
        if (v.bases[i] > 15u) { set_error("rtx_otu_unoise: byte %u in the table (the device path takes 4-bit codes)", v.bases[i]); return RTX_ERR_INVALID; }
    if ((rc = st->h_words.resize(total + 1))) return rc;
    {
        uint64_t *words = st->h_words.data();
        const uint64_t *off = st->h_off.data();
        parallel_ranges(n, rtx::host_threads(4u), 4096, [=](unsigned, uint64_t a, uint64_t b) {
            for (uint64_t r = a; r < b; r++) {
                const uint64_t len = v.base_off[r + 1] - v.base_off[r];
                if (len <= RTX_OTU_MAX_LEN) unoise_pack(v.bases + v.base_off[r], (uint32_t)len, words + off[r]);
            }
        });
        words[total] = 0;
    }
    const uint32_t W = std::max(1u, (max_len + 15u) >> 4);
    const uint64_t c_cap = (eligible + 63u) & ~63ull;
    if (c_cap * W * 8u > kArenaBudget) {
        set_error("rtx_otu_unoise: %llu possible centroids of up to %u codes need %llu bytes (at most %llu)", (unsigned long long)eligible, max_len,
                  (unsigned long long)(c_cap * W * 8u), (unsigned long long)kArenaBudget);
        return RTX_ERR_OOM;
    }
    const uint32_t peq_stride = unoise_peq_words(max_len) | 1u;  // (odd: the sixteen rows start in different banks)
    const size_t lds = (size_t)16 * peq_stride * 8u;            // at most 16 x 67 x 8 = 8 576 bytes
    std::vector<uint64_t> tier;
    rtx::unoise_tiers(v, prm.alpha, tier);
    if ((rc = st->d_words.alloc(total + 1)) || (rc = st->d_off.alloc(n + 1)) || (rc = st->d_len.alloc(n)) || (rc = st->d_w.alloc(n)) || (rc = st->d_lim.alloc(n)) ||
        (rc = st->d_c_rank.alloc(c_cap)) || (rc = st->d_c_w.alloc(c_cap)) || (rc = st->d_c_len.alloc(c_cap)) || (rc = st->d_c_words.alloc(c_cap * W)) ||
        (rc = st->d_n_cent.alloc(1)) || (rc = st->d_slot_of.alloc(n)) || (rc = st->d_best.alloc(n)) || (rc = st->d_counters.alloc(3)) || (rc = st->d_status.alloc(n)) ||
        (rc = st->h_n_cent.resize(1)) || (rc = st->h_best.resize(n)) || (rc = st->h_counters.resize(3)) || (rc = st->h_status.resize(n)))
        return rc;
    RTX_HIP(hipMemcpyAsync(st->d_words.p, st->h_words.data(), (total + 1) * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_off.p, st->h_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_len.p, st->h_len.data(), n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_w.p, v.sizes, n * 8, hipMemcpyHostToDevice, s));            // (pageable: the copy is staged before the call returns)
    RTX_HIP(hipMemcpyAsync(st->d_lim.p, u.lim.data(), n * 4, hipMemcpyHostToDevice, s));    // (likewise)
    RTX_HIP(hipMemsetAsync(st->d_c_rank.p, 0xFF, c_cap * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_c_words.p, 0, c_cap * W * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_n_cent.p, 0, 4, s));
    RTX_HIP(hipMemsetAsync(st->d_slot_of.p, 0xFF, n * 4, s));
    RTX_HIP(hipMemsetAsync(st->d_best.p, 0xFF, n * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_counters.p, 0, 3 * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_status.p, RTX_UNOISE_LEFT, n, s));
    UnoiseParams p{};
    p.words = st->d_words.p;
    p.r_off = st->d_off.p;
    p.r_len = st->d_len.p;
    p.r_w = st->d_w.p;
    p.lim = st->d_lim.p;
    p.n = (uint32_t)n;
    p.alpha = prm.alpha;
    p.max_diffs = prm.max_diffs;
    p.minsize = prm.minsize;
    p.W = W;
    p.peq_stride = peq_stride;
    p.c_rank = st->d_c_rank.p;
    p.c_w = st->d_c_w.p;
    p.c_len = st->d_c_len.p;
    p.c_words = st->d_c_words.p;
    p.c_cap = (uint32_t)c_cap;
    p.n_cent = st->d_n_cent.p;
    p.best = st->d_best.p;
    p.status = st->d_status.p;
    p.slot_of = st->d_slot_of.p;
    p.counters = st->d_counters.p;
    RTX_HIP(hipStreamSynchronize(s));
    double t1 = now_s();
    u.seconds[0] = t1 - t0;

    const uint64_t cap = g_unoise_slice.load();
    double pair_s = 0;
    uint32_t n_cent = 0;
    u.tiers = (uint32_t)(tier.size() - 1);
    for (size_t t = 0; t + 1 < tier.size(); t++) {
        const uint32_t s0 = (uint32_t)tier[t], s1 = (uint32_t)tier[t + 1];
        // (lim never falls along the table: if the tier's last row has no candidate, none of its rows has; a row with lim 0 leaves the kernel at once)
        const bool pairs = n_cent > 0u && u.lim[s1 - 1u] > 0u;
        if (pairs) {
            RTX_HIP(hipEventRecord(st->ev0, s));
            const uint64_t c_slice = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)n_cent, kCentroidBudget, cap}));
            const uint64_t r_slice = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)(s1 - s0), std::max<uint64_t>(64, kPairBudget / c_slice), cap}));
            for (uint64_t c0 = 0; c0 < n_cent; c0 += c_slice) {
                const uint32_t c1 = (uint32_t)std::min<uint64_t>(n_cent, c0 + c_slice);
                const uint32_t tiles = (c1 - (uint32_t)c0 + 63u) / 64u;
                for (uint64_t r0 = s0; r0 < s1; r0 += r_slice) {
                    const uint32_t rows = (uint32_t)std::min<uint64_t>(s1 - r0, r_slice);
                    // enough waves to fill the device when the rows are few, one wave per row over all its tiles when they are many
                    const uint32_t groups = std::max(1u, std::min({tiles, 65535u, (16384u + rows - 1u) / rows}));
                    hipLaunchKernelGGL(unoise_pair_kernel, dim3(rows, groups), dim3(64), lds, s, p, (uint32_t)r0, (uint32_t)c0, c1);
                    u.launches++;
                }
            }
            RTX_HIP(hipGetLastError());
            RTX_HIP(hipEventRecord(st->ev1, s));
        }
        hipLaunchKernelGGL(unoise_decide_kernel, dim3((s1 - s0 + 255u) / 256u), dim3(256), 0, s, p, s0, s1);
        hipLaunchKernelGGL(unoise_append_kernel, dim3(1), dim3(256), 0, s, p, s0, s1);
        hipLaunchKernelGGL(unoise_scatter_kernel, dim3((s1 - s0 + 3u) / 4u), dim3(256), 0, s, p, s0, s1);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipMemcpyAsync(st->h_n_cent.data(), st->d_n_cent.p, 4, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipStreamSynchronize(s));
        if (pairs) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, st->ev0, st->ev1);
            pair_s += (double)ms * 1e-3;
        }
        if (st->h_n_cent[0] < n_cent || st->h_n_cent[0] > c_cap) { set_error("rtx_otu_unoise: the centroid list went from %u to %u of %llu", n_cent, st->h_n_cent[0], (unsigned long long)c_cap); return RTX_ERR_HIP; }
        n_cent = st->h_n_cent[0];
    }
    double t2 = now_s();
    u.seconds[1] = pair_s;
    u.seconds[2] = std::max(0.0, t2 - t1 - pair_s);

    RTX_HIP(hipMemcpyAsync(st->h_status.data(), st->d_status.p, n, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_best.data(), st->d_best.p, n * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_counters.data(), st->d_counters.p, 3 * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    u.pairs = st->h_counters[0];
    u.pairs_length = st->h_counters[1];
    u.pairs_finished = st->h_counters[2];
    u.status.assign(st->h_status.data(), st->h_status.data() + n);
    u.parent.assign(n, RTX_NO_REF);
    u.dist.assign(n, RTX_NO_DIST);
    for (uint64_t r = 0; r < n; r++) {
        if (u.status[r] != RTX_UNOISE_ABSORBED) continue;
        u.parent[r] = (uint32_t)st->h_best[r];
        u.dist[r] = (uint32_t)(st->h_best[r] >> 32);
    }
    if ((rc = rtx::unoise_build("rtx_otu_unoise", o, v))) return rc;
    if (u.n_status[RTX_UNOISE_ZOTU] != n_cent) { set_error("rtx_otu_unoise: %llu ZOTUs, %u centroids in the list", (unsigned long long)u.n_status[RTX_UNOISE_ZOTU], n_cent); return RTX_ERR_HIP; }
    u.seconds[3] = now_s() - t2;
    return RTX_OK;
}

}  // namespace

namespace rtxi {
void set_unoise_slice(uint64_t cap) { g_unoise_slice.store(cap); }
}  // namespace rtxi

extern "C" int rtx_otu_unoise(int device, rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out) {
    rtx_tally_view v{};
    rtx_unoise_params prm{};
    if (const int rc = rtx::unoise_open("rtx_otu_unoise", table, params, out, &v, &prm)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto *o = new rtx_otu();
    o->unoise.reset(new rtx_unoise_info());
    o->unoise->params = prm;
    rtx::unoise_lim(v, prm.alpha, o->unoise->lim);
    int rc = RTX_OK;
    if (v.n_entries == 0) {
        rc = rtx::unoise_build("rtx_otu_unoise", *o, v);  // (nothing to upload)
    } else {
        auto *st = new UnoiseStage();
        rc = st->open(device);
        if (!rc) rc = unoise(st, v, *o);
        destroy(st);
    }
    if (rc) { delete o; return rc; }
    *out = o;
    return RTX_OK;
}

// De novo chimera check of a run on the device (rtx_denovo_check; raxtax_hip.h, "de novo chimera check of a run"): every entry of a run --
// a row of an rtx_tally_table or the seed of an OTU -- against the more abundant entries of the same run that are not flagged themselves.
// The counting is rtx_chimera.hip's; what is new is where the references come from.  Entries are sorted by weight, so the parents of entry
// e are a PREFIX of the entry list (below lim(e), host_denovo.cpp) under a live mask: the stage builds a bitmap of its own over the
// entries below the largest lim, in the index's layout, and masks the planes at every checkpoint.
//   bitmap   [tile of 8192 entries][row][256 words]: rows 0 .. 65535 are the 8-mers themselves, row 65536 is all zero, row 65537 holds the
//            live mask (the bit of entry p set while p is not flagged).  The stride is a multiple of 16 bytes: the last tile may span
//            fewer than 64 lanes (tile_lanes).
//   denovo_bitmap_kernel  one wave per parent entry: every valid window's 8-mer sets the entry's bit (ref_slot + bitmap_word) with a 32-bit
//            atomicOr on a cleared bitmap; lane 0 sets the live bit.  OR commutes: the bitmap does not depend on the scheduling.
//   denovo_rows_kernel    chimera_rows_kernel with k << 10 in place of row_of[k] << 10.
//   denovo_scan_kernel    chimera_scan_kernel, one wave per (entry, tile, direction) for the tiles below ceil(lim(e) / 8192) only -- the
//            work is triangular, tile-major -- with the planes ANDed at a checkpoint with allow[w]: the lane's 16 bytes of the live row
//            (one load at wave start) AND the prefix mask of lim(e) (denovo_allow, rtx_math.hpp).
//   denovo_reduce_kernel  chimera_reduce_kernel over the tiles the entry scanned, and RTX_DENOVO_NO_PARENT.
//   denovo_update_kernel  one thread per entry of the round: a flag that differs from the one the round started with is taken over, the
//            live bit rewritten (atomicAnd / atomicOr), the lowest such entry kept (atomicMin).
// Rounds on the host: round 1 scans every entry with all parents live; the next round scans the entries e with lim(e) > the lowest entry
// whose flag changed -- a suffix of the list, as lim never decreases -- and a round that changes nothing ends it: the flags then solve the
// recursion of the definition, which has one solution.  Vector stores and ordinary vector atomics.
#include "host_denovo.hpp"
#include "rtx_stage.hpp"
#include "rtx_hit_common.hpp"

namespace {

struct DenovoParams {
    const uint8_t *bases;          // the entries' sequences, one byte per code
    const uint64_t *base_off;      // [n + 1]
    const uint32_t *lim;           // [n]
    uint32_t *bitmap;
    uint32_t n, n_par, ntiles, stride_bytes;
    uint32_t S, mindelta;
    uint32_t q0;                   // entry q of the slice is entry q0 + q
    uint32_t list_stride;
    uint32_t *lists;               // [slice][2][list_stride]
    uint32_t *n_valid;             // [slice]
    uint16_t *cpg;                 // [slice][2][S]
    uint2 *best;                   // [slice][2][S][ntiles]
    const uint32_t *ids;           // the entries of the slice (relative to q0) that a scan launch takes: one plane class, ascending
    uint32_t *out;                 // [n][12] rtx_chimera_rec
    uint32_t *flags;               // [n] the flags the round started with
    uint32_t *changed;             // [1] the lowest entry whose flag changed
};

// The waves of a scan launch, tile-major: tile t is scanned by the entries ids[first[t] ..) of the class -- a suffix, as lim never decreases --
// and its waves begin at item[t]; item[ntiles] waves per direction.
struct ScanGrid {
    uint32_t ntiles, n_ids;
    uint32_t first[kDenovoMaxTiles], item[kDenovoMaxTiles + 1];
};

__device__ __forceinline__ uint32_t entry_len(const DenovoParams &p, uint32_t e, uint64_t &b0) {
    b0 = p.base_off[e];
    const uint64_t len = p.base_off[e + 1] - b0;
    return len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
}

__global__ __launch_bounds__(256) void denovo_bitmap_kernel(DenovoParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (e >= p.n_par) return;  // (wave-uniform)
    uint64_t b0;
    const uint32_t len = entry_len(p, e, b0);
    const uint8_t *seq = p.bases + b0;
    uint32_t word, bit;
    ref_slot(e, p.stride_bytes, word, bit);
    if (lane == 0u) atomicOr(p.bitmap + bitmap_word(kDenovoLiveRow, word, kDenovoRows1), 1u << bit);
    for (uint32_t i = lane; i + 8u <= len; i += 64u) {  // a parent of any length: an entry above RTX_CHIMERA_MAX_QUERY is one too
        uint32_t k;
        if (chimera_window_kmer(seq, i, k)) atomicOr(p.bitmap + bitmap_word(k, word, kDenovoRows1), 1u << bit);
    }
}

__global__ __launch_bounds__(64) void denovo_rows_kernel(DenovoParams p) {
    __shared__ uint32_t off[2][kChimMaxSegments + 1];
    const uint32_t q = blockIdx.x, lane = threadIdx.x, S = p.S;
    uint64_t b0;
    const uint32_t len = entry_len(p, p.q0 + q, b0);
    const uint32_t n_pos = chimera_n_pos(len);
    if (lane < 2u) chimera_layout(n_pos, S, lane, off[lane]);
    __syncthreads();
    if (lane < 2u * S) p.cpg[(size_t)q * 2u * S + lane] = (uint16_t)(off[lane / S][lane % S + 1u] >> 3);
    const uint32_t cap = chimera_list_cap(off[0][S]);  // (<= list_stride: the host sized it for the longest entry that is checked)
    const uint32_t zero = kDenovoZeroRow << 10;
    const uint8_t *seq = p.bases + b0;
    uint32_t nv = 0;
    for (uint32_t dir = 0; dir < 2u; dir++) {
        uint32_t *list = p.lists + ((size_t)q * 2u + dir) * p.list_stride;
        for (uint32_t j = lane; j < cap; j += 64u) {
            const uint32_t i = chimera_list_window(n_pos, S, dir, off[dir], j);
            uint32_t v = zero, k;
            if (i != kChimNoRef && chimera_window_kmer(seq, i, k)) {
                nv += dir == 0u ? 1u : 0u;
                v = k << 10;
            }
            list[j] = v;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nv += __shfl_xor(nv, d, 64);
    if (lane == 0u) p.n_valid[q] = nv;
}

template <int NP>
__global__ __launch_bounds__(256) void denovo_scan_kernel(DenovoParams p, ScanGrid g) {
    const uint32_t lane = threadIdx.x & 63u, S = p.S;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (uint64_t)g.item[g.ntiles] * 2u) return;  // (wave-uniform)
    const uint32_t dir = (uint32_t)(item & 1u), w = (uint32_t)(item >> 1);
    uint32_t tile = 0;
    while (tile + 1u < g.ntiles && w >= g.item[tile + 1u]) tile++;  // (wave-uniform; at most 31 steps)
    const uint32_t at = g.first[tile] + (w - g.item[tile]);
    if (at >= g.n_ids) return;  // (never: the host built the grid from the same list)
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.ids[at]);
    const uint32_t lim = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.lim[p.q0 + q]);
    const uint32_t *list = p.lists + ((size_t)q * 2u + dir) * p.list_stride;
    const uint16_t *cpg = p.cpg + ((size_t)q * 2u + dir) * S;
    const uint32_t G = (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[S - 1u]);  // fold groups of the list
    if (G == 0u) return;  // no window: denovo_reduce_kernel reads nothing of such an entry
    uint2 *best = p.best + ((size_t)q * 2u + dir) * S * p.ntiles + tile;  // checkpoint k: best[k * ntiles]
    const __amdgpu_buffer_rsrc_t rsrc = tile_rsrc(p.bitmap, kDenovoRows1, tile);
    const uint32_t voff = lane * 16u, L = tile_lanes(p.stride_bytes, tile);
    uint32_t allow[4];
    {
        denovo_allow(lane, L, tile, lim, allow);
        const u32x4_t live = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, kDenovoLiveRow << 10, 0);
        allow[0] &= live.x;
        allow[1] &= live.y;
        allow[2] &= live.z;
        allow[3] &= live.w;
    }
    uint32_t pl[4][NP];
#pragma unroll
    for (int ww = 0; ww < 4; ww++)
#pragma unroll
        for (int b = 0; b < NP; b++) pl[ww][b] = 0u;
    uint32_t ncp = 0, next_cp = (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[0]);
    auto checkpoint = [&]() {
        uint32_t m, rl;
        denovo_lane_best<NP>(pl, allow, lane, L, m, rl);
        const uint32_t M = wave_max_u32(m);
        const uint32_t mine = M != 0u && m == M ? tile * 8192u + rl : kChimNoRef;
        const uint32_t R = ~wave_max_u32(~mine);  // the lowest one
        if (lane == 0u) best[(size_t)ncp * p.ntiles] = make_uint2(M, R);
        ncp++;
        next_cp = ncp < S ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[ncp]) : 0xFFFFFFFFu;
    };
    while (next_cp == 0u) checkpoint();  // empty segments in front (fewer windows than segments)
    // the fold loop of chimera_scan_kernel: two buffers of eight rows, the row offsets 64 at a time; the requests run past the list's end
    // into the zero row (kChimListTail)
    uint32_t idv = list[lane], idn = list[64u + lane];
    uint4 buf[2][8];
    load8v_at(buf[0], rsrc, voff, idv, 0);
    load8v_at(buf[1], rsrc, voff, idv, 8);
    for (uint32_t gi = 0; gi < G; gi += 2u) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const uint32_t gg = gi + (uint32_t)b;
            const uint4 c3 = tree8<NP>(pl, buf[b]);
            ripple4<NP, 3>(pl, c3);
            __builtin_amdgcn_sched_barrier(0);  // the requests below reuse the registers of the rows just folded: not hoisted above the fold
            const uint32_t tg = gg + 2u;
            if ((tg & 7u) == 0u) {  // (wave-uniform)
                idv = idn;
                idn = list[((tg >> 3) + 1u) * 64u + lane];
            }
            load8v_at(buf[b], rsrc, voff, idv, (int)((tg & 7u) * 8u));
            while (next_cp == gg + 1u) checkpoint();
        }
    }
}

// entries q0 + qa + blockIdx.x of the slice
__global__ __launch_bounds__(64) void denovo_reduce_kernel(DenovoParams p, uint32_t qa) {
    __shared__ uint32_t pm[kChimMaxSegments + 1], pr[kChimMaxSegments + 1], sm[kChimMaxSegments + 1], sr[kChimMaxSegments + 1];
    const uint32_t q = qa + blockIdx.x, e = p.q0 + q, lane = threadIdx.x, S = p.S;
    uint64_t b0;
    const uint32_t len = entry_len(p, e, b0), nv = p.n_valid[q], lim = p.lim[e];
    if (lane <= S) {
        pm[lane] = sm[lane] = 0u;
        pr[lane] = sr[lane] = kChimNoRef;
    }
    __syncthreads();
    if (nv != 0u && len <= kChimMaxQuery && lane < 2u * S) {  // (an entry with a valid window has a fold group: every checkpoint of every tile it scanned was stored)
        const uint32_t dir = lane / S, k = lane % S, nt = denovo_tiles(lim);
        const uint2 *b = p.best + ((size_t)q * 2u * S + lane) * p.ntiles;
        uint32_t bc = 0u, br = kChimNoRef;
        for (uint32_t t = 0; t < nt; t++) {
            const uint2 v = b[t];
            chimera_take(bc, br, v.x, v.y);
        }
        if (dir == 0u) { pm[k + 1u] = bc; pr[k + 1u] = br; }
        else { sm[S - 1u - k] = bc; sr[S - 1u - k] = br; }
    }
    __syncthreads();
    if (lane == 0u) {
        ChimRec r = chimera_record(len, nv, S, p.mindelta, pm, pr, sm, sr);
        if (r.status == kChimOk && lim == 0u) r = ChimRec{kDenovoNoParent, 0u, 0u, kChimNoRef, 0u, 0u, 0u, kChimNoRef, 0u, kChimNoRef, 0u, 0u};
        uint32_t *o = p.out + (size_t)e * 12u;
        reinterpret_cast<uint4 *>(o)[0] = make_uint4(r.status, r.n_valid, r.single, r.parent);
        reinterpret_cast<uint4 *>(o)[1] = make_uint4(r.seg, r.pos, r.left, r.parent_a);
        reinterpret_cast<uint4 *>(o)[2] = make_uint4(r.right, r.parent_b, r.delta, r.flag);
    }
}

// entries e0 + thread: the flags of the round against those it started with
__global__ __launch_bounds__(256) void denovo_update_kernel(DenovoParams p, uint32_t e0) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x + e0;
    if (i >= p.n) return;
    const uint32_t e = (uint32_t)i, now = p.out[(size_t)e * 12u + 11u];
    if (now == p.flags[e]) return;
    p.flags[e] = now;
    atomicMin(p.changed, e);
    if (e >= p.n_par) return;
    uint32_t word, bit;
    ref_slot(e, p.stride_bytes, word, bit);
    uint32_t *live = p.bitmap + bitmap_word(kDenovoLiveRow, word, kDenovoRows1);
    if (now) atomicAnd(live, ~(1u << bit));
    else atomicOr(live, 1u << bit);
}

constexpr uint64_t kBestBudget = 1ull << 30, kListBudget = 1ull << 29;  // bytes of a slice's checkpoint array / row lists (as rtx_chimera_run)

struct DenovoStage : StageShell {
    DevBuf<uint8_t> d_packed, d_bases;
    DevBuf<uint64_t> d_base_off;
    DevBuf<uint32_t> d_bitmap, d_lim, d_lists, d_n_valid, d_ids, d_out, d_flags, d_changed;
    DevBuf<uint16_t> d_cpg;
    DevBuf<uint2> d_best;
    PinBuf<uint8_t> h_packed;
    PinBuf<uint64_t> h_base_off;
    PinBuf<uint32_t> h_ids, h_out, h_changed;
};

int run(DenovoStage *st, const rtx_tally_view &v, rtx_denovo &d) {
    const uint64_t n = d.n_entries;
    const uint32_t S = d.params.segments;
    hipStream_t s = st->stream;
    int rc;
    const double t0 = now_s();
    // the entries' sequences back to back in entry order (with an OTU object: the seeds, gathered)
    std::vector<uint8_t> g_bases;
    std::vector<uint64_t> g_off;
    const uint8_t *bases = v.bases;
    const uint64_t *base_off = v.base_off;
    if (d.otu_mode) {
        g_off.resize(n + 1);
        g_off[0] = 0;
        for (uint64_t e = 0; e < n; e++) g_off[e + 1] = g_off[e] + (v.base_off[d.row[e] + 1u] - v.base_off[d.row[e]]);
        g_bases.resize(g_off[n] + 1);
        for (uint64_t e = 0; e < n; e++) std::memcpy(g_bases.data() + g_off[e], v.bases + v.base_off[d.row[e]], g_off[e + 1] - g_off[e]);
        bases = g_bases.data();
        base_off = g_off.data();
    }
    auto len_of = [&](uint64_t e) { return base_off[e + 1] - base_off[e]; };
    uint32_t max_pos = 0;
    for (uint64_t e = 0; e < n; e++) max_pos = std::max(max_pos, chimera_n_pos((uint32_t)std::min<uint64_t>(len_of(e), 0xFFFFFFFFull)));
    const uint64_t total = base_off[n] - base_off[0];
    const uint32_t n_par = d.lim[n - 1];  // (lim never decreases along the list)
    const uint32_t nt = denovo_tiles(n_par);
    if (nt > kDenovoMaxTiles) { set_error("rtx_denovo_check: %u parents", n_par); return RTX_ERR_INVALID; }
    const uint64_t bitmap_words = (uint64_t)nt * kDenovoRows1 * 256u;
    const uint32_t list_stride = chimera_list_cap(((max_pos + 7u) & ~7u) + 8u * S);
    const uint64_t best_per = 2ull * S * std::max(nt, 1u) * sizeof(uint2), list_per = 2ull * list_stride * 4u;
    const uint64_t slice = std::max<uint64_t>(1, std::min({n, kBestBudget / best_per, kListBudget / list_per, chimera_slice_cap()}));
    if ((rc = st->h_packed.resize(total + 64)) || (rc = st->h_base_off.resize(n + 1)) || (rc = st->h_ids.resize(n + 1)) || (rc = st->h_out.resize(n * 12)) ||
        (rc = st->h_changed.resize(1)) || (rc = st->d_packed.alloc(total + 64)) || (rc = st->d_bases.alloc(total + 64)) || (rc = st->d_base_off.alloc(n + 1)) ||
        (rc = st->d_bitmap.alloc(bitmap_words)) || (rc = st->d_lim.alloc(n)) || (rc = st->d_lists.alloc(slice * 2 * list_stride)) || (rc = st->d_n_valid.alloc(slice)) ||
        (rc = st->d_ids.alloc(n + 1)) || (rc = st->d_out.alloc(n * 12)) || (rc = st->d_flags.alloc(n)) || (rc = st->d_changed.alloc(1)) ||
        (rc = st->d_cpg.alloc(slice * 2 * S)) || (rc = st->d_best.alloc(slice * 2 * S * std::max(nt, 1u))))
        return rc;
    if ((rc = upload_packed_reads(s, n, bases, base_off, st->h_packed, st->h_base_off, st->d_packed, st->d_base_off, st->d_bases))) return rc;
    RTX_HIP(hipMemcpyAsync(st->d_lim.p, d.lim.data(), n * 4, hipMemcpyHostToDevice, s));  // (pageable: the copy is staged before the call returns)
    RTX_HIP(hipMemsetAsync(st->d_flags.p, 0, n * 4, s));
    if (bitmap_words) RTX_HIP(hipMemsetAsync(st->d_bitmap.p, 0, bitmap_words * 4, s));
    // the entries of every slice by plane class, ascending: ten planes hold n_pos <= 1023, twelve the rest; an entry above
    // RTX_CHIMERA_MAX_QUERY or without a parent prefix is in neither
    const uint64_t n_slices = (n + slice - 1) / slice;
    std::vector<uint32_t> n10(n_slices, 0), n12(n_slices, 0);
    uint32_t *ids = st->h_ids.data();
    for (uint64_t k = 0; k < n_slices; k++) {
        const uint64_t q0 = k * slice, m = std::min<uint64_t>(slice, n - q0);
        uint32_t *mine = ids + q0;
        for (uint64_t q = 0; q < m; q++)
            if (d.lim[q0 + q] && len_of(q0 + q) <= 1030u) mine[n10[k]++] = (uint32_t)q;
        for (uint64_t q = 0; q < m; q++)
            if (d.lim[q0 + q] && len_of(q0 + q) > 1030u && len_of(q0 + q) <= RTX_CHIMERA_MAX_QUERY) mine[n10[k] + n12[k]++] = (uint32_t)q;
    }
    RTX_HIP(hipMemcpyAsync(st->d_ids.p, ids, (n + 1) * 4, hipMemcpyHostToDevice, s));
    DenovoParams p{};
    p.bases = st->d_bases.p;
    p.base_off = st->d_base_off.p;
    p.lim = st->d_lim.p;
    p.bitmap = st->d_bitmap.p;
    p.n = (uint32_t)n;
    p.n_par = n_par;
    p.ntiles = std::max(nt, 1u);
    p.stride_bytes = denovo_stride_bytes(n_par);
    p.S = S;
    p.mindelta = d.params.mindelta;
    p.list_stride = list_stride;
    p.lists = st->d_lists.p;
    p.n_valid = st->d_n_valid.p;
    p.cpg = st->d_cpg.p;
    p.best = st->d_best.p;
    p.out = st->d_out.p;
    p.flags = st->d_flags.p;
    p.changed = st->d_changed.p;
    if (n_par) hipLaunchKernelGGL(denovo_bitmap_kernel, dim3((n_par + 3u) / 4u), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(s));
    double t1 = now_s(), scan_s = 0.0;
    d.seconds[0] = t1 - t0;

    uint64_t in_lists = ~0ull;  // the slice whose row lists the buffers hold
    uint64_t e0 = 0;
    for (d.rounds = 0, d.scans = 0;;) {
        if (d.rounds > n) { set_error("rtx_denovo_check: %u rounds over %llu entries", d.rounds + 1u, (unsigned long long)n); return RTX_ERR_HIP; }
        d.rounds++;
        d.scans += n - e0;
        if (e0 >= n) break;  // nothing to scan: a round that changes nothing
        for (uint64_t k = e0 / slice; k < n_slices; k++) {
            const uint64_t q0 = k * slice, m = std::min<uint64_t>(slice, n - q0);
            const uint32_t qa = (uint32_t)(std::max(e0, q0) - q0);  // the first entry of the slice that the round takes
            p.q0 = (uint32_t)q0;
            if (in_lists != k) {
                hipLaunchKernelGGL(denovo_rows_kernel, dim3((unsigned)m), dim3(64), 0, s, p);
                in_lists = k;
            }
            RTX_HIP(hipEventRecord(st->ev0, s));
            for (int cls = 0; cls < 2; cls++) {
                const uint32_t *mine = ids + q0 + (cls ? n10[k] : 0u);
                const uint32_t cnt = cls ? n12[k] : n10[k];
                ScanGrid g{};
                g.ntiles = nt;
                g.n_ids = cnt;
                const uint32_t from = (uint32_t)(std::lower_bound(mine, mine + cnt, qa) - mine);
                for (uint32_t t = 0; t < nt; t++) {  // the entries with more than t tiles: lim > t * 8192
                    const uint32_t f = (uint32_t)(std::partition_point(mine, mine + cnt, [&](uint32_t q) { return d.lim[q0 + q] <= t * 8192u; }) - mine);
                    g.first[t] = std::max(f, from);
                    g.item[t + 1] = g.item[t] + (cnt - g.first[t]);
                }
                const uint64_t waves = (uint64_t)g.item[nt] * 2u;
                if (!waves) continue;
                p.ids = st->d_ids.p + q0 + (cls ? n10[k] : 0u);
                if (cls == 0) hipLaunchKernelGGL(denovo_scan_kernel<10>, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p, g);
                else hipLaunchKernelGGL(denovo_scan_kernel<12>, dim3((unsigned)((waves + 3u) / 4u)), dim3(256), 0, s, p, g);
            }
            RTX_HIP(hipEventRecord(st->ev1, s));
            hipLaunchKernelGGL(denovo_reduce_kernel, dim3((unsigned)(m - qa)), dim3(64), 0, s, p, qa);
            RTX_HIP(hipGetLastError());
            if ((rc = st->wait())) return rc;  // (the event pair is the slice's: read before the next slice records it again)
            scan_s += (double)st->kernel_ms * 1e-3;
        }
        RTX_HIP(hipMemsetAsync(st->d_changed.p, 0xFF, 4, s));
        hipLaunchKernelGGL(denovo_update_kernel, dim3((unsigned)((n - e0 + 255u) / 256u)), dim3(256), 0, s, p, (uint32_t)e0);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipMemcpyAsync(st->h_changed.data(), st->d_changed.p, 4, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipStreamSynchronize(s));
        const uint32_t c = st->h_changed[0];
        if (c == 0xFFFFFFFFu) break;
        if (c >= n) { set_error("rtx_denovo_check: entry %u of %llu changed", c, (unsigned long long)n); return RTX_ERR_HIP; }
        e0 = (uint64_t)(std::partition_point(d.lim.begin(), d.lim.end(), [&](uint32_t l) { return l <= c; }) - d.lim.begin());
    }
    // the scan kernels by their events; the row lists, the reductions, the flag updates and the read-backs are the rounds' bookkeeping
    const double t2 = now_s();
    d.seconds[1] = scan_s;
    d.seconds[2] = std::max(0.0, t2 - t1 - scan_s);
    t1 = t2;
    RTX_HIP(hipMemcpyAsync(st->h_out.data(), st->d_out.p, n * 48, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    std::memcpy(d.rec.data(), st->h_out.data(), n * 48);
    for (uint64_t e = 0; e < n; e++) {
        const rtx_chimera_rec &r = d.rec[e];
        for (const uint32_t par : {r.parent, r.parent_a, r.parent_b})
            if (par != RTX_NO_REF && par >= d.lim[e]) { set_error("rtx_denovo_check: entry %llu names parent %u, its limit is %u", (unsigned long long)e, par, d.lim[e]); return RTX_ERR_HIP; }
    }
    rtx::denovo_totals(d);
    d.seconds[3] = now_s() - t1;
    return RTX_OK;
}

}  // namespace

static_assert(sizeof(rtx_chimera_rec) == 48 && sizeof(ChimRec) == 48, "twelve uint32");

extern "C" int rtx_denovo_check(int device, rtx_tally_table *table, rtx_otu *otu, const rtx_denovo_params *params, rtx_denovo **out) {
    rtx_tally_view v{};
    rtx_denovo_params prm{};
    if (const int rc = rtx::denovo_open("rtx_denovo_check", table, otu, params, out, &v, &prm)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto *d = new rtx_denovo();
    rtx::denovo_entries(*d, v, otu, prm);
    int rc = RTX_OK;
    if (d->n_entries) {
        auto *st = new DenovoStage();
        rc = st->open(device);
        if (!rc) rc = run(st, v, *d);
        destroy(st);
    }
    if (rc) { delete d; return rc; }
    *out = d;
    return RTX_OK;
}

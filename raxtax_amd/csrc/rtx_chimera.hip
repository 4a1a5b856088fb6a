// Chimera check against the references on the device (rtx_chimera_*): for every read the best single reference over all of its windows
// against the best pair of references over a left and a right part, at S - 1 candidate breakpoints (include/raxtax_hip.h has the exact
// definition; rtx_math.hpp the arithmetic, shared with the x86 emulator).  Like rtx_qual, rtx_trim and rtx_derep the stage stands IN FRONT
// of a handle: an object of its own with one stream and its own buffers.  Unlike them it BORROWS the handle's immutable index arrays -- the
// bitmap (one 1-KiB row per 8-mer and tile, every bit whatever the segment class) and the row table -- so the index must outlive it.
//
// The check is hit_count with positions kept: the rows of a read's windows are folded into bit planes in POSITION order, and the planes --
// never cleared -- are looked at after every segment: they hold the running prefix P_r[s] of every reference of the tile.
//   chimera_rows_kernel    one wave per read: window i -> row_of[k] << 10 (an invalid window or a k-mer without a row: the zero row), written
//                          in the padded layout of chimera_layout -- every segment a multiple of 8 rows -- once per direction, with the zero
//                          row behind the list as far as the scan's look-ahead loads reach; n_valid; the checkpoints in fold groups.
//   chimera_scan_kernel    one wave per (read, tile, direction): groups of eight rows through tree8 + a ripple from plane 3, two groups in
//                          flight; behind the last group of a segment a checkpoint that does not unpack: planes_max per word, a wave maximum,
//                          the candidate bits through the inverse of ref_slot to the lowest reference (chimera_lane_best), a wave minimum, one
//                          vector store of (count, reference).  Direction 0 folds the segments 0 .. S-1: P[1 .. S]; direction 1 folds
//                          S-1 .. 0: Suf[S-1 .. 0].  Ten planes for n_pos <= 1023, twelve above.
//   chimera_reduce_kernel  one wave per read: lane (direction, checkpoint) takes the tiles in ascending order (the first tile that holds the
//                          maximum holds the lowest reference), lane 0 builds the record (chimera_record).
// Vector stores and plain C++, no atomics.
#include <atomic>

#include "rtx_stage.hpp"
#include "rtx_hit_common.hpp"

namespace {

std::atomic<uint64_t> g_chimera_slice{~0ull};  // RTX_DEFAULT_CHIMERA_SLICE (tests: a small batch in many slices)

struct ChimParams {
    const uint8_t *bases;          // the staged reads of the call
    const uint64_t *base_off;      // [reads of the call + 1]
    const uint32_t *row_of;        // the handle's
    const uint32_t *bitmap;
    uint32_t n_rows, ntiles, stride_bytes;
    uint32_t S, mindelta;
    uint64_t q0;                   // read q of the slice is read q0 + q of the call
    uint32_t list_stride;          // entries of a (read, direction) list
    uint32_t *lists;               // [n][2][list_stride]
    uint32_t *n_valid;             // [n]
    uint16_t *cpg;                 // [n][2][S] fold groups in front of checkpoint k
    uint2 *best;                   // [n][2][S][ntiles] (count, reference) per checkpoint and tile
    const uint32_t *ids;           // the reads of the slice that a scan launch takes (one plane class)
    uint32_t n_ids;
    uint32_t *out;                 // [n][12] rtx_chimera_rec
};

__device__ __forceinline__ uint32_t read_len(const ChimParams &p, uint32_t q, uint64_t &b0) {
    b0 = p.base_off[p.q0 + q];
    const uint64_t len = p.base_off[p.q0 + q + 1] - b0;
    return len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
}

__global__ __launch_bounds__(64) void chimera_rows_kernel(ChimParams p) {
    __shared__ uint32_t off[2][kChimMaxSegments + 1];
    const uint32_t q = blockIdx.x, lane = threadIdx.x, S = p.S;
    uint64_t b0;
    const uint32_t len = read_len(p, q, b0);
    const uint32_t n_pos = chimera_n_pos(len);
    if (lane < 2u) chimera_layout(n_pos, S, lane, off[lane]);
    __syncthreads();
    if (lane < 2u * S) p.cpg[(size_t)q * 2u * S + lane] = (uint16_t)(off[lane / S][lane % S + 1u] >> 3);
    const uint32_t cap = chimera_list_cap(off[0][S]);  // (<= list_stride: the host sized it for the longest read of the call)
    const uint32_t zero = p.n_rows << 10;
    const uint8_t *seq = p.bases + b0;
    uint32_t nv = 0;
    for (uint32_t dir = 0; dir < 2u; dir++) {
        uint32_t *list = p.lists + ((size_t)q * 2u + dir) * p.list_stride;
        for (uint32_t j = lane; j < cap; j += 64u) {
            const uint32_t i = chimera_list_window(n_pos, S, dir, off[dir], j);
            uint32_t v = zero, k;
            if (i != kChimNoRef && chimera_window_kmer(seq, i, k)) {
                nv += dir == 0u ? 1u : 0u;
                const uint32_t r = p.row_of[k];
                if (r != kEmptyRow) v = r << 10;
            }
            list[j] = v;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nv += __shfl_xor(nv, d, 64);
    if (lane == 0u) p.n_valid[q] = nv;
}

template <int NP>
__global__ __launch_bounds__(256) void chimera_scan_kernel(ChimParams p) {
    const uint32_t lane = threadIdx.x & 63u, S = p.S;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (uint64_t)p.n_ids * p.ntiles * 2u) return;  // (wave-uniform)
    // tile-major: the waves in flight at one time work on one tile's region of the bitmap, and reads of related sequences ask for the same rows of it
    const uint32_t dir = (uint32_t)(item & 1u), tile = (uint32_t)((item >> 1) / p.n_ids);
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.ids[(item >> 1) % p.n_ids]);
    const uint32_t *list = p.lists + ((size_t)q * 2u + dir) * p.list_stride;
    const uint16_t *cpg = p.cpg + ((size_t)q * 2u + dir) * S;
    const uint32_t G = (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[S - 1u]);  // fold groups of the list
    if (G == 0u) return;  // no window: chimera_reduce_kernel reads nothing of such a read
    uint2 *best = p.best + ((size_t)q * 2u + dir) * S * p.ntiles + tile;  // checkpoint k: best[k * ntiles]
    const __amdgpu_buffer_rsrc_t rsrc = tile_rsrc(p.bitmap, p.n_rows + 1u, tile);
    const uint32_t voff = lane * 16u, L = tile_lanes(p.stride_bytes, tile);
    uint32_t pl[4][NP];
#pragma unroll
    for (int w = 0; w < 4; w++)
#pragma unroll
        for (int b = 0; b < NP; b++) pl[w][b] = 0u;
    uint32_t ncp = 0, next_cp = (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[0]);
    auto checkpoint = [&]() {
        uint32_t m, rl;
        chimera_lane_best<NP>(pl, lane, L, m, rl);
        const uint32_t M = wave_max_u32(m);
        const uint32_t mine = M != 0u && m == M ? tile * 8192u + rl : kChimNoRef;
        const uint32_t R = ~wave_max_u32(~mine);  // the lowest one
        if (lane == 0u) best[(size_t)ncp * p.ntiles] = make_uint2(M, R);
        ncp++;
        next_cp = ncp < S ? (uint32_t)__builtin_amdgcn_readfirstlane((int)cpg[ncp]) : 0xFFFFFFFFu;
    };
    while (next_cp == 0u) checkpoint();  // empty segments in front (fewer windows than segments)
    // Two buffers of eight rows; group g + 2 is requested as soon as group g has been folded.  The row offsets come 64 at a time (eight
    // groups): idv holds those of the group being requested, idn the next 64.  The requests run up to three groups past the list's end and
    // idn a further 64 entries: the zero row (kChimListTail), which exists and adds nothing.
    uint32_t idv = list[lane], idn = list[64u + lane];
    uint4 buf[2][8];
    load8v_at(buf[0], rsrc, voff, idv, 0);
    load8v_at(buf[1], rsrc, voff, idv, 8);
    for (uint32_t g = 0; g < G; g += 2u) {
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const uint32_t gg = g + (uint32_t)b;
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

__global__ __launch_bounds__(64) void chimera_reduce_kernel(ChimParams p) {
    __shared__ uint32_t pm[kChimMaxSegments + 1], pr[kChimMaxSegments + 1], sm[kChimMaxSegments + 1], sr[kChimMaxSegments + 1];
    const uint32_t q = blockIdx.x, lane = threadIdx.x, S = p.S;
    uint64_t b0;
    const uint32_t len = read_len(p, q, b0), nv = p.n_valid[q];
    if (lane <= S) {
        pm[lane] = sm[lane] = 0u;
        pr[lane] = sr[lane] = kChimNoRef;
    }
    __syncthreads();
    if (nv != 0u && len <= kChimMaxQuery && lane < 2u * S) {  // (a read with a valid window has a fold group: every checkpoint of every tile was stored)
        const uint32_t dir = lane / S, k = lane % S;
        const uint2 *b = p.best + ((size_t)q * 2u * S + lane) * p.ntiles;
        uint32_t bc = 0u, br = kChimNoRef;
        for (uint32_t t = 0; t < p.ntiles; t++) {
            const uint2 v = b[t];
            chimera_take(bc, br, v.x, v.y);
        }
        if (dir == 0u) { pm[k + 1u] = bc; pr[k + 1u] = br; }
        else { sm[S - 1u - k] = bc; sr[S - 1u - k] = br; }
    }
    __syncthreads();
    if (lane == 0u) {
        const ChimRec r = chimera_record(len, nv, S, p.mindelta, pm, pr, sm, sr);
        uint32_t *o = p.out + (size_t)q * 12u;
        reinterpret_cast<uint4 *>(o)[0] = make_uint4(r.status, r.n_valid, r.single, r.parent);
        reinterpret_cast<uint4 *>(o)[1] = make_uint4(r.seg, r.pos, r.left, r.parent_a);
        reinterpret_cast<uint4 *>(o)[2] = make_uint4(r.right, r.parent_b, r.delta, r.flag);
    }
}

constexpr uint64_t kBestBudget = 1ull << 30, kListBudget = 1ull << 29;  // bytes of a slice's checkpoint array / row lists

}  // namespace

static_assert(sizeof(rtx_chimera_rec) == 48 && sizeof(ChimRec) == 48, "twelve uint32");

struct rtx_chimera : StageShell {  // (the events stand around the scan kernels of a slice; kernel_ms is their sum over the slices of a run)
    const rtx_index *ix = nullptr;
    uint32_t S = 0, mindelta = 0;
    DevBuf<uint8_t> d_packed, d_bases;
    DevBuf<uint64_t> d_base_off;
    DevBuf<uint32_t> d_lists, d_n_valid, d_ids, d_out;
    DevBuf<uint16_t> d_cpg;
    DevBuf<uint2> d_best;
    PinBuf<uint8_t> h_packed;
    PinBuf<uint64_t> h_base_off;
    PinBuf<uint32_t> h_ids, h_out;
};

namespace rtxi {
void set_chimera_slice(uint64_t cap) { g_chimera_slice.store(cap); }
uint64_t chimera_slice_cap() { return g_chimera_slice.load(); }
}  // namespace rtxi

namespace rtx {
int chimera_check_params(const char *who, const rtx_chimera_params *p) {
    if (!p) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (p->segments < 2u || p->segments > RTX_CHIMERA_MAX_SEGMENTS) {
        set_error("%s: %u segments (2 .. %u)", who, p->segments, RTX_CHIMERA_MAX_SEGMENTS);
        return RTX_ERR_INVALID;
    }
    return RTX_OK;
}
bool index_chimera(const rtx_index *index, rtx_chimera_params *params) {
    if (params) *params = index->chimera;
    return index->chimera_on;
}
}  // namespace rtx

extern "C" {

int rtx_chimera_create(const rtx_index *index, const rtx_chimera_params *params, rtx_chimera **out) {
    if (!out || !index) { set_error("rtx_chimera_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (const int rc = rtx::chimera_check_params("rtx_chimera_create", params)) return rc;
    if (index->n_refs != index->n_total) { set_error("rtx_chimera_create: a reference shard holds a part of the database; the chimera check needs all of it"); return RTX_ERR_INVALID; }
    if (index->strand_opt) {
        set_error("rtx_chimera_create: the handle has RTX_OPT_STRAND set; the chimera check reads a read in the orientation given (both orientations: not done)");
        return RTX_ERR_INVALID;
    }
    RTX_HIP(hipSetDevice(index->device));
    auto c = new rtx_chimera();
    c->ix = index;
    c->S = params->segments;
    c->mindelta = params->mindelta;
    if (const int rc = c->open(index->device)) { delete c; return rc; }  // (the handle's device was checked when the handle was made)
    *out = c;
    return RTX_OK;
}

void rtx_chimera_destroy(rtx_chimera *c) { destroy(c); }

int rtx_chimera_run(rtx_chimera *c, uint64_t n, const uint8_t *bases, const uint64_t *base_off, rtx_chimera_rec *out) {
    if (!c) { set_error("rtx_chimera_run: null argument"); return RTX_ERR_INVALID; }
    c->kernel_ms = 0.f;
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFF0ull) { set_error("rtx_chimera_run: %llu reads in one batch (at most 2^31 - 16)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !out) { set_error("rtx_chimera_run: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::check_reads("rtx_chimera_run", n, base_off, bases, ~0ull)) return rc;
    uint32_t max_pos = 0;
    for (uint64_t q = 0; q < n; q++) max_pos = std::max(max_pos, chimera_n_pos((uint32_t)std::min<uint64_t>(base_off[q + 1] - base_off[q], 0xFFFFFFFFull)));
    const uint64_t total = base_off[n] - base_off[0];
    const rtx_index *ix = c->ix;
    RTX_HIP(hipSetDevice(c->device));
    const uint32_t S = c->S, nt = ix->ntiles;
    // a list is sized for the longest read of the call (at most 4 313 rows + the tail); a slice keeps the checkpoints and the lists in budget
    const uint32_t list_stride = chimera_list_cap(((max_pos + 7u) & ~7u) + 8u * S);
    const uint64_t best_per_read = 2ull * S * nt * sizeof(uint2), list_per_read = 2ull * list_stride * 4u;
    const uint64_t slice = std::max<uint64_t>(1, std::min({n, kBestBudget / best_per_read, kListBudget / list_per_read, chimera_slice_cap()}));
    int rc;
    if ((rc = c->h_packed.resize(total + 64)) || (rc = c->h_base_off.resize(n + 1)) || (rc = c->h_ids.resize(slice)) || (rc = c->h_out.resize(slice * 12)) ||
        (rc = grow(c->d_packed, total + 64)) || (rc = grow(c->d_bases, total + 64)) || (rc = grow(c->d_base_off, n + 1)) ||
        (rc = grow(c->d_lists, slice * 2 * list_stride)) || (rc = grow(c->d_n_valid, slice)) || (rc = grow(c->d_ids, slice)) || (rc = grow(c->d_out, slice * 12)) ||
        (rc = grow(c->d_cpg, slice * 2 * S)) || (rc = grow(c->d_best, slice * 2 * S * nt)))
        return rc;
    hipStream_t s = c->stream;
    if ((rc = upload_packed_reads(s, n, bases, base_off, c->h_packed, c->h_base_off, c->d_packed, c->d_base_off, c->d_bases))) return rc;
    ChimParams p{};
    p.bases = c->d_bases.p;
    p.base_off = c->d_base_off.p;
    p.row_of = ix->d_row_of.p;
    p.bitmap = ix->d_bitmap.p;
    p.n_rows = ix->n_rows;
    p.ntiles = nt;
    p.stride_bytes = ix->stride_bytes;
    p.S = S;
    p.mindelta = c->mindelta;
    p.list_stride = list_stride;
    p.lists = c->d_lists.p;
    p.n_valid = c->d_n_valid.p;
    p.cpg = c->d_cpg.p;
    p.best = c->d_best.p;
    p.out = c->d_out.p;
    for (uint64_t q0 = 0; q0 < n; q0 += slice) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(slice, n - q0);
        // the reads of the slice by plane class: ten planes hold n_pos <= 1023, twelve the rest
        uint32_t n10 = 0, n12 = 0;
        uint32_t *ids = c->h_ids.data();
        for (uint32_t q = 0; q < m; q++) {
            const uint64_t len = base_off[q0 + q + 1] - base_off[q0 + q];
            if (len <= 1030u) ids[n10++] = q;
        }
        for (uint32_t q = 0; q < m; q++) {
            const uint64_t len = base_off[q0 + q + 1] - base_off[q0 + q];
            if (len > 1030u && len <= RTX_CHIMERA_MAX_QUERY) ids[n10 + n12++] = q;
        }
        if (n10 + n12) RTX_HIP(hipMemcpyAsync(c->d_ids.p, ids, (size_t)(n10 + n12) * 4, hipMemcpyHostToDevice, s));
        p.q0 = q0;
        hipLaunchKernelGGL(chimera_rows_kernel, dim3(m), dim3(64), 0, s, p);
        RTX_HIP(hipEventRecord(c->ev0, s));
        if (n10) {
            p.ids = c->d_ids.p;
            p.n_ids = n10;
            hipLaunchKernelGGL(chimera_scan_kernel<10>, dim3((unsigned)(((uint64_t)n10 * nt * 2u + 3u) / 4u)), dim3(256), 0, s, p);
        }
        if (n12) {
            p.ids = c->d_ids.p + n10;
            p.n_ids = n12;
            hipLaunchKernelGGL(chimera_scan_kernel<12>, dim3((unsigned)(((uint64_t)n12 * nt * 2u + 3u) / 4u)), dim3(256), 0, s, p);
        }
        RTX_HIP(hipEventRecord(c->ev1, s));
        hipLaunchKernelGGL(chimera_reduce_kernel, dim3(m), dim3(64), 0, s, p);
        RTX_HIP(hipGetLastError());
        RTX_HIP(hipMemcpyAsync(c->h_out.data(), c->d_out.p, (size_t)m * 48, hipMemcpyDeviceToHost, s));
        const float ms = c->kernel_ms;  // of the slices before this one
        if ((rc = c->wait())) return rc;
        c->kernel_ms += ms;
        std::memcpy(out + q0, c->h_out.data(), (size_t)m * 48);
    }
    return RTX_OK;
}

int rtx_chimera_kernel_time(const rtx_chimera *c, float *ms) { return kernel_time("rtx_chimera_kernel_time", c, ms); }

int rtx_index_set_chimera(rtx_index *index, const rtx_chimera_params *params) {
    if (!index) { set_error("rtx_index_set_chimera: null index"); return RTX_ERR_INVALID; }
    if (!params) {
        index->chimera = rtx_chimera_params{};
        index->chimera_on = false;
        return RTX_OK;
    }
    if (const int rc = rtx::chimera_check_params("rtx_index_set_chimera", params)) return rc;
    index->chimera = *params;
    index->chimera_on = true;
    return RTX_OK;
}

int rtx_index_chimera(const rtx_index *index, rtx_chimera_params *params, int *on) {
    if (!index || !params || !on) { set_error("rtx_index_chimera: null argument"); return RTX_ERR_INVALID; }
    *on = rtx::index_chimera(index, params) ? 1 : 0;
    return RTX_OK;
}

}  // extern "C"

// Quality filter on the device (rtx_qual_*): where a read is cut and why it is discarded, from its FASTQ quality string (include/raxtax_hip.h
// has the exact semantics; rtx_math.hpp the arithmetic, shared with rtx_qual_read on the host and the x86 emulator).  Like rtx_trim and
// rtx_derep the stage stands IN FRONT of a handle (host_raxtax.cpp: rtx_index_set_quality): an object of its own with one stream and its own
// buffers, so that the lookup thread of rtx_raxtax can run it on chunk c + 1 while the handle on that device classifies chunk c.
//
// One byte per base of the input ranges travels: the raw quality byte in bits 0-6, bit 7 set where the base is no A/C/G/T -- the host's
// staging is one OR pass over the two input arrays into pinned memory (qual_stage), the per-base table lookup and the running sums are the
// device's.  Every range starts at a multiple of 16 bytes of the staged array (at most 15 bytes of padding per read, never read as data), so
// that every load is a whole aligned 16-byte piece; a uint32 offset (in pieces) and a uint32 length per read go with it.
//   qual_kernel  a group of 16 lanes per read, four reads per wave, 16 reads per block.  A step is 16 pieces = 256 coalesced bytes of a read:
//                a 250-base read takes one step, a 658-base barcode three; the groups of a wave run as many steps as its longest read.
//                The 94-entry table (computed on the host, uploaded at create) sits in LDS.  Per step: every lane sums its piece
//                (qual_piece_sum: 16 prefix sums in registers), the lane totals are scanned over the group (four row shifts of a 64-bit
//                sum and of the N count), every lane looks for its first stopping byte with what lies in front of it (qual_piece_stop),
//                the first of the group is a minimum over its 16 lanes, and the sums up to there -- or the group's totals, the carry into the
//                next step -- are read from the lane that holds them.  A read is streamed to its end also behind its cut: a byte outside
//                Q 0 .. 93 anywhere in the range decides the verdict.  Lane 0 of the group stores hi, ee and the verdict.
//                Vector stores and plain C++, no atomics.
#include "rtx_stage.hpp"
#include "host_qual.hpp"

namespace {

struct QualParams {
    const uint8_t *bytes;          // the staged ranges; read q at 16 * off16[q]
    const uint32_t *off16, *len;   // [n]
    const uint64_t *table;         // [RTX_QUAL_TABLE]
    uint64_t *ee;                  // [n]
    uint32_t *hi, *verdict;        // [n]
    uint32_t n;
    QualCfg cfg;
};

__global__ __launch_bounds__(256) void qual_kernel(QualParams p) {
    __shared__ uint64_t table[RTX_QUAL_TABLE];
    if (threadIdx.x < RTX_QUAL_TABLE) table[threadIdx.x] = p.table[threadIdx.x];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (kQualGroup - 1u), g0 = lane & ~(kQualGroup - 1u);
    const uint32_t q = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (64u / kQualGroup) + lane / kQualGroup;
    const bool mine = q < p.n;
    uint32_t len = 0;
    const uint4 *row = nullptr;
    if (mine) {
        len = p.len[q];
        row = reinterpret_cast<const uint4 *>(p.bytes + (size_t)p.off16[q] * kQualPiece);
    }
    bool short_tl;
    const uint32_t end = qual_end(p.cfg, len, short_tl);
    constexpr uint32_t kStep = kQualGroup * kQualPiece;
    uint32_t steps = (len + kStep - 1u) / kStep;  // the groups of a wave run in step: as long as its longest read
    steps = max(steps, (uint32_t)__shfl_xor((int)steps, 16, 64));
    steps = max(steps, (uint32_t)__shfl_xor((int)steps, 32, 64));
    uint64_t carry_e = 0;
    uint32_t carry_n = 0, hi = end;
    bool bad = false, done = false;
    for (uint32_t s = 0; s < steps; s++) {  // (wave-uniform; no lane leaves before the shuffles)
        const uint32_t pos = s * kStep + gl * kQualPiece;
        QualWords t{{0u, 0u, 0u, 0u}};
        if (pos < len) {  // (the piece lies inside the read's padded range)
            const uint4 v = row[s * kQualGroup + gl];
            t = QualWords{{v.x, v.y, v.z, v.w}};
        }
        QualPiece pc;
        qual_piece_sum(p.cfg, table, t, pos, len, end, pc);
        bad = bad || pc.bad;
        uint64_t sum_e = pc.c[kQualPiece - 1u];  // -> inclusive over the lanes of the group
        uint32_t sum_n = (uint32_t)__popc(pc.ns);
#pragma unroll
        for (uint32_t d = 1; d < kQualGroup; d <<= 1) {
            const uint64_t oe = __shfl_up(sum_e, d, kQualGroup);
            const uint32_t on = __shfl_up(sum_n, d, kQualGroup);
            if (gl >= d) { sum_e += oe; sum_n += on; }
        }
        const uint64_t before_e = carry_e + sum_e - pc.c[kQualPiece - 1u];
        const uint32_t before_n = carry_n + sum_n - (uint32_t)__popc(pc.ns);
        uint64_t e;
        uint32_t nn;
        const uint32_t stop = qual_piece_stop(p.cfg, pc, before_e, pos, end, e, nn);
        const uint32_t cand = stop != kQualPiece ? pos + stop : 0xFFFFFFFFu;
        uint32_t first = cand;
#pragma unroll
        for (uint32_t d = 1; d < kQualGroup; d <<= 1) first = min(first, (uint32_t)__shfl_xor((int)first, (int)d, kQualGroup));
        const bool found = first != 0xFFFFFFFFu;
        // the sums in front of the cut lie with the lane that holds it; without a cut the last lane holds the group's totals (its e is its whole piece)
        const uint32_t holders = (uint32_t)(__ballot(found && cand == first) >> g0) & 0xFFFFu;
        const uint32_t src = g0 + (found ? (uint32_t)__ffs((int)holders) - 1u : kQualGroup - 1u);
        const uint64_t at_e = __shfl(before_e + e, (int)src, 64);
        const uint32_t at_n = __shfl(before_n + nn, (int)src, 64);
        if (!done) {
            carry_e = at_e;
            carry_n = at_n;
            if (found) { hi = first; done = true; }
        }
    }
    const bool bad_any = ((uint32_t)(__ballot(bad) >> g0) & 0xFFFFu) != 0u;
    if (mine && gl == 0u) {
        p.hi[q] = bad_any ? 0u : hi;
        p.ee[q] = bad_any ? 0ull : carry_e;
        p.verdict[q] = qual_verdict(p.cfg, bad_any, short_tl, hi, carry_e, carry_n);
    }
}

}  // namespace

struct rtx_qual : StageShell {
    QualCfg cfg{};
    DevBuf<uint64_t> d_table, d_ee;
    DevBuf<uint8_t> d_bytes;
    DevBuf<uint32_t> d_in, d_out;             // off16 | len; hi | verdict
    PinBuf<uint8_t> h_bytes;
    PinBuf<uint32_t> h_in, h_out;
    PinBuf<uint64_t> h_ee;
};

namespace rtx {
bool index_quality(const rtx_index *index, rtx_qual_params *params) {
    if (params) *params = index->quality;
    return index->quality_on;
}
}  // namespace rtx

extern "C" {

int rtx_qual_create(int device, const rtx_qual_params *params, rtx_qual **out) {
    if (!out || !params) { set_error("rtx_qual_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (const int rc = rtx::qual_check_params("rtx_qual_create", params)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto q = new rtx_qual();
    rtx::qual_cfg_init(q->cfg, *params);
    if (const int rc = q->open(device)) { delete q; return rc; }
    if (q->d_table.alloc(RTX_QUAL_TABLE) != RTX_OK ||
        hipMemcpy(q->d_table.p, rtx::qual_table(), sizeof(uint64_t) * RTX_QUAL_TABLE, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("rtx_qual_create: the error table could not be uploaded");
        delete q;
        return RTX_ERR_HIP;
    }
    *out = q;
    return RTX_OK;
}

void rtx_qual_destroy(rtx_qual *q) { destroy(q); }

int rtx_qual_run(rtx_qual *q, uint64_t n, const uint8_t *bases, const uint8_t *quals, const uint64_t *base_off, const uint32_t *lo_in,
                 const uint32_t *hi_in, uint32_t *hi_out, uint64_t *ee_out, uint32_t *verdict_out) {
    if (!q) { set_error("rtx_qual_run: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFF0ull) { set_error("rtx_qual_run: %llu reads in one batch (at most 2^31 - 16)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !hi_out || !ee_out || !verdict_out || (lo_in == nullptr) != (hi_in == nullptr)) { set_error("rtx_qual_run: null argument"); return RTX_ERR_INVALID; }
    q->begin();
    int rc;
    if ((rc = q->h_in.resize(2 * n))) return rc;
    uint32_t *h_off = q->h_in.data(), *h_len = h_off + n;
    uint64_t pieces = 0;
    if ((rc = rtx::layout_ranges("rtx_qual_run", n, base_off, lo_in, hi_in, RTX_QUAL_MAX_READ, kQualPiece, h_off, h_len, &pieces))) return rc;
    if (pieces && (!bases || !quals)) { set_error("rtx_qual_run: null bases or quals"); return RTX_ERR_INVALID; }
    RTX_HIP(hipSetDevice(q->device));
    const size_t bytes = (size_t)pieces * kQualPiece;
    if ((rc = q->h_bytes.resize(bytes + 16)) || (rc = q->h_out.resize(2 * n)) || (rc = q->h_ee.resize(n)) || (rc = grow(q->d_bytes, bytes + 16)) ||
        (rc = grow(q->d_in, 2 * n)) || (rc = grow(q->d_out, 2 * n)) || (rc = grow(q->d_ee, n)))
        return rc;
    uint8_t *hb = q->h_bytes.data();
    const unsigned nt = std::max(1u, rtx::host_threads(4u));
    std::vector<uint8_t> seen(nt, 0);  // per thread of the fan
    rtx::parallel_ranges(n, nt, 4096, [&](unsigned k, uint64_t a, uint64_t b) {
        uint8_t s = 0;
        for (uint64_t r = a; r < b; r++) {
            const uint64_t at = base_off[r] + (lo_in ? lo_in[r] : 0u);
            if (h_len[r]) s |= rtx::qual_stage(bases + at, quals + at, h_len[r], hb + (size_t)h_off[r] * kQualPiece);
        }
        seen[k] = s;
    });
    for (uint8_t s : seen)
        if (s & 0x80u) { set_error("rtx_qual_run: a quality byte of 128 or more"); return RTX_ERR_INVALID; }
    q->staged();
    hipStream_t s = q->stream;
    if (bytes) RTX_HIP(hipMemcpyAsync(q->d_bytes.p, hb, bytes, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(q->d_in.p, h_off, 2 * n * 4, hipMemcpyHostToDevice, s));
    QualParams p{};
    p.bytes = q->d_bytes.p;
    p.off16 = q->d_in.p;
    p.len = q->d_in.p + n;
    p.table = q->d_table.p;
    p.ee = q->d_ee.p;
    p.hi = q->d_out.p;
    p.verdict = q->d_out.p + n;
    p.n = (uint32_t)n;
    p.cfg = q->cfg;
    const unsigned per_block = 4u * (64u / kQualGroup);
    RTX_HIP(hipEventRecord(q->ev0, s));
    hipLaunchKernelGGL(qual_kernel, dim3((unsigned)((n + per_block - 1u) / per_block)), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipEventRecord(q->ev1, s));
    RTX_HIP(hipMemcpyAsync(q->h_out.data(), q->d_out.p, 2 * n * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(q->h_ee.data(), q->d_ee.p, n * 8, hipMemcpyDeviceToHost, s));
    if ((rc = q->wait())) return rc;
    for (uint64_t r = 0; r < n; r++) hi_out[r] = (lo_in ? lo_in[r] : 0u) + q->h_out.data()[r];
    scatter_columns(q->h_out.data() + n, n, {verdict_out});
    std::memcpy(ee_out, q->h_ee.data(), n * 8);
    q->finish();
    return RTX_OK;
}

int rtx_qual_kernel_time(const rtx_qual *q, float *ms) { return kernel_time("rtx_qual_kernel_time", q, ms); }

int rtx_qual_stage_times(const rtx_qual *q, double seconds[3]) { return stage_times("rtx_qual_stage_times", q, seconds); }

int rtx_index_set_quality(rtx_index *index, const rtx_qual_params *params) {
    if (!index) { set_error("rtx_index_set_quality: null index"); return RTX_ERR_INVALID; }
    if (!params) {  // honoured by the host mirror alone (host_raxtax.cpp): nothing else of the handle changes
        index->quality = rtx_qual_params{};
        index->quality_on = false;
        return RTX_OK;
    }
    if (const int rc = rtx::qual_check_params("rtx_index_set_quality", params)) return rc;
    index->quality_on = rtx::qual_params_on(*params);
    index->quality = index->quality_on ? *params : rtx_qual_params{};
    return RTX_OK;
}

int rtx_index_quality(const rtx_index *index, rtx_qual_params *params, int *on) {
    if (!index || !params || !on) { set_error("rtx_index_quality: null argument"); return RTX_ERR_INVALID; }
    *on = rtx::index_quality(index, params) ? 1 : 0;
    return RTX_OK;
}

}  // extern "C"

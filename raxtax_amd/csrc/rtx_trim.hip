// Primer trimming on the device (rtx_trim_*): where the PCR primers of an amplicon read end, per read and per end (include/raxtax_hip.h has
// the exact semantics: Sellers' search of each pattern in a window at the read's end, IUPAC codes matched by an AND, the least errors and
// then the lowest index among the patterns of an end).  The stage stands IN FRONT of a handle and of dereplication (host_raxtax.cpp:
// rtx_index_set_primers): an object of its own with one stream and its own buffers, so that the lookup thread of rtx_raxtax can run it on
// chunk c + 1 while the handle on that device classifies chunk c.
//
// Only the ends of the reads travel: the host stages, per read, the first W5 and the last W3 bases (the largest windows of either end; the 3'
// window reversed, so that a 3' search is the 5' search of the reversed problem) into pinned rows of a fixed stride -- two bases per byte, a
// byte above 15 as 0 (both match nothing: every batch packs), whole 16-byte loads -- and a uint32 length per read.  Row q lies at
// q * stride: about a fifth of the bytes of the whole reads, and regular addressing.
//   trim_kernel  one lane per read.  The patterns (four one-hot bit planes, m, k, w; the 3' ones reversed at create) arrive in the kernel
//                argument and stay in scalar registers; the loop over the patterns of an end and the loop over the 32-base chunks of a
//                window are uniform over the wave, a lane whose read has ended sits the steps out.  Eq is the OR of the planes the text
//                code selects (identity_step), Pv / Mv are 64 bits per lane, the score is followed at bit m - 1, the best (e, j) is kept
//                with <=.  trim_read / trim_search (rtx_math.hpp) carry all of it; rtx_primer_search and the x86 emulator call the same.
//                Vector stores and plain C++, no atomics, no LDS.
#include "rtx_stage.hpp"

namespace {

struct TrimParams {
    const uint8_t *rows5, *rows3;  // [n] rows of stride5 / stride3 bytes (null when the end has no pattern)
    const uint32_t *len;           // [n]
    uint32_t n, stride5, stride3, n5, n3;
    uint32_t *lo, *hi, *hit;       // [n]
    TrimPattern pat[RTX_TRIM_MAX_PATTERNS];  // the 5' ones, then the 3' ones
};

__global__ __launch_bounds__(256) void trim_kernel(TrimParams p) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= p.n) return;
    // (a pointer that is never dereferenced when its end has no pattern: trim_read runs no search there)
    const uint4 *row5 = reinterpret_cast<const uint4 *>(p.rows5 + (size_t)q * p.stride5);
    const uint4 *row3 = reinterpret_cast<const uint4 *>(p.rows3 + (size_t)q * p.stride3);
    auto load5 = [row5](uint32_t c) { const uint4 v = row5[c]; return TrimWords{{v.x, v.y, v.z, v.w}}; };
    auto load3 = [row3](uint32_t c) { const uint4 v = row3[c]; return TrimWords{{v.x, v.y, v.z, v.w}}; };
    uint32_t lo, hi, hit;
    trim_read(p.pat, p.n5, p.n3, load5, load3, p.len[q], lo, hi, hit);
    p.lo[q] = lo;
    p.hi[q] = hi;
    p.hit[q] = hit;
}

}  // namespace

struct rtx_trim : StageShell {
    TrimPattern pat[RTX_TRIM_MAX_PATTERNS];
    uint32_t n5 = 0, n3 = 0, w5 = 0, w3 = 0;
    DevBuf<uint8_t> d_rows;
    DevBuf<uint32_t> d_len, d_out;
    PinBuf<uint8_t> h_rows;
    PinBuf<uint32_t> h_len, h_out;
};

namespace rtx {
const std::vector<TrimPrimer> &index_primers(const rtx_index *index) { return index->primers; }
}  // namespace rtx

extern "C" {

int rtx_trim_create(int device, const rtx_trim_pattern *pats, uint32_t n, rtx_trim **out) {
    if (!out || !pats) { set_error("rtx_trim_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (n == 0) { set_error("rtx_trim_create: no patterns"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::trim_check_patterns("rtx_trim_create", pats, n)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto t = new rtx_trim();
    for (uint32_t e = 0; e < 2u; e++)  // the 5' patterns, then the 3' ones, each end in the order of the list
        for (uint32_t i = 0; i < n; i++) {
            if (pats[i].end != e) continue;
            TrimPattern &p = t->pat[t->n5 + t->n3];
            trim_pattern_init(p, pats[i].codes, pats[i].len, pats[i].max_errors, pats[i].window, e == RTX_TRIM_3P, i);
            (e ? t->n3 : t->n5)++;
            uint32_t &w = e ? t->w3 : t->w5;
            w = std::max(w, p.w);
        }
    if (const int rc = t->open(device)) { delete t; return rc; }
    *out = t;
    return RTX_OK;
}

void rtx_trim_destroy(rtx_trim *t) { destroy(t); }

int rtx_trim_run(rtx_trim *t, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *lo, uint32_t *hi, uint32_t *hit) {
    if (!t) { set_error("rtx_trim_run: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFFEull) { set_error("rtx_trim_run: %llu reads in one batch (at most 2^31 - 2)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !lo || !hi || !hit) { set_error("rtx_trim_run: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::check_reads("rtx_trim_run", n, base_off, bases, 0xFFFFFFFFull)) return rc;
    RTX_HIP(hipSetDevice(t->device));
    const uint32_t s5 = t->n5 ? trim_row_stride(t->w5) : 0u, s3 = t->n3 ? trim_row_stride(t->w3) : 0u;
    const size_t row_bytes = (size_t)n * (s5 + s3);
    int rc;
    if ((rc = t->h_rows.resize(row_bytes + 16)) || (rc = t->h_len.resize(n)) || (rc = t->h_out.resize(3 * n)) || (rc = grow(t->d_rows, row_bytes + 16)) ||
        (rc = grow(t->d_len, n)) || (rc = grow(t->d_out, 3 * n)))
        return rc;
    uint8_t *h5 = t->h_rows.data(), *h3 = h5 + (size_t)n * s5;  // (n * s5 is a multiple of 16: the 3' rows are aligned as well)
    uint32_t *hl = t->h_len.data();
    stage_end_rows(n, bases, base_off, t->w5, s5, t->w3, s3, h5, h3, hl);
    hipStream_t s = t->stream;
    if (row_bytes) RTX_HIP(hipMemcpyAsync(t->d_rows.p, h5, row_bytes, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(t->d_len.p, hl, n * 4, hipMemcpyHostToDevice, s));
    TrimParams p{};
    p.rows5 = t->d_rows.p;
    p.rows3 = t->d_rows.p + (size_t)n * s5;
    p.len = t->d_len.p;
    p.n = (uint32_t)n;
    p.stride5 = s5;
    p.stride3 = s3;
    p.n5 = t->n5;
    p.n3 = t->n3;
    p.lo = t->d_out.p;
    p.hi = t->d_out.p + n;
    p.hit = t->d_out.p + 2 * n;
    for (uint32_t i = 0; i < t->n5 + t->n3; i++) p.pat[i] = t->pat[i];
    RTX_HIP(hipEventRecord(t->ev0, s));
    hipLaunchKernelGGL(trim_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipEventRecord(t->ev1, s));
    RTX_HIP(hipMemcpyAsync(t->h_out.data(), t->d_out.p, 3 * n * 4, hipMemcpyDeviceToHost, s));
    if ((rc = t->wait())) return rc;
    scatter_columns(t->h_out.data(), n, {lo, hi, hit});
    return RTX_OK;
}

int rtx_index_set_primers(rtx_index *index, const rtx_trim_pattern *pats, uint32_t n) {
    if (!index) { set_error("rtx_index_set_primers: null index"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::trim_check_patterns("rtx_index_set_primers", pats, n)) return rc;
    std::vector<rtx::TrimPrimer> list(n);  // honoured by the host mirror alone (host_raxtax.cpp): nothing else of the handle changes
    for (uint32_t i = 0; i < n; i++) {
        list[i].codes.assign(pats[i].codes, pats[i].codes + pats[i].len);
        list[i].end = pats[i].end;
        list[i].max_errors = pats[i].max_errors;
        list[i].window = pats[i].window;
    }
    index->primers.swap(list);
    return RTX_OK;
}

int rtx_index_primers(const rtx_index *index, uint32_t *n) {
    if (!index || !n) { set_error("rtx_index_primers: null argument"); return RTX_ERR_INVALID; }
    *n = (uint32_t)index->primers.size();
    return RTX_OK;
}

int rtx_trim_kernel_time(const rtx_trim *t, float *ms) { return kernel_time("rtx_trim_kernel_time", t, ms); }

}  // extern "C"

// Sample demultiplexing on the device (rtx_demux_*): which inline tag stands at each end of a read and which sample the pair names
// (include/raxtax_hip.h has the exact semantics: Hamming distance of every tag of an end at the offsets 0 .. max_offset, IUPAC codes matched
// by an AND, the least distance wins, two tags at the least distance are ambiguous).  An object of its own like rtx_trim: one stream and
// its own buffers, no rtx_index.
//
// Only the ends of the reads travel, as in rtx_trim_run: the host stages, per read, the first and the last max_offset + 32 bases (the 3'
// window reversed) into pinned rows of a fixed stride -- two bases per byte, a byte above 15 as 0, whole 16-byte loads (trim_stage_row) --
// and a uint32 length per read.  Row q lies at q * stride: no lane reads outside its own row, whatever the read's length.
//   demux_kernel  one lane per read.  The tags (two 64-bit words of nibbles, the codes behind the tag zero; m; the place in the caller's
//                 list) lie in global memory, 5' then 3', and are read by the index of a loop that is uniform over the wave: scalar loads
//                 through the scalar cache, which a list of 96 + 96 tags (4.5 KiB) fits; 1024 + 1024 (48 KiB) are served from L2.  Not
//                 LDS: a copy per workgroup would cost its fill and, at the largest list, the occupancy that hides those loads.  The
//                 window is shifted by one nibble per offset; per (offset, tag) two ANDs, two folds of a nibble to a bit and two
//                 popcounts (demux_end, rtx_math.hpp).  The pair table is dense, (n5 + 1) x (n3 + 1) uint32 in HBM, one load per read.
//                 rtx_demux_read and the x86 emulator call the same demux_read.  Vector stores and plain C++, no atomics, no LDS.
#include "rtx_stage.hpp"

#include "host_demux.hpp"

namespace {

struct DemuxKernelParams {
    const uint8_t *rows5, *rows3;  // [n] rows of `stride` bytes
    const uint32_t *len;           // [n]
    const DemuxTag *tags;          // [n5 + n3]
    const uint32_t *table;         // demux_table_size(n5, n3)
    uint32_t n, stride, n5, n3, max_mismatches, max_offset;
    uint32_t *sample, *lo, *hi, *hit, *info;  // [n]
};

__device__ __forceinline__ DemuxWindow load_window(const uint8_t *row, uint32_t stride) {
    const uint4 a = *reinterpret_cast<const uint4 *>(row);
    DemuxWindow x{{a.x | ((uint64_t)a.y << 32), a.z | ((uint64_t)a.w << 32), 0ull}};
    if (stride > 16u) {  // (uniform: max_offset > 0)
        const uint4 b = *reinterpret_cast<const uint4 *>(row + 16);
        x.w[2] = b.x | ((uint64_t)b.y << 32);
    }
    return x;
}

__global__ __launch_bounds__(256) void demux_kernel(DemuxKernelParams p) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= p.n) return;
    const DemuxWindow x5 = load_window(p.rows5 + (size_t)q * p.stride, p.stride);
    const DemuxWindow x3 = load_window(p.rows3 + (size_t)q * p.stride, p.stride);
    const uint32_t *table = p.table;
    const uint32_t n3 = p.n3;
    auto pair = [table, n3](uint32_t i5, uint32_t i3) { return table[demux_table_slot(n3, i5, i3)]; };
    uint32_t sample, lo, hi, hit, info;
    demux_read(p.tags, p.n5, p.n3, pair, p.max_mismatches, p.max_offset, x5, x3, p.len[q], sample, lo, hi, hit, info);
    p.sample[q] = sample;
    p.lo[q] = lo;
    p.hi[q] = hi;
    p.hit[q] = hit;
    p.info[q] = info;
}

}  // namespace

struct rtx_demux : StageShell {
    uint32_t n5 = 0, n3 = 0, max_mismatches = 0, max_offset = 0;
    DevBuf<DemuxTag> d_tags;
    DevBuf<uint32_t> d_table;
    DevBuf<uint8_t> d_rows;
    DevBuf<uint32_t> d_len, d_out;
    PinBuf<uint8_t> h_rows;
    PinBuf<uint32_t> h_len, h_out;
};

namespace rtx {
const DemuxList &index_tags(const rtx_index *index) { return index->tags; }
uint32_t index_profile_samples(const rtx_index *index) { return index->prof.on ? index->prof.n_samples : 0u; }
}  // namespace rtx

extern "C" {

int rtx_index_set_tags(rtx_index *index, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                       const rtx_demux_params *params) {
    if (!index) { set_error("rtx_index_set_tags: null index"); return RTX_ERR_INVALID; }
    rtx::DemuxList list;  // honoured by the host mirror alone (host_raxtax.cpp): nothing else of the handle changes
    if (n_tags) {
        rtx::DemuxSet set;
        if (const int rc = rtx::demux_build("rtx_index_set_tags", tags, n_tags, pairs, n_pairs, params, set)) return rc;
        for (uint32_t i = 0; i < n_tags; i++) {
            list.codes.emplace_back(tags[i].codes, tags[i].codes + tags[i].len);
            list.end.push_back(tags[i].end);
        }
        list.pairs.assign(pairs, pairs + n_pairs);
        list.params = *params;
    }
    index->tags = std::move(list);
    return RTX_OK;
}

int rtx_index_tags(const rtx_index *index, uint32_t *n_tags) {
    if (!index || !n_tags) { set_error("rtx_index_tags: null argument"); return RTX_ERR_INVALID; }
    *n_tags = (uint32_t)index->tags.codes.size();
    return RTX_OK;
}

int rtx_demux_create(int device, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                     const rtx_demux_params *params, rtx_demux **out) {
    if (!out) { set_error("rtx_demux_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    rtx::DemuxSet set;
    if (const int rc = rtx::demux_build("rtx_demux_create", tags, n_tags, pairs, n_pairs, params, set)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto d = new rtx_demux();
    d->n5 = set.n5;
    d->n3 = set.n3;
    d->max_mismatches = set.max_mismatches;
    d->max_offset = set.max_offset;
    const std::vector<uint32_t> table = set.dense_table();
    auto upload = [&]() -> int {
        int rc;
        if ((rc = d->d_tags.alloc(set.tags.size())) || (rc = d->d_table.alloc(table.size()))) return rc;
        RTX_HIP(hipMemcpy(d->d_tags.p, set.tags.data(), set.tags.size() * sizeof(DemuxTag), hipMemcpyHostToDevice));
        RTX_HIP(hipMemcpy(d->d_table.p, table.data(), table.size() * 4, hipMemcpyHostToDevice));
        return RTX_OK;
    };
    int rc = d->open(device);
    if (!rc) rc = upload();
    if (rc) { delete d; return rc; }
    *out = d;
    return RTX_OK;
}

void rtx_demux_destroy(rtx_demux *d) { destroy(d); }

int rtx_demux_run(rtx_demux *d, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *sample, uint32_t *lo, uint32_t *hi,
                  uint32_t *hit, uint32_t *info) {
    if (!d) { set_error("rtx_demux_run: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFFEull) { set_error("rtx_demux_run: %llu reads in one batch (at most 2^31 - 2)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !sample || !lo || !hi || !hit || !info) { set_error("rtx_demux_run: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::check_reads("rtx_demux_run", n, base_off, bases, 0xFFFFFFFFull)) return rc;
    RTX_HIP(hipSetDevice(d->device));
    const uint32_t w = demux_window(d->max_offset), stride = trim_row_stride(w);  // (16 or 32: the 3' rows are aligned as well)
    const size_t row_bytes = (size_t)n * stride * 2u;
    int rc;
    if ((rc = d->h_rows.resize(row_bytes)) || (rc = d->h_len.resize(n)) || (rc = d->h_out.resize(5 * n)) || (rc = grow(d->d_rows, row_bytes)) ||
        (rc = grow(d->d_len, n)) || (rc = grow(d->d_out, 5 * n)))
        return rc;
    uint8_t *h5 = d->h_rows.data(), *h3 = h5 + (size_t)n * stride;
    uint32_t *hl = d->h_len.data();
    stage_end_rows(n, bases, base_off, w, stride, w, stride, h5, h3, hl);
    hipStream_t s = d->stream;
    RTX_HIP(hipMemcpyAsync(d->d_rows.p, h5, row_bytes, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(d->d_len.p, hl, n * 4, hipMemcpyHostToDevice, s));
    DemuxKernelParams p{};
    p.rows5 = d->d_rows.p;
    p.rows3 = d->d_rows.p + (size_t)n * stride;
    p.len = d->d_len.p;
    p.tags = d->d_tags.p;
    p.table = d->d_table.p;
    p.n = (uint32_t)n;
    p.stride = stride;
    p.n5 = d->n5;
    p.n3 = d->n3;
    p.max_mismatches = d->max_mismatches;
    p.max_offset = d->max_offset;
    p.sample = d->d_out.p;
    p.lo = d->d_out.p + n;
    p.hi = d->d_out.p + 2 * n;
    p.hit = d->d_out.p + 3 * n;
    p.info = d->d_out.p + 4 * n;
    RTX_HIP(hipEventRecord(d->ev0, s));
    hipLaunchKernelGGL(demux_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipEventRecord(d->ev1, s));
    RTX_HIP(hipMemcpyAsync(d->h_out.data(), d->d_out.p, 5 * n * 4, hipMemcpyDeviceToHost, s));
    if ((rc = d->wait())) return rc;
    scatter_columns(d->h_out.data(), n, {sample, lo, hi, hit, info});
    return RTX_OK;
}

int rtx_demux_kernel_time(const rtx_demux *d, float *ms) { return kernel_time("rtx_demux_kernel_time", d, ms); }

}  // extern "C"

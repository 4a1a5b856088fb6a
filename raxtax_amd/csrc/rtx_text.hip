// The `.out` and `.tsv` text of a download, produced on the device: the same bytes rtx_format_query (host_format.cpp) prints for the view,
// the labels and the exact matches of the batch -- the generators are rtx_math.hpp's (text_out_row, text_tsv_row), which the x86 emulation
// runs as well (tests/test_text_format_cpu.py).
//
// Three passes per text (`.out`, then `.tsv` when asked for), behind the batch's final rows (rtx_finalise.hip):
//   measure  a thread per query counts the bytes of its lines (+ the NUL)        -> len[q]
//   scan     rocprim's exclusive scan                                            -> off[q], off[nq] = total
//   write    a wave per query: each lane takes rows of the query (row offsets from a wave scan of their lengths) and writes the bytes of
//            its rows that fall into a window of the text into LDS; the wave then stores the window with 16-byte stores (byte stores only at
//            the two unaligned ends of a query's text, which it shares with its neighbours).  Long texts (labels of kilobytes, reads of
//            thousands of bases under --tsv) take several windows; a row is regenerated per window it touches and clipped to it.
// The host reads the total between the scan and the write, so the buffer is sized before anything is written: no truncation, no rerun.
// Per query (input order) its lines joined by '\n' and a NUL; status != RTX_Q_OK: the empty text.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "rtx_index.hpp"
#include "rtx_wave.hpp"

namespace rtx {

struct TextParams {
    TextSrc src;  // lineage table + final rows
    uint64_t nq;
    const uint8_t *status;
    const unsigned long long *row_begin;
    const uint32_t *row_count;
    const double *gs;
    const char *labels;
    const uint64_t *label_off;
    // exact matches: the device lookup's groups (grp != nullptr) or the ids the caller passed (ex_off / ex_ids)
    const uint32_t *grp, *goff, *gids;
    const uint64_t *ex_off;
    const uint32_t *ex_ids;
    bool override_ok;  // neither RTX_SKIP_EXACT_MATCHES nor RTX_RAW_CONFIDENCE
    bool tsv;
    const uint8_t *bases;  // the batch's input set: two bases per byte (packed) or one
    const uint64_t *base_off;
    bool packed;
    unsigned long long *len;       // measure: [nq + 1] (the last one 0)
    const unsigned long long *off;  // write: [nq + 1]
    char *text;
    uint64_t cap;
};

__device__ __forceinline__ uint32_t text_one(const TextParams &p, uint64_t q) {  // the only exact match, or kTextNoOverride
    if (!p.override_ok) return kTextNoOverride;
    return exact_only(ExactRef{p.ex_ids, p.ex_off, p.grp, p.goff, p.gids}, q);
}

__device__ __forceinline__ uint32_t text_rows(const TextParams &p, uint64_t q, uint32_t one) {
    const uint32_t n = p.status[q] != RTX_Q_OK ? 0u : p.row_count[q];
    return n == 0u ? 0u : (one != kTextNoOverride ? 1u : n);
}

// row i of query q through sink s (with the '\n' in front of every row but the first)
template <class S>
__device__ __forceinline__ void text_emit(S &s, const TextParams &p, uint64_t q, uint32_t i, uint32_t one) {
    if (i) s.put('\n');
    const uint64_t l0 = p.label_off[q];
    const TextRow r = text_row(p.src, p.labels + l0, p.label_off[q + 1] - l0, p.row_begin[q], i, one, p.gs[q]);
    if (p.tsv) {
        const uint64_t b0 = p.base_off[q];
        const uint8_t *bases = p.bases;
        if (p.packed)
            text_tsv_row(s, r, p.base_off[q + 1] - b0, [&](uint64_t j) { const uint64_t k = b0 + j; return (uint8_t)((bases[k >> 1] >> ((k & 1u) * 4u)) & 15u); });
        else
            text_tsv_row(s, r, p.base_off[q + 1] - b0, [&](uint64_t j) { return bases[b0 + j]; });
    } else {
        text_out_row(s, r);
    }
}

__global__ __launch_bounds__(256) void text_measure_kernel(TextParams p) {
    const uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (q >= p.nq) return;
    const uint32_t one = text_one(p, q), n = text_rows(p, q, one);
    TextCount c;
    for (uint32_t i = 0; i < n; i++) text_emit(c, p, q, i, one);
    p.len[q] = c.pos + 1u;  // + the NUL
}

constexpr uint32_t kTextWaves = 4;
constexpr uint32_t kTextWin = 4096;     // bytes of a window (a multiple of 16)
constexpr uint32_t kTextRounds = 4;     // rows per lane: 4 x 64 >= kWalkMaxRows
static_assert(kTextRounds * 64u >= kWalkMaxRows, "the rows of a query must fit the lanes of a wave");

__global__ __launch_bounds__(kTextWaves * 64) void text_write_kernel(TextParams p) {
    __shared__ __attribute__((aligned(16))) char s_win[kTextWaves][kTextWin + 16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * kTextWaves + wave;
    if (q >= p.nq) return;  // (wave-uniform)
    const uint64_t base = p.off[q], total = p.off[q + 1] - base;  // with the NUL
    if (base + total > p.cap) return;  // (the host sized the buffer from the same offsets)
    const uint32_t one = text_one(p, q), n = text_rows(p, q, one);
    uint64_t r_start[kTextRounds], r_len[kTextRounds];
    uint64_t carry = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTextRounds; k++) {
        const uint32_t i = k * 64u + lane;
        TextCount c;
        if (i < n) text_emit(c, p, q, i, one);
        const uint32_t len = (uint32_t)c.pos;  // (a row is below 4 GiB)
        const uint32_t incl = wave_incl_scan_u32(len);
        r_start[k] = carry + incl - len;
        r_len[k] = len;
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    char *const win = s_win[wave];
    const uint32_t shift = (uint32_t)((uintptr_t)(p.text + base) & 15u);  // window byte j sits at win[shift + j]: global and LDS agree mod 16
    for (uint64_t w0 = 0; w0 < total; w0 += kTextWin) {
        const uint64_t w1 = w0 + kTextWin < total ? w0 + kTextWin : total;
#pragma unroll
        for (uint32_t k = 0; k < kTextRounds; k++) {
            const uint32_t i = k * 64u + lane;
            if (i < n && r_start[k] < w1 && r_start[k] + r_len[k] > w0) {
                TextWindow tw{win + shift, r_start[k], w0, w1};
                text_emit(tw, p, q, i, one);
            }
        }
        if (lane == 0 && total - 1u >= w0 && total - 1u < w1) win[shift + (total - 1u - w0)] = '\0';
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // store the window: 16-byte chunks of the aligned span, bytes only where the chunk holds bytes of a neighbour
        char *const g = p.text + base + w0 - shift;  // 16-byte aligned
        const uint32_t end = shift + (uint32_t)(w1 - w0), n_chunks = (end + 15u) >> 4;
        for (uint32_t c = lane; c < n_chunks; c += 64u) {
            const uint32_t a = c << 4;
            if (a >= shift && a + 16u <= end) {
                *reinterpret_cast<uint4 *>(g + a) = *reinterpret_cast<const uint4 *>(win + a);
            } else {
                for (uint32_t j = a < shift ? shift : a; j < a + 16u && j < end; j++) g[j] = win[j];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace rtx

namespace rtxi {

// One text (`.out`, or `.tsv`) of the batch whose final rows are on the device: measure, scan, size, write, copy into hv / hoff.
static int text_pass(rtx_index *ix, TextParams p, hipStream_t s, PinBuf<char> &hv, PinBuf<uint64_t> &hoff) {
    const uint64_t nq = p.nq;
    int rc;
    if ((rc = ix->d_text_len.alloc(nq + 1)) || (rc = ix->d_text_off.alloc(nq + 1))) return rc;
    RTX_HIP(hipMemsetAsync(ix->d_text_len.p + nq, 0, 8, s));
    p.len = ix->d_text_len.p;
    hipLaunchKernelGGL(text_measure_kernel, dim3((unsigned)((nq + 255u) / 256u)), dim3(256), 0, s, p);
    size_t tmp_bytes = 0;
    RTX_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, ix->d_text_len.p, ix->d_text_off.p, 0ull, nq + 1, rocprim::plus<unsigned long long>(), s));
    if ((rc = ix->d_text_tmp.alloc(tmp_bytes))) return rc;
    RTX_HIP(rocprim::exclusive_scan(ix->d_text_tmp.p, tmp_bytes, ix->d_text_len.p, ix->d_text_off.p, 0ull, nq + 1, rocprim::plus<unsigned long long>(), s));
    if ((rc = hoff.resize(nq + 1))) return rc;
    RTX_HIP(hipMemcpyAsync(hoff.data(), ix->d_text_off.p, (nq + 1) * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    const uint64_t total = hoff[nq];
    if ((rc = ix->d_text.alloc(total + total / 4 + 64)) || (rc = hv.resize(total))) return rc;  // (grows: the next batch's text is about as long)
    p.off = ix->d_text_off.p;
    p.text = ix->d_text.p;
    p.cap = ix->d_text.n;
    hipLaunchKernelGGL(text_write_kernel, dim3((unsigned)((nq + kTextWaves - 1u) / kTextWaves)), dim3(kTextWaves * 64), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipMemcpyAsync(hv.data(), ix->d_text.p, total, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    return RTX_OK;
}

// The text of the batch being downloaded, from the final rows of its result set r, its input set (labels, bases, the ids passed in) and, if
// the device looked them up, the groups of its exact matches.  Synchronous: the input set is free for the next rtx_batch_prefetch when it
// returns.  Nothing happens without rtx_index_text_setup or without labels.
int enqueue_text(rtx_index *ix, const rtx_index::ResultSet &r) {
    const rtx_index::Inputs &in = ix->in[r.in_set];
    const uint64_t nq = r.n_q;
    rtx_index::HostText &ht = ix->host_text[ix->res_set];
    ht.valid = false;
    if (!ix->text_on || !in.has_labels || in.n_labels != nq) return RTX_OK;
    if (r.n_user != r.n_q) return RTX_OK;  // RTX_OPT_STRAND: no device text (the host formats the chosen orientation)
    TextParams p{};
    p.src = TextSrc{ix->d_lin_bytes.p, ix->d_lin_off.p, ix->d_lin_depth.p, r.d_fin_lineage.p, r.d_fin_depth8.p, r.d_fin_hund.p,
                    r.d_fin_local.p, ix->fin_D};
    p.nq = nq;
    p.status = r.d_fin_status.p;
    p.row_begin = r.d_fin_row_begin.p;
    p.row_count = r.d_fin_row_count.p;
    p.gs = r.d_fin_gs.p;
    p.labels = in.d_labels.p;
    p.label_off = in.d_label_off.p;
    p.grp = r.dev_exact ? r.d_exact_grp.p : nullptr;
    p.goff = ix->d_em_goff.p;
    p.gids = ix->d_em_gids.p;
    p.ex_off = in.d_exact_off.p;
    p.ex_ids = in.d_exact_ids.p;
    p.override_ok = !(ix->text_flags & (RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE));
    p.bases = in.d_packed.p;
    p.base_off = in.d_base_off.p;
    p.packed = in.packed;
    hipStream_t s = ix->copy_stream ? ix->copy_stream : ix->stream;
    int rc;
    p.tsv = false;
    if ((rc = text_pass(ix, p, s, ht.out, ht.out_off))) return rc;
    if (ix->text_flags & RTX_TEXT_TSV) {
        p.tsv = true;
        if ((rc = text_pass(ix, p, s, ht.tsv, ht.tsv_off))) return rc;
    }
    ht.tsv_on = (ix->text_flags & RTX_TEXT_TSV) != 0u;
    ht.nq = nq;
    ht.valid = true;
    return RTX_OK;
}

}  // namespace rtxi

extern "C" {

int rtx_index_text_setup(rtx_index *ix, const rtx_tree *tree, uint32_t flags) {
    int rc = bind(ix);
    if (rc) return rc;
    if (flags & ~(RTX_SKIP_EXACT_MATCHES | RTX_RAW_CONFIDENCE | RTX_TEXT_TSV)) { set_error("rtx_index_text_setup: unknown flags %#x", flags); return RTX_ERR_INVALID; }
    if (!tree) {
        ix->text_on = false;
        ix->text_tree_uid = 0;
        ix->d_lin_bytes.release(); ix->d_lin_off.release(); ix->d_lin_depth.release();
        ix->d_text.release(); ix->d_text_len.release(); ix->d_text_off.release(); ix->d_text_tmp.release();
        return RTX_OK;
    }
    const uint64_t n = tree->lineages.size();
    if (n != ix->n_total) { set_error("rtx_index_text_setup: the tree has %llu tips, the handle's database %llu", (unsigned long long)n, (unsigned long long)ix->n_total); return RTX_ERR_INVALID; }
    if (ix->text_tree_uid != tree->uid || !ix->d_lin_off.p) {  // the lineage table, once per tree
        std::vector<uint64_t> off(n + 1, 0);
        std::vector<uint8_t> depth(n);
        for (uint64_t i = 0; i < n; i++) {
            const std::string &l = tree->lineages[i];
            off[i + 1] = off[i] + l.size();
            const uint64_t d = 1 + (uint64_t)std::count(l.begin(), l.end(), ',');
            if (d > RTX_MAX_DEPTH) { set_error("lineage deeper than RTX_MAX_DEPTH: %s", l.c_str()); return RTX_ERR_DEPTH; }
            depth[i] = (uint8_t)d;
        }
        std::vector<char> bytes(off[n] + 1);
        for (uint64_t i = 0; i < n; i++) std::memcpy(bytes.data() + off[i], tree->lineages[i].data(), tree->lineages[i].size());
        if ((rc = ix->d_lin_bytes.alloc(bytes.size())) || (rc = ix->d_lin_off.alloc(n + 1)) || (rc = ix->d_lin_depth.alloc(n))) return rc;
        RTX_HIP(hipMemcpy(ix->d_lin_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
        RTX_HIP(hipMemcpy(ix->d_lin_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice));
        RTX_HIP(hipMemcpy(ix->d_lin_depth.p, depth.data(), n, hipMemcpyHostToDevice));
        ix->text_tree_uid = tree->uid;
    }
    ix->text_flags = flags;
    ix->text_on = true;
    return RTX_OK;
}

int rtx_batch_prefetch_labels(rtx_index *ix, uint64_t n_queries, const char *const *labels) {
    int rc = bind(ix);
    if (rc) return rc;
    if (!labels && n_queries) { set_error("rtx_batch_prefetch_labels: null labels"); return RTX_ERR_INVALID; }
    rtx_index::Inputs &in = ix->in[ix->cur_in ^ 1u];
    if (!ix->h2d_stream) RTX_HIP(hipStreamCreateWithFlags(&ix->h2d_stream, hipStreamNonBlocking));
    if (!in.ready) RTX_HIP(hipEventCreateWithFlags(&in.ready, hipEventDisableTiming));
    if (in.recorded) RTX_HIP(hipEventSynchronize(in.ready));  // the last transfer out of this set's pinned buffers
    if (ix->ev_activated) RTX_HIP(hipStreamWaitEvent(ix->h2d_stream, ix->ev_activated, 0));
    if ((rc = in.h_label_off.resize(n_queries + 1))) return rc;
    in.h_label_off[0] = 0;
    for (uint64_t q = 0; q < n_queries; q++) {
        if (!labels[q]) { set_error("rtx_batch_prefetch_labels: label %llu is null", (unsigned long long)q); return RTX_ERR_INVALID; }
        in.h_label_off[q + 1] = in.h_label_off[q] + std::strlen(labels[q]);
    }
    const uint64_t total = in.h_label_off[n_queries];
    if ((rc = in.h_labels.resize(total + 1)) || (rc = in.d_labels.alloc(total + 1)) || (rc = in.d_label_off.alloc(n_queries + 1))) return rc;
    for (uint64_t q = 0; q < n_queries; q++) std::memcpy(in.h_labels.data() + in.h_label_off[q], labels[q], in.h_label_off[q + 1] - in.h_label_off[q]);
    RTX_HIP(hipMemcpyAsync(in.d_labels.p, in.h_labels.data(), total + 1, hipMemcpyHostToDevice, ix->h2d_stream));
    RTX_HIP(hipMemcpyAsync(in.d_label_off.p, in.h_label_off.data(), (n_queries + 1) * 8, hipMemcpyHostToDevice, ix->h2d_stream));
    RTX_HIP(hipEventRecord(in.ready, ix->h2d_stream));
    in.recorded = true;
    in.labels_pending = true;
    in.n_labels = n_queries;
    return RTX_OK;
}

int rtx_batch_text(rtx_index *ix, rtx_text_view *out) {
    if (!ix || !out) { set_error("rtx_batch_text: null argument"); return RTX_ERR_INVALID; }
    const rtx_index::HostText &ht = ix->host_text[ix->res_set];
    if (!ht.valid && ix->host_res[ix->res_set].both) { set_error("rtx_batch_text: no device text under RTX_OPT_STRAND (format the view on the host: rtx_format_query)"); return RTX_ERR_STATE; }
    if (!ht.valid) { set_error("rtx_batch_text: the last download has no text (rtx_index_text_setup, then labels with the batch: rtx_batch_prefetch_labels)"); return RTX_ERR_STATE; }
    out->n_queries = ht.nq;
    out->out = ht.out.data();
    out->out_off = ht.out_off.data();
    out->tsv = ht.tsv_on ? ht.tsv.data() : nullptr;
    out->tsv_off = ht.tsv_on ? ht.tsv_off.data() : nullptr;
    return RTX_OK;
}

}  // extern "C"

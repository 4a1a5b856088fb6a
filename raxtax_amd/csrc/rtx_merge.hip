// Paired-end merging on the device (rtx_merge_*): the two mates of every pair overlapped into one read, before anything else of an amplicon
// pipeline runs (include/raxtax_hip.h has the exact semantics; rtx_math.hpp the arithmetic, shared with rtx_merge_pair on the host and the x86
// emulator).  Like rtx_trim, rtx_derep and rtx_qual an object of its own with one stream and its own buffers, so that the reader of the CLI can
// merge block b + 1 while the handles classify block b.
//
// The mates travel as they are given: one byte per base code and one quality byte per base, forward and reverse, with the callers' offsets --
// the host's staging is one copy of the four arrays into pinned memory that also ORs the quality bytes together (a byte of 128 or more is
// refused).  The merged read of pair i goes into a slot of (nf + nr rounded up to 16) bytes whose offset is known before the launch: one launch,
// no scan in between.
//   merge_kernel  one wave per pair, four pairs per block of 256, nothing shared between the waves: no block barrier.  The wave stages F and the
//                 reverse complement R' as nibble words and the two quality strings as bytes in LDS (merge_stage4: a lane builds four bases of
//                 an array per step; R is read backwards, the complement taken on the way in; 3104 bytes per pair), its lanes OR the bad-byte
//                 flag.  A mate that is too long is only streamed for that flag.  Candidates are dealt over the lanes, lane l takes
//                 ov = min_overlap + l + 64 j (merge_candidate: ceil(ov / 16) words, each one unaligned 16-nibble read of F, an aligned one of
//                 R', an AND and a zero-nibble count; left as soon as d > max_diffs); the best key per lane, a maximum over the wave
//                 (rtx_wave.hpp: DPP, no atomics); then all 64 lanes write the merged codes and quality bytes, lane l position l + 64 k
//                 (merge_base_at).  Lane 0 stores overlap, diffs, verdict and the merged length.  Vector stores and plain C++.
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"
#include "host_merge.hpp"

namespace {

struct MergeParams {
    const uint8_t *f_bases, *f_quals, *r_bases, *r_quals;  // the mates as given
    const uint64_t *f_off, *r_off, *slot_off;              // [n + 1] each
    uint8_t *m_bases, *m_quals;                            // the slots
    uint32_t *overlap, *diffs, *verdict, *merged_len;      // [n]
    uint32_t n;
    MergeCfg cfg;
};

constexpr uint32_t kMergeWaves = 4u;  // pairs of a block

__global__ __launch_bounds__(256) void merge_kernel(MergeParams p) {
    __shared__ __attribute__((aligned(16))) uint64_t s_wf[kMergeWaves][kMergeWords], s_wr[kMergeWaves][kMergeWords];
    __shared__ __attribute__((aligned(16))) uint8_t s_qf[kMergeWaves][kMergeMaxRead], s_qr[kMergeWaves][kMergeMaxRead];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kMergeWaves + wave;
    if (i >= p.n) return;  // (the whole wave; there is no block barrier)
    const uint64_t f_at = p.f_off[i], r_at = p.r_off[i], len_f = p.f_off[i + 1] - f_at, len_r = p.r_off[i + 1] - r_at;
    const uint32_t nf = (uint32_t)len_f, nr = (uint32_t)len_r;  // (below 2^32: rtx_merge_run)
    const bool fits = nf <= kMergeMaxRead && nr <= kMergeMaxRead;
    const uint64_t *wf = s_wf[wave], *wr = s_wr[wave];
    const uint8_t *qf = s_qf[wave], *qr = s_qr[wave];
    bool bad = false;
#pragma unroll
    for (uint32_t side = 0; side < 2u; side++) {
        const uint8_t *codes = side ? p.r_bases + r_at : p.f_bases + f_at, *quals = side ? p.r_quals + r_at : p.f_quals + f_at;
        const uint32_t n = side ? nr : nf;
        if (fits) {
            uint16_t *words = reinterpret_cast<uint16_t *>(side ? s_wr[wave] : s_wf[wave]);
            uint32_t *qs = reinterpret_cast<uint32_t *>(side ? s_qr[wave] : s_qf[wave]);
            for (uint32_t h = lane; 4u * h < n; h += 64u) {  // (h < 256: inside the arrays)
                uint32_t nib16, q32;
                bool b;
                merge_stage4(p.cfg, [codes](uint32_t k) { return (uint32_t)codes[k]; }, [quals](uint32_t k) { return (uint32_t)quals[k]; }, n, side == 1u, h, nib16, q32, b);
                words[h] = (uint16_t)nib16;
                qs[h] = q32;
                bad = bad || b;
            }
        } else {
            for (uint32_t k = lane; k < n; k += 64u) bad = bad || merge_bad_byte(p.cfg, quals[k]);
        }
    }
    uint32_t verdict = merge_pre_verdict(p.cfg, __ballot(bad) != 0ull, nf, nr), ov = 0, d = 0, mlen = 0;
    if (verdict == 0u) {  // (the same in every lane)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the staged words and bytes of the other lanes
        __builtin_amdgcn_wave_barrier();
        auto word_f = [wf](uint32_t w) { return wf[w]; };
        auto word_r = [wr](uint32_t w) { return wr[w]; };
        const uint32_t most = nf < nr ? nf : nr;
        uint32_t best = 0;
        for (uint32_t c = p.cfg.min_overlap + lane; c <= most; c += kMergeStride) {
            const uint32_t k = merge_candidate(p.cfg, word_f, word_r, nf, c);
            best = k > best ? k : best;
        }
        best = rtx::wave_max_u32(best);
        if (best == 0u) {
            verdict = kMgNoOverlap;
        } else {
            merge_key_read(best, ov, d);
            mlen = nf + nr - ov;
            uint8_t *mb = p.m_bases + p.slot_off[i], *mq = p.m_quals + p.slot_off[i];  // (mlen <= nf + nr <= the slot)
            for (uint32_t at = lane; at < mlen; at += 64u) {
                uint32_t code, byte;
                merge_base_at(p.cfg, word_f, word_r, [qf](uint32_t k) { return (uint32_t)qf[k]; }, [qr](uint32_t k) { return (uint32_t)qr[k]; }, nf, ov, at, code, byte);
                mb[at] = (uint8_t)code;
                mq[at] = (uint8_t)byte;
            }
        }
    }
    if (lane == 0u) {
        p.overlap[i] = ov;
        p.diffs[i] = d;
        p.verdict[i] = verdict;
        p.merged_len[i] = mlen;
    }
}

}  // namespace

struct rtx_merge : StageShell {
    rtx_merge_params params{};
    MergeCfg cfg{};
    DevBuf<uint8_t> d_in, d_out;              // F bases | F quals | R bases | R quals; merged bases | merged quals
    DevBuf<uint64_t> d_off;                   // f_off | r_off | slot_off
    DevBuf<uint32_t> d_res;                   // overlap | diffs | verdict | merged_len
    PinBuf<uint8_t> h_in;
    PinBuf<uint64_t> h_off;
    PinBuf<uint32_t> h_res;
};

extern "C" {

int rtx_merge_create(int device, const rtx_merge_params *params, rtx_merge **out) {
    if (!out || !params) { set_error("rtx_merge_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (const int rc = rtx::merge_check_params("rtx_merge_create", params)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto m = new rtx_merge();
    m->params = *params;
    rtx::merge_cfg_init(m->cfg, *params);
    if (const int rc = m->open(device)) { delete m; return rc; }
    *out = m;
    return RTX_OK;
}

void rtx_merge_destroy(rtx_merge *m) { destroy(m); }

int rtx_merge_run(rtx_merge *m, uint64_t n, const uint8_t *f_bases, const uint8_t *f_quals, const uint64_t *f_off, const uint8_t *r_bases,
                  const uint8_t *r_quals, const uint64_t *r_off, uint32_t *overlap, uint32_t *diffs, uint32_t *verdict, uint32_t *merged_len,
                  uint64_t *slot_off, uint8_t *merged_bases, uint8_t *merged_quals, uint64_t slot_cap) {
    if (!m) { set_error("rtx_merge_run: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) {
        if (slot_off) slot_off[0] = 0;
        return RTX_OK;
    }
    if (n > 0x7FFFFFF0ull) { set_error("rtx_merge_run: %llu pairs in one batch (at most 2^31 - 16)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!f_off || !r_off || !overlap || !diffs || !verdict || !merged_len || !slot_off) { set_error("rtx_merge_run: null argument"); return RTX_ERR_INVALID; }
    m->begin();
    int rc;
    if ((rc = m->h_off.resize(3 * (n + 1)))) return rc;
    uint64_t *hf = m->h_off.data(), *hr = hf + n + 1, *hs = hr + n + 1;
    hs[0] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (f_off[i + 1] < f_off[i] || r_off[i + 1] < r_off[i]) { set_error("base_off not monotone at pair %llu", (unsigned long long)i); return RTX_ERR_INVALID; }
        const uint64_t nf = f_off[i + 1] - f_off[i], nr = r_off[i + 1] - r_off[i];
        if (nf > 0x7FFFFFFFull || nr > 0x7FFFFFFFull) { set_error("rtx_merge_run: a mate of pair %llu has 2^31 bases or more", (unsigned long long)i); return RTX_ERR_INVALID; }
        hf[i] = f_off[i] - f_off[0];
        hr[i] = r_off[i] - r_off[0];
        hs[i + 1] = hs[i] + ((nf + nr + 15u) & ~15ull);
    }
    const uint64_t bf = f_off[n] - f_off[0], br = r_off[n] - r_off[0], slots = hs[n];
    hf[n] = bf;
    hr[n] = br;
    if ((bf && (!f_bases || !f_quals)) || (br && (!r_bases || !r_quals))) { set_error("rtx_merge_run: null bases or quals"); return RTX_ERR_INVALID; }
    if (slots > slot_cap || (slots && (!merged_bases || !merged_quals))) {
        set_error("rtx_merge_run: the slots of the batch take %llu bytes, %llu are given", (unsigned long long)slots, (unsigned long long)slot_cap);
        return RTX_ERR_INVALID;
    }
    RTX_HIP(hipSetDevice(m->device));
    const size_t in_bytes = 2 * (size_t)(bf + br);
    if ((rc = m->h_in.resize(in_bytes + 16)) || (rc = m->h_res.resize(4 * n)) || (rc = grow(m->d_in, in_bytes + 16)) || (rc = grow(m->d_out, 2 * (size_t)slots + 16)) ||
        (rc = grow(m->d_off, 3 * (n + 1))) || (rc = grow(m->d_res, 4 * n)))
        return rc;
    // staging: the four arrays into pinned memory, the quality bytes ORed together on the way
    uint8_t *hb = m->h_in.data();
    const uint8_t *src[4] = {f_bases + (bf ? f_off[0] : 0), f_quals + (bf ? f_off[0] : 0), r_bases + (br ? r_off[0] : 0), r_quals + (br ? r_off[0] : 0)};
    const uint64_t cnt[4] = {bf, bf, br, br}, dst[4] = {0, bf, 2 * bf, 2 * bf + br};
    const unsigned nt = std::max(1u, (unsigned)std::min<uint64_t>(rtx::host_threads(4u), (in_bytes + (1u << 22) - 1) >> 22));
    std::vector<uint8_t> seen(nt, 0);
    rtx::parallel_ranges(nt, nt, 1, [&](unsigned k, uint64_t, uint64_t) {  // (the split is by bytes: thread k takes its share of each array)
        uint8_t s = 0;
        for (int a = 0; a < 4; a++) {
            const uint64_t lo = cnt[a] * k / nt, hi = cnt[a] * (k + 1) / nt;
            if (hi == lo) continue;
            memcpy(hb + dst[a] + lo, src[a] + lo, hi - lo);
            if (a & 1)
                for (uint64_t j = lo; j < hi; j++) s |= src[a][j];
        }
        seen[k] = s;
    });
    for (uint8_t s : seen)
        if (s & 0x80u) { set_error("rtx_merge_run: a quality byte of 128 or more"); return RTX_ERR_INVALID; }
    m->staged();
    hipStream_t s = m->stream;
    if (in_bytes) RTX_HIP(hipMemcpyAsync(m->d_in.p, hb, in_bytes, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(m->d_off.p, hf, 3 * (n + 1) * 8, hipMemcpyHostToDevice, s));
    MergeParams p{};
    p.f_bases = m->d_in.p;
    p.f_quals = m->d_in.p + bf;
    p.r_bases = m->d_in.p + 2 * bf;
    p.r_quals = m->d_in.p + 2 * bf + br;
    p.f_off = m->d_off.p;
    p.r_off = m->d_off.p + (n + 1);
    p.slot_off = m->d_off.p + 2 * (n + 1);
    p.m_bases = m->d_out.p;
    p.m_quals = m->d_out.p + slots;
    p.overlap = m->d_res.p;
    p.diffs = m->d_res.p + n;
    p.verdict = m->d_res.p + 2 * n;
    p.merged_len = m->d_res.p + 3 * n;
    p.n = (uint32_t)n;
    p.cfg = m->cfg;
    RTX_HIP(hipEventRecord(m->ev0, s));
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((n + kMergeWaves - 1u) / kMergeWaves)), dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipEventRecord(m->ev1, s));
    RTX_HIP(hipMemcpyAsync(m->h_res.data(), m->d_res.p, 4 * n * 4, hipMemcpyDeviceToHost, s));
    if (slots) {  // (what lies in a slot behind its merged read is not defined)
        RTX_HIP(hipMemcpyAsync(merged_bases, m->d_out.p, slots, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipMemcpyAsync(merged_quals, m->d_out.p + slots, slots, hipMemcpyDeviceToHost, s));
    }
    if ((rc = m->wait())) return rc;
    scatter_columns(m->h_res.data(), n, {overlap, diffs, verdict, merged_len});
    std::memcpy(slot_off, hs, (n + 1) * 8);
    m->finish();
    return RTX_OK;
}

int rtx_merge_kernel_time(const rtx_merge *m, float *ms) { return kernel_time("rtx_merge_kernel_time", m, ms); }

int rtx_merge_stage_times(const rtx_merge *m, double seconds[3]) { return stage_times("rtx_merge_stage_times", m, seconds); }

int rtx_merge_queries(rtx_merge *m, const rtx_queries *fwd, const rtx_queries *rev, const char *const *skip, uint64_t n_skip, rtx_queries **merged) {
    if (!fwd || !rev || !merged || (n_skip && !skip)) { set_error("rtx_merge_queries: null argument"); return RTX_ERR_INVALID; }
    *merged = nullptr;
    if (!fwd->fastq || !rev->fastq) { set_error("rtx_merge_queries: both handles must come from a FASTQ parse"); return RTX_ERR_INVALID; }
    const uint64_t n = fwd->labels.size();
    if (rev->labels.size() != n) {
        set_error("paired FASTQ: %llu forward and %llu reverse records", (unsigned long long)n, (unsigned long long)rev->labels.size());
        return RTX_ERR_PARSE;
    }
    for (uint64_t i = 0; i < n; i++) {
        const char *a, *b;
        uint64_t la, lb;
        rtx::merge_label_key(fwd->labels[i].c_str(), 1, a, la);
        rtx::merge_label_key(rev->labels[i].c_str(), 2, b, lb);
        if (la != lb || memcmp(a, b, la) != 0) {
            set_error("paired FASTQ pair %llu: the labels '%s' and '%s' do not pair", (unsigned long long)i + 1, fwd->labels[i].c_str(), rev->labels[i].c_str());
            return RTX_ERR_PARSE;
        }
    }
    if (!m) { set_error("rtx_merge_queries: null argument"); return RTX_ERR_INVALID; }  // (behind the pairing: that needs no device)
    try {
        std::vector<uint32_t> res(4 * std::max<uint64_t>(n, 1));
        std::vector<uint64_t> slot(n + 1, 0);
        uint64_t cap = 0;
        for (uint64_t i = 0; i < n; i++)
            cap += ((fwd->base_off[i + 1] - fwd->base_off[i]) + (rev->base_off[i + 1] - rev->base_off[i]) + 15u) & ~15ull;
        std::vector<uint8_t> mb(cap + 1), mq(cap + 1);
        if (const int rc = rtx_merge_run(m, n, fwd->bases.data(), fwd->quals.data(), fwd->base_off.data(), rev->bases.data(), rev->quals.data(), rev->base_off.data(),
                                         res.data(), res.data() + n, res.data() + 2 * n, res.data() + 3 * n, slot.data(), mb.data(), mq.data(), cap))
            return rc;
        std::unordered_map<std::string_view, int> skipset;
        for (uint64_t i = 0; i < n_skip; i++) skipset.emplace(skip[i], 1);
        auto q = new rtx_queries();
        q->fastq = true;
        q->merged = true;
        q->quals.reserve(1);
        for (uint64_t i = 0; i < n; i++) {
            if (skipset.count(fwd->labels[i])) continue;
            const uint32_t len = res[3 * n + i];
            q->labels.push_back(fwd->labels[i]);
            q->bases.insert(q->bases.end(), mb.begin() + slot[i], mb.begin() + slot[i] + len);
            q->quals.insert(q->quals.end(), mq.begin() + slot[i], mq.begin() + slot[i] + len);
            q->base_off.push_back(q->bases.size());
            q->mg_nf.push_back((uint32_t)(fwd->base_off[i + 1] - fwd->base_off[i]));
            q->mg_nr.push_back((uint32_t)(rev->base_off[i + 1] - rev->base_off[i]));
            q->mg_overlap.push_back(res[i]);
            q->mg_diffs.push_back(res[n + i]);
            q->mg_verdict.push_back(res[2 * n + i]);
        }
        *merged = q;
        return RTX_OK;
    } catch (const std::bad_alloc &) {
        set_error("out of host memory");
        return RTX_ERR_OOM;
    }
}

int rtx_queries_merge_report(const rtx_queries *merged, const uint32_t **nf, const uint32_t **nr, const uint32_t **overlap, const uint32_t **diffs,
                             const uint32_t **verdict) {
    if (!merged || !nf || !nr || !overlap || !diffs || !verdict) { set_error("rtx_queries_merge_report: null argument"); return RTX_ERR_INVALID; }
    if (!merged->merged) { set_error("rtx_queries_merge_report: the handle does not come from rtx_merge_queries"); return RTX_ERR_STATE; }
    *nf = merged->mg_nf.data();
    *nr = merged->mg_nr.data();
    *overlap = merged->mg_overlap.data();
    *diffs = merged->mg_diffs.data();
    *verdict = merged->mg_verdict.data();
    return RTX_OK;
}

}  // extern "C"

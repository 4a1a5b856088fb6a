// Paired-end merging on the host (include/raxtax_hip.h): the checks of a parameter struct, the pairing rule of two labels, rtx_merge_pair --
// one pair with the staging, candidate and consensus functions merge_kernel runs (rtx_math.hpp), the candidates one after the other -- and
// rtx_fastq_block_end_n, which cuts two FASTQ files that are read piecewise at the same record.  No device involved: tests pin the definition
// with it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <cstring>

#include "host_merge.hpp"
#include "rtx_internal.hpp"
#include "rtx_math.hpp"

namespace rtx {

int merge_check_params(const char *who, const rtx_merge_params *p) {
    if (!p) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (p->ascii_base != 33u && p->ascii_base != 64u) { set_error("%s: ascii_base %u (33 or 64)", who, p->ascii_base); return RTX_ERR_INVALID; }
    if (p->min_overlap == 0u) { set_error("%s: min_overlap 0 (at least 1)", who); return RTX_ERR_INVALID; }
    if (p->max_diff_pct > 100u) { set_error("%s: max_diff_pct %u (0 .. 100)", who, p->max_diff_pct); return RTX_ERR_INVALID; }
    if (p->q_cap > kQualMaxQ) { set_error("%s: q_cap %u (at most %u)", who, p->q_cap, kQualMaxQ); return RTX_ERR_INVALID; }
    return RTX_OK;
}

void merge_cfg_init(MergeCfg &c, const rtx_merge_params &p) {
    c.base = p.ascii_base;
    c.min_overlap = p.min_overlap;
    c.max_diffs = p.max_diffs;
    c.max_diff_pct = p.max_diff_pct;
    c.q_cap = p.q_cap;
}

void merge_label_key(const char *label, int mate, const char *&begin, uint64_t &len) {
    begin = label;
    len = 0;
    while (label[len] && label[len] != ' ' && label[len] != '\t') len++;
    if (len >= 2 && label[len - 2] == '/' && label[len - 1] == (mate == 1 ? '1' : '2')) len -= 2;
}

}  // namespace rtx

extern "C" uint64_t rtx_fastq_block_end_n(const char *text, uint64_t len, uint64_t max_records, uint64_t *n_records) {
    uint64_t lines = 0, end = 0, pos = 0, recs = 0;
    const void *nl;
    while (text && recs < max_records && pos < len && (nl = memchr(text + pos, '\n', len - pos)) != nullptr) {
        pos = (uint64_t)((const char *)nl - text) + 1;
        if ((++lines & 3u) == 0) { end = pos; recs++; }
    }
    if (n_records) *n_records = recs;
    return end;
}

extern "C" int rtx_merge_pair(const rtx_merge_params *params, const uint8_t *f_bases, const uint8_t *f_quals, uint32_t nf, const uint8_t *r_bases,
                              const uint8_t *r_quals, uint32_t nr, uint32_t *overlap, uint32_t *diffs, uint32_t *verdict, uint32_t *merged_len,
                              uint8_t *merged_bases, uint8_t *merged_quals) {
    using namespace rtx;
    if (!overlap || !diffs || !verdict || !merged_len || (nf && (!f_bases || !f_quals)) || (nr && (!r_bases || !r_quals))) { set_error("rtx_merge_pair: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = merge_check_params("rtx_merge_pair", params)) return rc;
    MergeCfg cfg;
    merge_cfg_init(cfg, *params);
    bool bad = false;
    uint8_t seen = 0;
    for (uint32_t i = 0; i < nf; i++) { seen |= f_quals[i]; bad = bad || merge_bad_byte(cfg, f_quals[i]); }
    for (uint32_t i = 0; i < nr; i++) { seen |= r_quals[i]; bad = bad || merge_bad_byte(cfg, r_quals[i]); }
    if (seen & 0x80u) { set_error("rtx_merge_pair: a quality byte of 128 or more"); return RTX_ERR_INVALID; }
    *overlap = *diffs = *merged_len = 0u;
    *verdict = merge_pre_verdict(cfg, bad, nf, nr);
    if (*verdict) return RTX_OK;
    uint64_t wf[kMergeWords], wr[kMergeWords];
    uint8_t qf[kMergeMaxRead], qr[kMergeMaxRead];
    memset(wf, 0, sizeof wf);
    memset(wr, 0, sizeof wr);
    memset(qf, 0, sizeof qf);
    memset(qr, 0, sizeof qr);
    for (int side = 0; side < 2; side++) {
        const uint8_t *codes = side ? r_bases : f_bases, *quals = side ? r_quals : f_quals;
        const uint32_t n = side ? nr : nf;
        uint64_t *words = side ? wr : wf;
        uint8_t *qs = side ? qr : qf;
        for (uint32_t h = 0; 4u * h < n; h++) {
            uint32_t nib16, q32;
            bool b;
            merge_stage4(cfg, [codes](uint32_t i) { return (uint32_t)codes[i]; }, [quals](uint32_t i) { return (uint32_t)quals[i]; }, n, side == 1, h, nib16, q32, b);
            words[h >> 2] |= (uint64_t)nib16 << (16u * (h & 3u));
            memcpy(qs + 4u * h, &q32, 4);  // (little-endian, as the device stores the four bytes)
        }
    }
    auto word_f = [&wf](uint32_t w) { return wf[w]; };
    auto word_r = [&wr](uint32_t w) { return wr[w]; };
    const uint32_t best = merge_best_serial(cfg, word_f, word_r, nf, nr);
    if (!best) { *verdict = kMgNoOverlap; return RTX_OK; }
    if (!merged_bases || !merged_quals) { set_error("rtx_merge_pair: null argument"); return RTX_ERR_INVALID; }
    merge_key_read(best, *overlap, *diffs);
    *merged_len = nf + nr - *overlap;
    for (uint32_t p = 0; p < *merged_len; p++) {
        uint32_t code, byte;
        merge_base_at(cfg, word_f, word_r, [&qf](uint32_t i) { return (uint32_t)qf[i]; }, [&qr](uint32_t i) { return (uint32_t)qr[i]; }, nf, *overlap, p, code, byte);
        merged_bases[p] = (uint8_t)code;
        merged_quals[p] = (uint8_t)byte;
    }
    return RTX_OK;
}

// Quality filter on the host (include/raxtax_hip.h): the error table, the checks of a parameter struct and its integer form, and
// rtx_qual_read -- one read with the staging and the piece functions qual_kernel runs (rtx_math.hpp: qual_stage, qual_piece_sum,
// qual_piece_stop, qual_verdict).  No device involved: tests pin the definition with it.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (rtx_math.hpp: __forceinline__; the file also builds with a plain host compiler)
#endif
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "host_qual.hpp"
#include "rtx_internal.hpp"
#include "rtx_math.hpp"

namespace rtx {

const uint64_t *qual_table() {
    static uint64_t table[RTX_QUAL_TABLE];
    static std::once_flag once;
    std::call_once(once, [] {
        // 10^(-Q/10) * 2^40 in long double (64 bits of mantissa, the values have at most 41): the nearest integer
        for (int q = 0; q < RTX_QUAL_TABLE; q++) table[q] = (uint64_t)llroundl(powl(10.0L, -(long double)q / 10.0L) * 1099511627776.0L);
    });
    return table;
}

static bool qual_bad_double(double x) { return std::isnan(x); }

int qual_check_params(const char *who, const rtx_qual_params *p) {
    if (!p) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    if (p->ascii_base != 33u && p->ascii_base != 64u) { set_error("%s: ascii_base %u (33 or 64)", who, p->ascii_base); return RTX_ERR_INVALID; }
    if (p->trunc_qual > (int32_t)kQualMaxQ) { set_error("%s: trunc_qual %d (at most %u)", who, p->trunc_qual, kQualMaxQ); return RTX_ERR_INVALID; }
    if (qual_bad_double(p->trunc_ee) || qual_bad_double(p->max_ee) || qual_bad_double(p->max_ee_rate)) { set_error("%s: a threshold is not a number", who); return RTX_ERR_INVALID; }
    return RTX_OK;
}

bool qual_params_on(const rtx_qual_params &p) {
    return p.trunc_len != 0u || p.trunc_qual >= 0 || !(p.trunc_ee < 0) || p.min_len != 0u || p.max_len != 0u || p.max_ns >= 0 || !(p.max_ee < 0) || !(p.max_ee_rate < 0);
}

// (as the integers that are compared: -1 and -2 switch a field off alike)
bool qual_params_equal(const rtx_qual_params &a, const rtx_qual_params &b) {
    QualCfg x, y;
    qual_cfg_init(x, a);
    qual_cfg_init(y, b);
    return x.base == y.base && x.trunc_len == y.trunc_len && x.trunc_qual == y.trunc_qual && x.trunc_ee == y.trunc_ee && x.min_len == y.min_len &&
           x.max_len == y.max_len && x.max_ns == y.max_ns && x.max_ee == y.max_ee && x.max_ee_rate == y.max_ee_rate;
}

// floor(x * 2^40), at most 2^63; off below 0.  (x * 2^40 is exact in a double unless it overflows, and then it is above 2^63.)
static uint64_t qual_threshold(double x) {
    if (x < 0) return kQualOff;
    const double v = std::floor(std::ldexp(x, 40));
    return v >= 9223372036854775808.0 ? (1ull << 63) : (uint64_t)v;
}

void qual_cfg_init(QualCfg &c, const rtx_qual_params &p) {
    c.base = p.ascii_base;
    c.trunc_len = p.trunc_len;
    c.trunc_qual = p.trunc_qual < 0 ? -1 : p.trunc_qual;
    c.trunc_ee = qual_threshold(p.trunc_ee);
    c.min_len = p.min_len;
    c.max_len = p.max_len;
    c.max_ns = p.max_ns < 0 ? -1 : p.max_ns;
    c.max_ee = qual_threshold(p.max_ee);
    c.max_ee_rate = qual_threshold(p.max_ee_rate);
}

// dst[i] = quals[i] | 0x80 where bases[i] is none of 1, 2, 4, 8; the OR of the quality bytes comes back (bit 7: a byte of 128 or more)
uint8_t qual_stage(const uint8_t *bases, const uint8_t *quals, uint64_t n, uint8_t *dst) {
    uint8_t seen = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t b = bases[i];
        const uint8_t acgt = (uint8_t)((b == 1) | (b == 2) | (b == 4) | (b == 8));
        seen |= quals[i];
        dst[i] = (uint8_t)(quals[i] | (uint8_t)((acgt ^ 1u) << 7));
    }
    return seen;
}

}  // namespace rtx

extern "C" int rtx_qual_error_table(uint64_t out[RTX_QUAL_TABLE]) {
    if (!out) { rtx::set_error("rtx_qual_error_table: null argument"); return RTX_ERR_INVALID; }
    memcpy(out, rtx::qual_table(), sizeof(uint64_t) * RTX_QUAL_TABLE);
    return RTX_OK;
}

extern "C" int rtx_qual_read(const rtx_qual_params *params, const uint8_t *bases, const uint8_t *quals, uint64_t len, uint32_t lo, uint32_t hi_in,
                             uint32_t *hi_out, uint64_t *ee_out, uint32_t *verdict_out) {
    if (!hi_out || !ee_out || !verdict_out || (len && (!bases || !quals))) { rtx::set_error("rtx_qual_read: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::qual_check_params("rtx_qual_read", params)) return rc;
    if (len > RTX_QUAL_MAX_READ) { rtx::set_error("rtx_qual_read: a read of %llu bases (at most %u)", (unsigned long long)len, RTX_QUAL_MAX_READ); return RTX_ERR_INVALID; }
    if (lo > hi_in || hi_in > len) { rtx::set_error("rtx_qual_read: the range [%u, %u) of a read of %llu bases", lo, hi_in, (unsigned long long)len); return RTX_ERR_INVALID; }
    rtx::QualCfg cfg;
    rtx::qual_cfg_init(cfg, *params);
    const uint32_t n = hi_in - lo;
    std::vector<uint8_t> row((size_t)(n + 15u) / 16u * 16u + 16u, 0);
    if (n && (rtx::qual_stage(bases + lo, quals + lo, n, row.data()) & 0x80u)) { rtx::set_error("rtx_qual_read: a quality byte of 128 or more"); return RTX_ERR_INVALID; }
    auto load = [&row](uint32_t i) { rtx::QualWords t; memcpy(t.w, row.data() + 16u * (size_t)i, 16); return t; };
    uint32_t kept;
    rtx::qual_read_serial(cfg, rtx::qual_table(), load, n, kept, *ee_out, *verdict_out);
    *hi_out = lo + kept;
    return RTX_OK;
}

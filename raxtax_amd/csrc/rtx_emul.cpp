// Host-side emulation of the device arithmetic in rtx_math.hpp, for the CPU test-suite
// (tests/test_device_math_cpu.py).  TEST SUPPORT ONLY: it is not part of libraxtax_hip.so
// and never runs on the product path.  It executes the very same inline functions the HIP
// kernels call (bit-plane adders/unpack, pmf recurrence), sequentially on x86, so that
// their logic is checked against the oracle without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <array>
#include <vector>

#include "rtx_math.hpp"

using namespace rtx;

// Folds n_rows words (one 32-reference column; n_rows a multiple of 8) into NP planes by one of the kernels' schedules:
//   sched 32: hit_count_kernel / fold_ring<NB = 4> -- 32 rows = four tree8 + two CSAs on plane 3 + one on plane 4 + ripple from plane 5,
//             the rest eight at a time (planes_add8);
//   sched 24: hit_count_pair_kernel (fold_seg<NB = 3>, rtx_hit_pair.hip) -- 24 rows = three tree8, a CSA on plane 3 for the first two
//             carries, a half adder on plane 3 for the third, a CSA on plane 4, ripple from plane 5; the rows a list lacks for its last
//             group are the zero row, as the kernel pads its lists.
template <int NP>
static void emul_fold(uint32_t (&pl)[NP], const uint32_t *rows, uint32_t n_rows, int sched) {
    auto t8 = [&](const uint32_t *r) { return planes_tree8<NP>(pl, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]); };
    uint32_t r = 0;
    if (sched == 24) {
        std::vector<uint32_t> padded(rows, rows + n_rows);
        padded.resize((n_rows + 23u) / 24u * 24u, 0u);
        for (; r + 24 <= padded.size(); r += 24) {
            const uint32_t c3a = t8(&padded[r]), c3b = t8(&padded[r + 8]), c3c = t8(&padded[r + 16]);
            uint32_t c4a, c5;
            csa(pl[3], c3a, c3b, pl[3], c4a);
            const uint32_t c4b = pl[3] & c3c;  // half_plane (rtx_hit_common.hpp): a carry-save adder with one input 0
            pl[3] ^= c3c;
            csa(pl[4], c4a, c4b, pl[4], c5);
            planes_ripple<NP, 5>(pl, c5);
        }
        return;
    }
    for (; r + 32 <= n_rows; r += 32) {
        uint32_t c3a = t8(rows + r), c3b = t8(rows + r + 8), c4a, c4b, c5;
        csa(pl[3], c3a, c3b, pl[3], c4a);
        c3a = t8(rows + r + 16);
        c3b = t8(rows + r + 24);
        csa(pl[3], c3a, c3b, pl[3], c4b);
        csa(pl[4], c4a, c4b, pl[4], c5);
        planes_ripple<NP, 5>(pl, c5);
    }
    for (; r + 8 <= n_rows; r += 8)
        planes_add8<NP>(pl, rows[r], rows[r + 1], rows[r + 2], rows[r + 3], rows[r + 4], rows[r + 5], rows[r + 6], rows[r + 7]);
}

// the 32 counters of a word by planes_unpack4; the two other unpack forms of the epilogues must give the same (else the counter is
// poisoned: 0xFFFFFFFF planes_unpack8, 0xFFFFFFFE planes_unpack32 + planes_unpack8_hi)
template <int NP>
static void emul_unpack(const uint32_t (&pl)[NP], uint32_t *out) {
    for (int g = 0; g < 8; g++) {
        uint32_t lo, hi;
        planes_unpack4<NP>(pl, g, lo, hi);
        for (int j = 0; j < 4; j++) out[4 * g + j] = ((lo >> (8 * j)) & 0xFF) | (((hi >> (8 * j)) & 0xFF) << 8);
    }
    for (int b = 0; b < 4; b++) {
        uint32_t lo0, hi0, lo1, hi1;
        planes_unpack8<NP>(pl, b, lo0, hi0, lo1, hi1);
        for (int j = 0; j < 4; j++) {
            const uint32_t c0 = ((lo0 >> (8 * j)) & 0xFF) | (((hi0 >> (8 * j)) & 0xFF) << 8);
            const uint32_t c1 = ((lo1 >> (8 * j)) & 0xFF) | (((hi1 >> (8 * j)) & 0xFF) << 8);
            if (c0 != out[8 * b + j] || c1 != out[8 * b + 4 + j]) out[8 * b + j] = 0xFFFFFFFFu;  // poison: the test fails
        }
    }
    uint32_t lo[4][2];
    planes_unpack32<NP>(pl, lo);
    for (int b = 0; b < 4; b++) {
        uint32_t hi0, hi1;
        planes_unpack8_hi<NP>(pl, b, hi0, hi1);
        for (int j = 0; j < 4; j++) {
            const uint32_t c0 = ((lo[b][0] >> (8 * j)) & 0xFF) | (((hi0 >> (8 * j)) & 0xFF) << 8);
            const uint32_t c1 = ((lo[b][1] >> (8 * j)) & 0xFF) | (((hi1 >> (8 * j)) & 0xFF) << 8);
            if (c0 != out[8 * b + j] || c1 != out[8 * b + 4 + j]) out[8 * b + j] = 0xFFFFFFFEu;
        }
    }
}

template <typename F>
static int emul_with_planes(int planes, F &&f) {  // the plane counts the kernels are instantiated with
    switch (planes) {
        case 8: f(std::integral_constant<int, 8>{}); return 0;
        case 10: f(std::integral_constant<int, 10>{}); return 0;
        case 11: f(std::integral_constant<int, 11>{}); return 0;
        case 12: f(std::integral_constant<int, 12>{}); return 0;
        case 16: f(std::integral_constant<int, 16>{}); return 0;
    }
    return -1;
}

extern "C" {

void emul_merge_bytes(const uint32_t *sb, uint32_t *st);

// The arithmetic of the two-level bounds pass (rtx_bounds2.hip) on one 32-counter column: the rows are dealt to `groups` lane groups as the
// load instructions deal them (unit of 8 * groups rows: group g takes rows 8 g .. 8 g + 7 of the unit), every group folds its own (tree8 +
// ripple), the partial plane sets are added pairwise as bit-sliced numbers (the butterfly of reduce_rows) and the largest counter is taken on
// the planes.  n_rows must be a multiple of 8 * groups.  out: 32 counters; returns max << 8 | lowest counter that holds it.
uint32_t emul_planes_grouped(const uint32_t *rows, uint32_t n_rows, uint32_t groups, uint32_t *out) {
    constexpr int NP = 10;
    std::vector<std::array<uint32_t, NP>> part(groups);
    for (auto &p : part) p.fill(0);
    for (uint32_t u = 0; u + 8 * groups <= n_rows; u += 8 * groups)
        for (uint32_t g = 0; g < groups; g++) {
            const uint32_t *r = rows + u + 8 * g;
            uint32_t pl[NP];
            for (int p = 0; p < NP; p++) pl[p] = part[g][p];
            planes_ripple<NP, 3>(pl, planes_tree8<NP>(pl, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]));
            for (int p = 0; p < NP; p++) part[g][p] = pl[p];
        }
    for (uint32_t d = 1; d < groups; d <<= 1)  // butterfly: every group ends with the total
        for (uint32_t g = 0; g < groups; g++)
            if (!(g & d)) {
                uint32_t a[NP], b[NP];
                for (int p = 0; p < NP; p++) { a[p] = part[g][p]; b[p] = part[g | d][p]; }
                planes_add<NP>(a, b);
                for (int p = 0; p < NP; p++) part[g][p] = part[g | d][p] = a[p];
            }
    uint32_t tot[NP];
    for (int p = 0; p < NP; p++) tot[p] = part[groups - 1][p];
    for (int b = 0; b < 32; b++) {
        uint32_t c = 0;
        for (int p = 0; p < NP; p++) c |= ((tot[p] >> b) & 1u) << p;
        out[b] = c;
    }
    uint32_t cand;
    const uint32_t m = planes_max<NP>(tot, cand);
    return (m << 8) | (uint32_t)__builtin_ctz(cand);
}

// rows: n_rows x 1 words (one 32-reference column).  n_rows must be a multiple of 8; planes 8, 10, 11, 12 or 16; sched 32 or 24
// (emul_fold).  out: 32 counters.  Returns 0, or -1 for arguments it does not cover (out untouched).
int emul_planes_count_sched(const uint32_t *rows, uint32_t n_rows, int planes, int sched, uint32_t *out) {
    if ((n_rows & 7u) || (sched != 32 && sched != 24)) return -1;
    return emul_with_planes(planes, [&](auto tag) {
        constexpr int NP = decltype(tag)::value;
        uint32_t pl[NP];
        for (int p = 0; p < NP; p++) pl[p] = 0;
        emul_fold<NP>(pl, rows, n_rows, sched);
        emul_unpack<NP>(pl, out);
    });
}
void emul_planes_count(const uint32_t *rows, uint32_t n_rows, int planes, uint32_t *out) {
    emul_planes_count_sched(rows, n_rows, planes, 32, out);
}

// planes_gt on the planes that hold the 32 counters `counts` (each < 2^planes): bit r = counts[r] > c.  *mask; returns 0 / -1 as above.
int emul_planes_gt(const uint32_t *counts, int planes, uint32_t c, uint32_t *mask) {
    return emul_with_planes(planes, [&](auto tag) {
        constexpr int NP = decltype(tag)::value;
        uint32_t pl[NP];
        for (int p = 0; p < NP; p++) {
            pl[p] = 0;
            for (int r = 0; r < 32; r++) pl[p] |= ((counts[r] >> p) & 1u) << r;
        }
        *mask = planes_gt<NP>(pl, c);
    });
}

// The counts of one 32-reference word of a (query, tile) as kmer_extract and the epilogue of hit_count make them: of the rows flagged
// sparse the first kSegMaxSparseRows go through byte counters -- word-wide adds of 1 << 8 (r & 3), as the LDS atomics of sparse_hits:
// a 256th hit would carry into the neighbour's byte -- the rest and every dense row are folded into the planes (padded to eight with
// the zero row); then the merge: planes 8 the byte form of hit_epilogue_x (lo + sb, word-wide), else the SWAR merge (emul_merge_bytes).
int emul_tile_word_counts(const uint32_t *rows, const uint8_t *sparse, uint32_t n_rows, int planes, int sched, uint32_t *out) {
    uint32_t cnt8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint32_t> dense;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < n_rows; i++) {
        if (sparse[i] && ns < kSegMaxSparseRows) {
            ns++;
            for (uint32_t r = 0; r < 32; r++)
                if ((rows[i] >> r) & 1u) cnt8[r >> 2] += 1u << ((r & 3u) * 8u);
        } else {
            dense.push_back(rows[i]);
        }
    }
    dense.resize((dense.size() + 7u) / 8u * 8u, 0u);
    return emul_with_planes(planes, [&](auto tag) {
        constexpr int NP = decltype(tag)::value;
        uint32_t pl[NP];
        for (int p = 0; p < NP; p++) pl[p] = 0;
        emul_fold<NP>(pl, dense.data(), (uint32_t)dense.size(), sched);
        uint32_t lo[4][2];
        planes_unpack32<NP>(pl, lo);
        for (int b = 0; b < 4; b++) {  // references 8 b .. 8 b + 7: byte counters cnt8[2 b], cnt8[2 b + 1]
            if (NP <= 8) {
                const uint32_t w[2] = {lo[b][0] + cnt8[2 * b], lo[b][1] + cnt8[2 * b + 1]};
                for (int j = 0; j < 8; j++) out[8 * b + j] = (w[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
            } else {
                uint32_t hi0, hi1;
                planes_unpack8_hi<NP>(pl, b, hi0, hi1);
                uint32_t st[4] = {byte_perm(hi0, lo[b][0], 0x05010400u), byte_perm(hi0, lo[b][0], 0x07030602u),
                                  byte_perm(hi1, lo[b][1], 0x05010400u), byte_perm(hi1, lo[b][1], 0x07030602u)};
                emul_merge_bytes(&cnt8[2 * b], st);
                for (int j = 0; j < 8; j++) out[8 * b + j] = (st[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
            }
        }
    });
}

// Sequential emulation of prob_table_kernel (same lane grouping, pruning and arithmetic; only the
// order of the cross-lane sums differs).  hist has t+1 entries.  Returns 0, or 1 when the kernel
// would flag RTX_Q_NO_KMERS.  stats (may be null): [0] heavy group-steps, [1] light group-steps,
// [2] skipped groups, [3] i_lo.
int emul_prob_table(uint32_t t, const uint32_t *hist, uint64_t n_refs, const double *lf, double *table_z, double *z,
                    double *gs, uint64_t *stats) {
    const uint32_t n = t >> 1;
    if (t == 0) return 1;
    std::vector<uint32_t> ms;
    for (uint32_t m = 0; m <= t; m++)
        if (hist[m]) ms.push_back(m);
    const uint32_t D = (uint32_t)ms.size();
    std::vector<double> inv(t + n + 2, 0.0);
    for (uint32_t x = 1; x <= t + n; x++) inv[x] = 1.0 / (double)x;
    const double ln_total = ln_binom_tab(lf, t + n - 1, n);
    std::vector<double> tab(t + 1, 0.0);
    uint64_t st_heavy = 0, st_light = 0, st_skip = 0, st_ilo = 0;
    if (ms.back() == t) {
        for (uint32_t m : ms) tab[m] = only_last_pmf_tab(lf, t, n, m, ln_total);
    } else {
        if (n == 0) return 1;
        const uint32_t M = ms.back();
        uint32_t i_lo = 0;
        if (M > 0) {
            i_lo = n;
            for (uint32_t i = 0; i <= n; i++)
                if (ln_pmf_tab(lf, t, n, M, i, ln_total) >= kLnNegligibleP) { i_lo = i; break; }
        }
        st_ilo = i_lo;
        const uint32_t ngroups = (D + 63) / 64;  // lane groups (waves) in descending order of m
        std::vector<double> prod(n + 1, 1.0), Pi(n + 1, 0.0), base(ngroups, 1.0);
        std::vector<uint32_t> bw(ngroups, 0), istart(ngroups, 0);
        std::vector<uint8_t> skipped(ngroups, 0);
        for (uint32_t g = 0; g < ngroups; g++) {
            const uint32_t m_hi = ms[D - 1 - g * 64];
            if (m_hi == 0 || group_negligible(lf, t, n, m_hi, i_lo, ln_total)) {
                skipped[g] = 1;
                st_skip++;
                continue;
            }
            const uint32_t nl = std::min<uint32_t>(64, D - g * 64);
            // start index of the group: first i at which its smallest count's pmf reaches e^-100
            uint32_t m_lo = ms[D - 1 - (g * 64 + nl - 1)];
            if (m_lo == 0) m_lo = nl > 1 ? ms[D - 1 - (g * 64 + nl - 2)] : m_hi;
            uint32_t i_s = i_lo;
            for (uint32_t i = 0; i < i_lo; i++)
                if (ln_pmf_tab(lf, t, n, m_lo, i, ln_total) >= kLnNegligibleP) { i_s = i; break; }
            istart[g] = i_s;
            std::vector<PmfState> st(nl);
            std::vector<uint32_t> h(nl, 0);
            std::vector<uint8_t> act(nl, 0), sat(nl, 0);
            for (uint32_t l = 0; l < nl; l++) {
                const uint32_t m = ms[D - 1 - (g * 64 + l)];
                act[l] = m != 0;
                if (act[l]) { st[l] = pmf_start_at(lf, t, n, m, i_s, ln_total); h[l] = hist[m]; }
            }
            bw[g] = n + 1;
            for (uint32_t i = i_s; i <= n; i++) {
                bool all_sat = i > i_s;
                for (uint32_t l = 0; l < nl; l++) {
                    if (!act[l]) continue;
                    const uint32_t m = ms[D - 1 - (g * 64 + l)];
                    if (i > i_s) {
                        const double c_old = st[l].c;
                        const int k_old = st[l].k;
                        pmf_step(st[l], inv.data(), t, n, m, i);
                        sat[l] = st[l].c == c_old && k_old == 0 && st[l].k == 0;
                    }
                    all_sat = all_sat && sat[l];
                }
                if (all_sat) {
                    double b = 1.0;
                    for (uint32_t l = 0; l < nl; l++)
                        if (act[l]) b *= pmf_cmf_pow(st[l], h[l]);
                    base[g] = b;
                    bw[g] = i;
                    break;
                }
                if (i >= i_lo) {
                    double f = 1.0;
                    for (uint32_t l = 0; l < nl; l++)
                        if (act[l]) f *= pmf_cmf_pow(st[l], h[l]);
                    prod[i] *= f;
                    st_heavy++;
                } else {
                    st_light++;
                }
            }
        }
        for (uint32_t i = i_lo; i <= n; i++) {
            double p = prod[i];
            for (uint32_t g = 0; g < ngroups; g++)
                if (!skipped[g] && i >= bw[g]) p *= base[g];
            Pi[i] = p;
        }
        for (uint32_t g = 0; g < ngroups; g++) {
            const uint32_t nl = std::min<uint32_t>(64, D - g * 64);
            for (uint32_t l = 0; l < nl; l++) {
                const uint32_t m = ms[D - 1 - (g * 64 + l)];
                if (m == 0) { tab[0] = Pi[0]; continue; }
                if (skipped[g]) { tab[m] = 0.0; continue; }
                const uint32_t i_s = istart[g];
                PmfState st = pmf_start_at(lf, t, n, m, i_s, ln_total);
                double acc = 0.0;
                const uint32_t last = std::min(n, bw[g] == 0 ? 0 : bw[g] - 1);
                for (uint32_t i = i_s; i <= last; i++) {
                    if (i > i_s) pmf_step(st, inv.data(), t, n, m, i);
                    if (i < i_lo) continue;
                    const double P = Pi[i];
                    if (P > 0.0 && st.k == 0 && st.c > 0.0) acc += st.v * P / st.c;
                }
                tab[m] = acc;
            }
        }
    }
    double Z = 0.0;
    for (uint32_t m : ms) Z += (double)hist[m] * tab[m];
    const double inv_n = 1.0 / (double)n_refs;
    double g = 0.0;
    for (uint32_t m = 0; m <= t; m++) table_z[m] = 0.0;
    for (uint32_t m : ms) {
        const double v = tab[m] / Z;
        table_z[m] = v;
        g += (double)hist[m] * (v - inv_n) * (v - inv_n);
    }
    *z = Z;
    *gs = sqrt(g);
    if (stats) { stats[0] = st_heavy; stats[1] = st_light; stats[2] = st_skip; stats[3] = st_ilo; }
    return 0;
}


// Sequential emulation of prob_lookup_kernel + prob_tables_build_kernel (rtx_prob_tables.hip): the rows
// C = ln cmf, R = pmf/cmf, sat and ilo are produced by the same recurrence (here on demand instead of from the
// memoised table), then P(i) and table[m] are formed exactly as the lookup kernel does.
// stats (may be null): [0] rows still moving at i_lo (the live rows), [1] points (row, i) folded into P, [2] i_lo, [3] bit s set: some
// live row moves last in the s-th 64-wide slice of i from i_lo (what the kernel's s_nlive is built from).
// u_thr > 0: the query as tile pruning treats it (prob_lookup_kernel with ProbParams::prune_thr / prune_i1): the counts up to u_thr
// become references without a hit (bin 0) with probability 0, and the sums over i start at i1 if that lies beyond i_lo.
static int emul_prob_lookup_x(uint32_t t, const uint32_t *hist_in, uint64_t n_refs, const double *lf, uint32_t u_thr, uint32_t i1,
                              double *table_z, double *z, double *gs, uint64_t *stats) {
    const uint32_t n = t >> 1;
    if (t == 0) return 1;
    std::vector<uint32_t> hist_v(hist_in, hist_in + t + 1);
    for (uint32_t m = 1; m <= u_thr && m <= t; m++) { hist_v[0] += hist_v[m]; hist_v[m] = 0; }
    const uint32_t *hist = hist_v.data();
    std::vector<uint32_t> ms;
    for (uint32_t m = 0; m <= t; m++)
        if (hist[m]) ms.push_back(m);
    std::vector<double> inv(t + n + 2, 0.0);
    for (uint32_t x = 1; x <= t + n; x++) inv[x] = 1.0 / (double)x;
    const double ln_total = ln_binom_tab(lf, t + n - 1, n);
    std::vector<double> tab(t + 1, 0.0);
    uint64_t st_rows = 0, st_points = 0, st_ilo = 0, st_slices = 0;
    uint32_t sat2 = 0;  // first i behind sat at which pmf / cmf < 2^-90 (prob_tables_build_kernel: kRatioNegligible)
    auto build_row = [&](uint32_t m, std::vector<double> &C, std::vector<double> &R, uint32_t &sat, uint32_t &ilo) {
        C.assign(n + 1, 0.0);
        R.assign(n + 1, 0.0);
        double ln_end = 0.0;  // the row is stored relative to its final value (prob_tables_build_kernel)
        {
            PmfState e = pmf_start(lf, t, n, m, ln_total);
            for (uint32_t i = 1; i <= n; i++) pmf_step(e, inv.data(), t, n, m, i);
            if (e.k == 0 && e.c > 0.0) ln_end = log(e.c);
        }
        PmfState st = pmf_start(lf, t, n, m, ln_total);
        sat = n + 1;
        sat2 = n + 1;
        ilo = n;
        bool found = false;
        for (uint32_t i = 0; i <= n; i++) {
            if (i > 0) {
                const double c_old = st.c;
                const int k_old = st.k;
                pmf_step(st, inv.data(), t, n, m, i);
                if (sat == n + 1 && st.c == c_old && k_old == 0 && st.k == 0) sat = i;
            }
            const bool live = st.k == 0 && st.c > 0.0;
            C[i] = live ? log(st.c) - ln_end : -INFINITY;
            R[i] = live ? st.v / st.c : 0.0;
            if (sat2 == n + 1 && sat != n + 1 && R[i] < 8.0779356694631609e-28) sat2 = i;
            if (!found && ln_pmf_tab(lf, t, n, m, i, ln_total) >= kLnNegligibleP) { ilo = i; found = true; }
        }
    };
    if (ms.back() == t) {
        for (uint32_t m : ms) tab[m] = only_last_pmf_tab(lf, t, n, m, ln_total);
    } else {
        if (n == 0) return 1;
        const uint32_t M = ms.back();
        std::vector<double> C, R;
        uint32_t sat = 0, ilo = 0, i_lo = 0;
        if (M > 0) { build_row(M, C, R, sat, ilo); i_lo = ilo; }
        if (u_thr && i1 > i_lo && i1 <= n) i_lo = i1;
        st_ilo = i_lo;
        std::vector<double> Pi(n + 1, 0.0);  // sum_m hist[m] ln cmf_m(i), then exp
        struct Row { uint32_t m, sat; std::vector<double> R; };
        std::vector<Row> rows;
        for (size_t j = ms.size(); j-- > 0;) {
            const uint32_t m = ms[j];
            if (m == 0) continue;
            build_row(m, C, R, sat, ilo);
            if (sat2 <= i_lo) continue;  // nothing left of the row at i_lo: factor 1, table 0
            for (uint32_t i = i_lo; i <= n; i++)
                if (i < sat) { Pi[i] = fma((double)hist[m], C[i], Pi[i]); st_points++; }
            rows.push_back(Row{m, sat2, R});
            st_rows++;
            const uint32_t s_end = std::min(sat, n + 1);
            const uint32_t nsl = s_end > i_lo ? (s_end - i_lo + 63u) >> 6 : 1u;  // (prob_lookup_kernel: s_nlive)
            st_slices |= 1ull << (std::min(nsl, 16u) - 1u);
        }
        for (uint32_t i = 0; i <= n; i++) Pi[i] = exp(Pi[i]);
        for (const Row &r : rows) {
            const uint32_t last = std::min(n, r.sat - 1);
            double acc = 0.0;
            for (uint32_t i = i_lo; i <= last; i++) acc += r.R[i] * Pi[i];
            tab[r.m] = acc;
        }
        if (ms[0] == 0) tab[0] = i_lo == 0 && u_thr == 0 ? Pi[0] : 0.0;
    }
    double Z = 0.0;
    for (uint32_t m : ms) Z += (double)hist[m] * tab[m];
    const double inv_n = 1.0 / (double)n_refs;
    double g = 0.0;
    for (uint32_t m = 0; m <= t; m++) table_z[m] = 0.0;
    for (uint32_t m : ms) {
        const double v = tab[m] / Z;
        table_z[m] = v;
        g += (double)hist[m] * (v - inv_n) * (v - inv_n);
    }
    *z = Z;
    *gs = sqrt(g);
    if (stats) { stats[0] = st_rows; stats[1] = st_points; stats[2] = st_ilo; stats[3] = st_slices; }
    return 0;
}
int emul_prob_lookup(uint32_t t, const uint32_t *hist, uint64_t n_refs, const double *lf, double *table_z, double *z,
                     double *gs, uint64_t *stats) {
    return emul_prob_lookup_x(t, hist, n_refs, lf, 0, 0, table_z, z, gs, stats);
}
int emul_prob_lookup_pruned(uint32_t t, const uint32_t *hist, uint64_t n_refs, const double *lf, uint32_t u_thr, uint32_t i1,
                            double *table_z, double *z, double *gs) {
    return emul_prob_lookup_x(t, hist, n_refs, lf, u_thr, i1, table_z, z, gs, nullptr);
}

// ln cmf_m(i), i = 0 .. n, exactly as prob_tables_build_kernel stores it (the rows prune_kernel reads for G)
static void emul_ln_cmf_row(uint32_t t, uint32_t m, const double *lf, std::vector<double> &C) {
    const uint32_t n = t >> 1;
    C.assign(n + 1, 0.0);
    if (m == 0) return;
    std::vector<double> inv(t + n + 2, 0.0);
    for (uint32_t x = 1; x <= t + n; x++) inv[x] = 1.0 / (double)x;
    const double ln_total = ln_binom_tab(lf, t + n - 1, n);
    double ln_end = 0.0;  // relative to the row's final value (prob_tables_build_kernel)
    {
        PmfState e = pmf_start(lf, t, n, m, ln_total);
        for (uint32_t i = 1; i <= n; i++) pmf_step(e, inv.data(), t, n, m, i);
        if (e.k == 0 && e.c > 0.0) ln_end = log(e.c);
    }
    PmfState st = pmf_start(lf, t, n, m, ln_total);
    for (uint32_t i = 0; i <= n; i++) {
        if (i > 0) pmf_step(st, inv.data(), t, n, m, i);
        C[i] = st.k == 0 && st.c > 0.0 ? log(st.c) - ln_end : -INFINITY;
    }
}

// Sequential restatement of step 3 of prune_kernel (rtx_prune.hip): the threshold u (the largest count a reference may have
// and still be treated as a reference without a hit) and i* + 1 from the exact counts `hm` of the 64 references of the block
// with the largest bound (0: no reference / zeroed).  Same inequalities, same tables; only the order of the sums over the
// lanes differs.  The GPU tests hold the kernel's (u, i* + 1) against this, the CPU tests hold this against the oracle on
// adversarial histograms (tests/test_prune_threshold_cpu.py).
// n_groups = 0: the criterion "(3)" -- every reference of the database priced at the candidate threshold (reference shards: every
// shard must arrive at the same threshold, and a shard knows only its own tiles).  n_groups > 0: the tile-aware criterion "(4)" of a
// whole-database handle: gub[g] = the largest bound of group g of tiles (every count of its gn[g] references is at most that), the
// dropped references are priced at min(u, gub), the kept ones number at most the references of the groups with gub > u.
static void emul_prune_threshold_x(uint32_t t, uint64_t n_refs, const uint32_t *hm_in, const double *lf, uint32_t tab_tmax, uint32_t n_groups,
                                   const uint32_t *gub, const uint64_t *gn, uint32_t *u_out, uint32_t *i1_out) {
    const double kLnEps = kPruneLnEpsHD;
    const uint32_t n = t >> 1;
    uint32_t hm[64], M = 0;
    for (int l = 0; l < 64; l++) { hm[l] = hm_in[l]; M = std::max(M, hm[l]); }
    *u_out = 0;
    *i1_out = 0;
    if (!(t >= 16u && t <= tab_tmax && M >= 1u && n >= 2u)) return;
    const double ln_n = log((double)n_refs), ln_total = ln_binom_tab(lf, t + n - 1, n);
    if (M >= t) {
        uint32_t u_max = 0;
        for (uint32_t u = 1; u < t; u++)
            if (ln_binom_tab(lf, u + n - 1, n) - ln_total + ln_n <= kLnEps) u_max = std::max(u_max, u);
        *u_out = u_max;
        return;
    }
    uint32_t n_h = 0, h_min = 0xFFFFFFFFu;
    std::vector<std::vector<double>> rows(64);
    for (int l = 0; l < 64; l++) {
        if (hm[l] * 5u < M * 4u) hm[l] = 0;
        if (hm[l]) { n_h++; h_min = std::min(h_min, hm[l]); emul_ln_cmf_row(t, hm[l], lf, rows[l]); }
    }
    auto passes = [&](uint32_t i) {
        double s = 0.0;
        for (int l = 0; l < 64; l++)
            if (hm[l]) s += rows[l][i];
        return s + log((double)n_h + (double)n_refs * (double)(i + 1u)) <= kLnEps;
    };
    if (!passes(0u)) return;
    uint32_t lo = 0, hi = n - 2u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (passes(mid)) lo = mid; else hi = mid - 1u;
    }
    const uint32_t i1 = lo + 1u;
    const double ln_len = log((double)(n - i1 + 1u));
    uint32_t first_fail = h_min;
    for (uint32_t u = 1; u < h_min; u++) {
        const double up = (double)(u + i1) * (double)(n - i1), dn = (double)(i1 + 1u) * (double)(t - u + n - i1 - 1u);
        if (!(up < dn && ln_len + ln_pmf_tab(lf, t, n, u, i1, ln_total) + ln_n <= kLnEps)) { first_fail = u; break; }
    }
    uint32_t u_max = first_fail - 1u;
    {   // the tighter criteria ("(3)" and "(4)" in rtx_prune.hip): window W = i1 .. i1 + 62 (lanes 0 .. 62), lane 63 = the tail point i1 + 63
        // (4): the kept references number at most those of the groups whose bound lies above the threshold of (2) -- every later candidate is larger
        double kept = (double)n_refs;
        if (n_groups) {
            kept = 0.0;
            for (uint32_t g = 0; g < n_groups; g++)
                if (gub[g] > u_max) kept += (double)gn[g];
        }
        const double ln_kept = log(kept > 1.0 ? kept : 1.0);
        double WA[64], WB[64], ww[64], gw[64];
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t iw = i1 + l;
            gw[l] = ww[l] = 0.0;
            if (iw > n || l == 63) continue;
            double lnG = 0.0;
            for (int h = 0; h < 64; h++)
                if (hm[h]) lnG += rows[h][iw];
            gw[l] = exp(lnG);
            ww[l] = exp(std::min(0.0, ln_kept + lnG));
        }
        double incl = 0.0, a_tot = 0.0;
        for (uint32_t l = 0; l < 64; l++) a_tot += ww[l];
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t iw = i1 + l;
            const bool vi = iw <= n;
            incl += ww[l];
            const double len_tail = vi ? (double)(n - iw + 1u) : 0.0;
            WA[l] = l == 63 ? len_tail * (a_tot + 1.0) : (vi ? incl - ww[l] : 0.0);
            WB[l] = l == 63 ? len_tail : gw[l];
        }
        const double nn = (double)n_refs;
        const bool has_tail = i1 + 63u <= n;
        auto sums_at = [&](uint32_t m, double &a, double &b) {
            a = b = 0.0;
            for (uint32_t l = 0; l < 64; l++) {
                const double P = i1 + l <= n && m != 0u ? exp(ln_pmf_tab(lf, t, n, m, i1 + l, ln_total)) : 0.0;
                a += P * WA[l];
                b += P * WB[l];
            }
        };
        // (4): S_A, S_B of the groups at their own bounds (capped below min H: a group above it is never dead); the groups far below the
        // threshold of (2) together at S(u_(2) - kPruneFarGap) unless too many lie near (prune_kernel: same rule)
        std::vector<double> gsa(n_groups, 0.0), gsb(n_groups, 0.0);
        std::vector<uint8_t> near(n_groups, 0), mid(n_groups, 0);
        double far_a = 0.0, far_b = 0.0, n_far = 0.0, mid_a = 0.0, mid_b = 0.0, n_mid = 0.0;
        if (n_groups) {
            const uint32_t m_far = u_max > kPruneFarGap ? u_max - kPruneFarGap : 0u;
            uint32_t n_near = 0;
            // near: above the threshold of (2), a window sum of their own; mid: within kPruneFarGap below it, together at S(u_(2))
            for (uint32_t g = 0; g < n_groups; g++) {
                near[g] = gn[g] > 0 && gub[g] > u_max;
                mid[g] = gn[g] > 0 && gub[g] > m_far && gub[g] <= u_max;
                n_near += near[g];
            }
            if (n_near > kPruneMaxNear) {
                std::vector<double> inv(t + n + 2, 0.0);
                for (uint32_t x = 1; x <= t + n; x++) inv[x] = 1.0 / (double)x;
                for (uint32_t g = 0; g < n_groups; g++) {
                    near[g] = gn[g] > 0;
                    prune_window_sums(lf, inv.data(), t, n, std::min(gub[g], h_min - 1u), i1, ln_total, [&](uint32_t l) { return WA[l]; },
                                      [&](uint32_t l) { return WB[l]; }, gsa[g], gsb[g]);
                }
            } else {
                for (uint32_t g = 0; g < n_groups; g++) {
                    if (mid[g]) n_mid += (double)gn[g];
                    else if (!near[g]) n_far += (double)gn[g];
                }
                if (m_far) sums_at(m_far, far_a, far_b);
                if (n_mid > 0.0) sums_at(u_max, mid_a, mid_b);
                for (uint32_t g = 0; g < n_groups; g++)
                    if (near[g]) sums_at(std::min(gub[g], h_min - 1u), gsa[g], gsb[g]);
            }
        }
        auto crit = [&](uint32_t u) {
            double a, b;
            sums_at(u, a, b);
            bool falling = true;
            if (has_tail) {
                const uint32_t j = i1 + 63u;
                falling = (double)(u + j) * (double)(n - j) < (double)(j + 1u) * (double)(t - u + n - j - 1u);
            }
            if (!n_groups) return falling && nn * a <= kPruneHalfEpsHD && nn * b <= kPruneHalfEpsHD;
            double ta = n_far * far_a + n_mid * mid_a, tb = n_far * far_b + n_mid * mid_b;
            for (uint32_t g = 0; g < n_groups; g++) {
                if (!near[g]) continue;
                const bool dead = gub[g] <= u;
                ta += (double)gn[g] * (dead ? gsa[g] : a);
                tb += (double)gn[g] * (dead ? gsb[g] : b);
            }
            return falling && ta <= kPruneHalfEpsHD && tb <= kPruneHalfEpsHD;
        };
        uint32_t lo2 = u_max, hi2 = h_min - 1u;
        while (lo2 < hi2) {
            const uint32_t mid = (lo2 + hi2 + 1u) >> 1;
            if (crit(mid)) lo2 = mid; else hi2 = mid - 1u;
        }
        u_max = lo2;
    }
    *u_out = u_max;
    *i1_out = u_max ? i1 : 0u;
}

void emul_prune_threshold(uint32_t t, uint64_t n_refs, const uint32_t *hm_in, const double *lf, uint32_t tab_tmax, uint32_t *u_out,
                          uint32_t *i1_out) {
    emul_prune_threshold_x(t, n_refs, hm_in, lf, tab_tmax, 0, nullptr, nullptr, u_out, i1_out);
}
// The tile-aware criterion from the largest bound of every TILE of 8192 references (what the bounds pass leaves): the tiles are taken in
// groups of ceil(ntiles / 64) consecutive ones, as the 64 lanes of prune_kernel take them.
void emul_prune_threshold_tiles(uint32_t t, uint64_t n_refs, const uint32_t *hm_in, const double *lf, uint32_t tab_tmax, uint32_t ntiles,
                                const uint16_t *tile_ub, uint32_t *u_out, uint32_t *i1_out) {
    const uint32_t per = (ntiles + 63u) / 64u, ng = (ntiles + per - 1u) / per;
    std::vector<uint32_t> gub(ng, 0);
    std::vector<uint64_t> gn(ng, 0);
    for (uint32_t T = 0; T < ntiles; T++) {
        const uint32_t g = T / per;
        gub[g] = std::max<uint32_t>(gub[g], tile_ub[T]);
        const uint64_t lo = (uint64_t)T * 8192u, hi = std::min<uint64_t>(lo + 8192u, n_refs);
        gn[g] += hi > lo ? hi - lo : 0u;
    }
    emul_prune_threshold_x(t, n_refs, hm_in, lf, tab_tmax, ng, gub.data(), gn.data(), u_out, i1_out);
}

// Bit layout of the bitmap rows (rtx_math.hpp ref_slot) and its inverse as hit_count / seg_emit use it:
// word, bit of local reference r; and the reference of (tile, lane, group g, j) = the j-th count of a lane's g-th store.
void emul_ref_slot(uint32_t r, uint32_t stride_bytes, uint32_t *word, uint32_t *bit) { ref_slot(r, stride_bytes, *word, *bit); }
uint32_t emul_slot_ref(uint32_t tile, uint32_t lane, uint32_t g, uint32_t j, uint32_t stride_bytes) {
    return tile * 8192u + (g * tile_lanes(stride_bytes, tile) + lane) * 8u + j;
}

// The SWAR merge of hit_count's epilogue: eight byte counters (two dwords) added to eight u16 counts (four dwords).
void emul_merge_bytes(const uint32_t *sb, uint32_t *st) {
    st[0] += (sb[0] & 0xFFu) | ((sb[0] & 0xFF00u) << 8);
    st[1] += ((sb[0] >> 16) & 0xFFu) | ((sb[0] >> 24) << 16);
    st[2] += (sb[1] & 0xFFu) | ((sb[1] & 0xFF00u) << 8);
    st[3] += ((sb[1] >> 16) & 0xFFu) | ((sb[1] >> 24) << 16);
}

// One lane's view of the six butterfly stages of transpose64 (rtx_kernels.hip): x[64] in, columns out.
void emul_transpose64(const unsigned long long *in, unsigned long long *out) {
    unsigned long long x[64], y[64];
    for (int l = 0; l < 64; l++) x[l] = in[l];
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long m = s == 32 ? 0x00000000FFFFFFFFull : s == 16 ? 0x0000FFFF0000FFFFull : s == 8 ? 0x00FF00FF00FF00FFull
                                   : s == 4 ? 0x0F0F0F0F0F0F0F0Full : s == 2 ? 0x3333333333333333ull : 0x5555555555555555ull;
        for (int l = 0; l < 64; l++) y[l] = x[l ^ s];
        for (int l = 0; l < 64; l++) x[l] = (l & s) ? (((y[l] >> s) & m) | (x[l] & ~m)) : ((x[l] & m) | ((y[l] & m) << s));
    }
    for (int l = 0; l < 64; l++) out[l] = x[l];
}

// The finalisation of one query's result rows as finalise_kernel (rtx_finalise.hip) does it: for every row the number of rows that come
// before it in the order of lineage.rs:91-93 (fin_row_before: the rank count of the kernel's lanes) and its local signal
// (fin_local_signal).  k: [n][D] hundredths, depth: [n], size: [n][D] references below the row's ancestor per level.
// Returns the number of row pairs on which the word-wise compare of the kernel (fin_row_before_words over zero-padded big-endian words)
// and the byte-wise statement of lineage.rs:91-93 (fin_row_before) disagree: 0.
uint32_t emul_finalise_rows(uint32_t n, uint32_t D, const uint8_t *k, const uint32_t *depth, const uint32_t *size, double n_total, uint32_t *rank,
                            double *local) {
    const uint32_t kw = (D + 3u) / 4u;
    std::vector<uint32_t> words((size_t)n * kw, 0u);
    for (uint32_t r = 0; r < n; r++)
        for (uint32_t w = 0; w < kw; w++) {
            uint32_t v = 0;  // the word as the device loads it (little-endian bytes of the DevRow, zero beyond the depth)
            for (uint32_t b = 0; b < 4u; b++) {
                const uint32_t d = 4u * w + b;
                v |= (uint32_t)(d < depth[r] && d < D ? k[(size_t)r * D + d] : 0u) << (8u * b);
            }
            words[(size_t)r * kw + w] = fin_be32(v);
        }
    uint32_t disagree = 0;
    for (uint32_t r = 0; r < n; r++) {
        uint32_t before = 0;
        for (uint32_t x = 0; x < n; x++) {
            const bool a = x != r && fin_row_before(k + (size_t)x * D, depth[x], x, k + (size_t)r * D, depth[r], r);
            const bool b = x != r && fin_row_before_words(&words[(size_t)x * kw], depth[x], x, &words[(size_t)r * kw], depth[r], r, kw);
            disagree += a != b;
            before += b ? 1u : 0u;
        }
        rank[r] = before;
        double eb[64];
        const uint32_t s0 = fin_node_expected(size + (size_t)r * D, depth[r], n_total, eb);  // (per node in the library: node_tables)
        const uint8_t *kr = k + (size_t)r * D;
        local[r] = fin_local_signal([&](uint32_t d) { return kr[d]; }, eb, s0, depth[r]);
    }
    return disagree;
}

// "{:.5}" of n values by rtx_math.hpp's text_put_fix5 (what rtx_text.hip prints), each followed by '\n'; "{:.2}" of the hundredths
// 0 .. n_hund - 1 behind them, the same way.  Returns the bytes written (cap too small: -1).
int64_t emul_text_numbers(const double *v, uint64_t n, uint32_t n_hund, char *out, uint64_t cap) {
    TextWindow w{out, 0, 0, cap};
    for (uint64_t i = 0; i < n; i++) { text_put_fix5(w, v[i]); w.put('\n'); }
    for (uint32_t k = 0; k < n_hund; k++) { text_put_hund(w, k); w.put('\n'); }
    return w.pos > cap ? -1 : (int64_t)w.pos;
}

// The text of a batch as the kernels of rtx_text.hip lay it out, from host arrays of the same shape: per query (input order) its lines
// joined by '\n' and a NUL, at out_off[q]; a query with status != 0 (or without rows) has the empty text.  one[q]: the id of the query's
// only exact match where the override applies, else kTextNoOverride.  seq/seq_off: base codes (tsv only).  Returns the bytes (-1: cap).
int64_t emul_text_batch(const char *lin_bytes, const uint64_t *lin_off, const uint8_t *lin_depth, const uint32_t *row_lineage,
                        const uint8_t *row_depth, const uint8_t *row_hund, const double *row_local, uint32_t D, uint64_t nq,
                        const char *labels, const uint64_t *label_off, const uint8_t *status, const uint64_t *row_begin,
                        const uint32_t *row_count, const double *gs, const uint32_t *one, const uint8_t *seq, const uint64_t *seq_off,
                        int tsv, char *out, uint64_t cap, uint64_t *out_off) {
    const TextSrc t{lin_bytes, lin_off, lin_depth, row_lineage, row_depth, row_hund, row_local, D};
    TextWindow w{out, 0, 0, cap};
    for (uint64_t q = 0; q < nq; q++) {
        out_off[q] = w.pos;
        const uint64_t n_out = status[q] != 0 || row_count[q] == 0 ? 0 : (one[q] != kTextNoOverride ? 1 : row_count[q]);
        for (uint64_t i = 0; i < n_out; i++) {
            if (i) w.put('\n');
            const TextRow r = text_row(t, labels + label_off[q], label_off[q + 1] - label_off[q], row_begin[q], i, one[q], gs[q]);
            if (tsv) {
                const uint8_t *sq = seq + seq_off[q];
                text_tsv_row(w, r, seq_off[q + 1] - seq_off[q], [&](uint64_t j) { return sq[j]; });
            } else {
                text_out_row(w, r);
            }
        }
        w.put('\0');
    }
    out_off[nq] = w.pos;
    return w.pos > cap ? -1 : (int64_t)w.pos;
}

// The scan of one tile by nearest_kernel (rtx_nearest.hip), step by step and lane by lane with the functions the kernel calls: the lowest
// local reference of the tile whose count is `peak`, or 0xFFFFFFFF.  in_tile: references the tile holds (8192, fewer in the last tile).
// packed != 0: lo = the tile's low bytes, hi = its high-bit words (u16 per chunk of eight references); else lo = its u16 counts.
// Every step's lanes are all evaluated before the lowest lane with a match is taken, as the ballot does.
uint32_t emul_nearest_scan(const void *lo, const uint16_t *hi, uint32_t in_tile, uint32_t peak, int packed) {
    const uint32_t per = packed ? 16u : 8u;
    for (uint32_t step = 0; nearest_lane_base(step, 0u, per) < in_tile; step++) {
        uint32_t mask[64];
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t b0 = nearest_lane_base(step, lane, per);
            mask[lane] = 0;
            if (b0 >= in_tile) continue;
            uint32_t w[4];
            if (packed) {
                std::memcpy(w, static_cast<const uint8_t *>(lo) + b0, 16);
                uint32_t h2;
                std::memcpy(&h2, hi + (b0 >> 3), 4);
                mask[lane] = nearest_match16(w, h2, peak, b0, in_tile);
            } else {
                std::memcpy(w, static_cast<const uint16_t *>(lo) + b0, 16);
                mask[lane] = nearest_match8(w, peak, b0, in_tile);
            }
        }
        for (uint32_t lane = 0; lane < 64u; lane++)
            if (mask[lane]) return nearest_lane_base(step, lane, per) + (uint32_t)__builtin_ctz(mask[lane]);
    }
    return 0xFFFFFFFFu;
}
// The alignment of identity_kernel (rtx_identity.hip) with the functions the kernel calls, the blocks of a column one after the other where the
// kernel runs them skewed over the lanes of a group (the same carries between the same blocks): the semi-global edit distance of the query
// against the text r.  q: the query's bytes as the input set holds them from base q_first on -- two per byte (packed != 0: base k in the low
// nibble of byte k >> 1 when k is even) or raw; minus != 0: the reverse complement is aligned.  qlen 1 .. 4096.
uint32_t emul_identity(const uint8_t *q, uint64_t q_first, uint32_t qlen, int packed, int minus, const uint8_t *r, uint32_t rlen) {
    const uint32_t nb = (qlen + 63u) / 64u;
    std::vector<IdentityBlock> blk(nb);
    auto fetch_packed = [&](uint32_t j) { const uint64_t k = q_first + j; return (uint32_t)((q[k >> 1] >> ((k & 1u) * 4u)) & 15u); };
    auto fetch_raw = [&](uint32_t j) { return (uint32_t)q[q_first + j]; };
    for (uint32_t b = 0; b < nb; b++) {
        if (packed) identity_block_init(blk[b], fetch_packed, qlen, b, minus != 0);
        else identity_block_init(blk[b], fetch_raw, qlen, b, minus != 0);
    }
    uint32_t score = qlen, best = qlen;
    for (uint32_t j = 0; j < rlen; j++) {
        const uint32_t code = identity_code(r[j]);
        int h = 0;
        for (uint32_t b = 0; b < nb; b++) h = identity_step(blk[b], code, h, identity_out_mask(qlen, b));
        score += (uint32_t)h;
        best = std::min(best, score);
    }
    return best;
}
uint32_t emul_identity_hundredths(uint32_t dist, uint32_t qlen) { return identity_hundredths(dist, qlen); }

// Primer trimming as trim_kernel (rtx_trim.hip) runs it, with the functions the kernel calls: the read's ends staged into rows
// (trim_stage_row), the patterns as planes (trim_pattern_init), one read against them (trim_read -> trim_search).  codes / code_off: the
// patterns as given, [n_pat] each of end[] (0: 5', 1: 3'), max_errors[] and window[] (0: the default); x: one read of len bytes.
void emul_trim_read(uint32_t n_pat, const uint8_t *codes, const uint32_t *code_off, const uint32_t *end, const uint32_t *max_errors,
                    const uint32_t *window, const uint8_t *x, uint32_t len, uint32_t *lo, uint32_t *hi, uint32_t *hit) {
    std::vector<TrimPattern> pat;
    uint32_t n5 = 0, n3 = 0, w5 = 0, w3 = 0;
    for (uint32_t e = 0; e < 2; e++)
        for (uint32_t i = 0; i < n_pat; i++) {
            if (end[i] != e) continue;
            TrimPattern p;
            trim_pattern_init(p, codes + code_off[i], code_off[i + 1] - code_off[i], max_errors[i], window[i], e == 1u, i);
            pat.push_back(p);
            (e ? n3 : n5)++;
            uint32_t &w = e ? w3 : w5;
            w = std::max(w, p.w);
        }
    std::vector<uint8_t> row5(trim_row_stride(w5) + 16), row3(trim_row_stride(w3) + 16);
    if (n5) trim_stage_row(x, len, w5, false, row5.data());
    if (n3) trim_stage_row(x, len, w3, true, row3.data());
    auto loader = [](const std::vector<uint8_t> &row) {
        return [&row](uint32_t c) { TrimWords t; memcpy(t.w, row.data() + 16u * c, 16); return t; };
    };
    trim_read(pat.data(), n5, n3, loader(row5), loader(row3), len, *lo, *hi, *hit);
}

// Sample demultiplexing as demux_kernel (rtx_demux.hip) runs it, with the functions the kernel calls: the tags packed (demux_tag_init), the
// dense pair table, the ends of every read staged into rows (trim_stage_row) and one read against them (demux_read).  codes / code_off /
// end: the tags as given; pairs: n_pairs x (tag5, tag3, sample) with 0xFFFF for no tag, every one valid (the library checks, not this);
// bases / base_off: n reads; out: [5][n] sample, lo, hi, hit, info.
void emul_demux_reads(uint32_t n_tags, const uint8_t *codes, const uint32_t *code_off, const uint32_t *end, uint32_t n_pairs, const uint32_t *pairs,
                      uint32_t max_mismatches, uint32_t max_offset, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *out) {
    std::vector<DemuxTag> tags;
    std::vector<uint32_t> rank(n_tags);
    uint32_t cnt[2] = {0u, 0u};
    for (uint32_t e = 0; e < 2; e++)
        for (uint32_t i = 0; i < n_tags; i++) {
            if (end[i] != e) continue;
            DemuxTag t;
            demux_tag_init(t, codes + code_off[i], code_off[i + 1] - code_off[i], e == 1u, i);
            tags.push_back(t);
            rank[i] = cnt[e]++;
        }
    const uint32_t n5 = cnt[0], n3 = cnt[1];
    std::vector<uint32_t> table(demux_table_size(n5, n3), kDemuxNone);
    for (uint32_t i = 0; i < n_pairs; i++) {
        const uint32_t a = pairs[3 * i], b = pairs[3 * i + 1];
        table[demux_table_slot(n3, a == kDemuxNoTag ? n5 : rank[a], b == kDemuxNoTag ? n3 : rank[b])] = pairs[3 * i + 2];
    }
    const uint32_t w = demux_window(max_offset), stride = trim_row_stride(w);
    auto pair = [&](uint32_t i5, uint32_t i3) { return table[demux_table_slot(n3, i5, i3)]; };
    for (uint64_t q = 0; q < n; q++) {
        const uint8_t *x = bases + base_off[q];
        const uint64_t len = base_off[q + 1] - base_off[q];
        uint8_t row5[32], row3[32];
        trim_stage_row(x, len, w, false, row5);
        trim_stage_row(x, len, w, true, row3);
        demux_read(tags.data(), n5, n3, pair, max_mismatches, max_offset, demux_window_of(row5, stride), demux_window_of(row3, stride), (uint32_t)len,
                   out[q], out[n + q], out[2 * n + q], out[3 * n + q], out[4 * n + q]);
    }
}

// The quality filter as qual_kernel (rtx_qual.hip) runs it, with the functions the kernel calls, in the kernel's geometry: steps of 16 pieces
// of 16 bytes, the piece sums of a step first, then the scan over them, then every piece's stop with what lies in front of it, the first of
// the step, and the sums read from the piece that holds it.  cfg: the parameters as integers (base, trunc_len, trunc_qual, min_len,
// max_len, max_ns as uint32 / int32 in cfg32[6]; trunc_ee, max_ee, max_ee_rate in cfg64[3], ~0: off); table: the 94 errors; x: the staged
// bytes of one range (quality | 0x80 where the base is no A/C/G/T), len of them.
void emul_qual_read(const int32_t *cfg32, const uint64_t *cfg64, const uint64_t *table, const uint8_t *x, uint32_t len, uint32_t *kept, uint64_t *ee,
                    uint32_t *verdict) {
    QualCfg cfg;
    cfg.base = (uint32_t)cfg32[0];
    cfg.trunc_len = (uint32_t)cfg32[1];
    cfg.trunc_qual = cfg32[2];
    cfg.min_len = (uint32_t)cfg32[3];
    cfg.max_len = (uint32_t)cfg32[4];
    cfg.max_ns = cfg32[5];
    cfg.trunc_ee = cfg64[0];
    cfg.max_ee = cfg64[1];
    cfg.max_ee_rate = cfg64[2];
    std::vector<uint8_t> row((size_t)(len + 15u) / 16u * 16u + 16u, 0xFF);  // (what lies behind the range is never taken as data)
    if (len) memcpy(row.data(), x, len);
    bool short_tl, bad = false, done = false;
    const uint32_t end = qual_end(cfg, len, short_tl);
    uint64_t carry_e = 0;
    uint32_t carry_n = 0, hi = end;
    for (uint32_t s = 0; s * 256u < len; s++) {
        QualPiece pc[kQualGroup];
        uint64_t before_e[kQualGroup], run_e = carry_e;
        uint32_t before_n[kQualGroup], run_n = carry_n;
        for (uint32_t gl = 0; gl < kQualGroup; gl++) {
            const uint32_t pos = s * 256u + gl * 16u;
            QualWords t{{0u, 0u, 0u, 0u}};
            if (pos < len) memcpy(t.w, row.data() + pos, 16);
            qual_piece_sum(cfg, table, t, pos, len, end, pc[gl]);
            bad = bad || pc[gl].bad;
            before_e[gl] = run_e;
            before_n[gl] = run_n;
            run_e += pc[gl].c[kQualPiece - 1u];
            run_n += (uint32_t)__builtin_popcount(pc[gl].ns);
        }
        uint32_t first = 0xFFFFFFFFu, src = kQualGroup - 1u;
        uint64_t at_e[kQualGroup];
        uint32_t at_n[kQualGroup];
        for (uint32_t gl = 0; gl < kQualGroup; gl++) {
            const uint32_t pos = s * 256u + gl * 16u;
            uint64_t e;
            uint32_t nn;
            const uint32_t stop = qual_piece_stop(cfg, pc[gl], before_e[gl], pos, end, e, nn);
            at_e[gl] = before_e[gl] + e;
            at_n[gl] = before_n[gl] + nn;
            if (stop != kQualPiece && pos + stop < first) { first = pos + stop; src = gl; }
        }
        if (!done) {
            carry_e = at_e[src];
            carry_n = at_n[src];
            if (first != 0xFFFFFFFFu) { hi = first; done = true; }
        }
    }
    *kept = bad ? 0u : hi;
    *ee = bad ? 0ull : carry_e;
    *verdict = qual_verdict(cfg, bad, short_tl, hi, carry_e, carry_n);
}

// The contaminant screen as screen_kernel (rtx_screen.hip) runs it, with the functions the kernel calls, in the kernel's geometry: a group of
// 16 lanes, every lane its pieces of 16 window positions in steps of 256, each piece loaded with the 16 bytes behind it (zeros where they
// start at or behind the end), the lanes' counts summed and the lowest first hit taken with the source of the lane that holds it.
// slots: the table of the set, key and src per slot (rtx_screen_set_table); x: the codes of one range, len of them; out: windows, hits, first,
// source.
void emul_screen_read(const uint32_t *slots, uint32_t log2m, const uint8_t *x, uint32_t len, uint32_t *out) {
    const ScreenTable t{reinterpret_cast<const ScreenSlot *>(slots), log2m};
    std::vector<uint8_t> row((size_t)(len + 15u) / 16u * 16u + 16u, 0xFF);  // (what lies behind the range is never taken as data)
    if (len) memcpy(row.data(), x, len);
    ScreenAcc acc[kScreenGroup];
    for (uint32_t gl = 0; gl < kScreenGroup; gl++) {
        acc[gl] = ScreenAcc{0u, 0u, kScreenNone, kScreenNone};
        for (uint32_t pos = gl * kScreenPiece; pos + kScreenK <= len; pos += kScreenGroup * kScreenPiece) {
            ScreenWords a, b{{0u, 0u, 0u, 0u}};
            memcpy(a.w, row.data() + pos, 16);
            if (pos + kScreenPiece < len) memcpy(b.w, row.data() + pos + kScreenPiece, 16);
            screen_piece(t, a, b, pos, len, acc[gl]);
        }
    }
    uint32_t windows = 0, hits = 0, first = kScreenNone, source = kScreenNone;
    for (uint32_t gl = 0; gl < kScreenGroup; gl++) {
        windows += acc[gl].windows;
        hits += acc[gl].hits;
        first = std::min(first, acc[gl].first);
    }
    for (uint32_t gl = 0; gl < kScreenGroup; gl++) source = std::min(source, acc[gl].first == first ? acc[gl].source : kScreenNone);
    out[0] = windows;
    out[1] = hits;
    out[2] = first;
    out[3] = source;
}

// One pair as merge_kernel (rtx_merge.hip) merges it, with the functions the kernel calls, in the kernel's geometry: the mates staged four
// bases per lane and step (a too-long mate only streamed for its bad bytes), the candidates dealt over 64 lanes in strides of 64 -- each
// walked in words of 16 with the early leave --, the maximum over the lanes, then the merged bases written lane l at l + 64 k.
// cfg: ascii_base, min_overlap, max_diffs, max_diff_pct, q_cap; out: overlap, diffs, verdict, merged length; mb / mq take nf + nr bytes.
void emul_merge_pair(const uint32_t *cfg5, const uint8_t *fb, const uint8_t *fq, uint32_t nf, const uint8_t *rb, const uint8_t *rq, uint32_t nr, uint32_t *out,
                     uint8_t *mb, uint8_t *mq) {
    const MergeCfg cfg{cfg5[0], cfg5[1], cfg5[2], cfg5[3], cfg5[4]};
    std::vector<uint16_t> hf(4u * kMergeWords, 0xFFFFu), hr(4u * kMergeWords, 0xFFFFu);  // (what no lane wrote is never taken as data)
    std::vector<uint8_t> qf(kMergeMaxRead, 0xFF), qr(kMergeMaxRead, 0xFF);
    const bool fits = nf <= kMergeMaxRead && nr <= kMergeMaxRead;
    bool bad = false;
    for (uint32_t side = 0; side < 2u; side++) {
        const uint8_t *codes = side ? rb : fb, *quals = side ? rq : fq;
        const uint32_t n = side ? nr : nf;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            if (fits) {
                for (uint32_t h = lane; 4u * h < n; h += 64u) {
                    uint32_t nib16, q32;
                    bool b;
                    merge_stage4(cfg, [codes](uint32_t k) { return (uint32_t)codes[k]; }, [quals](uint32_t k) { return (uint32_t)quals[k]; }, n, side == 1u, h, nib16, q32, b);
                    (side ? hr : hf)[h] = (uint16_t)nib16;
                    memcpy((side ? qr : qf).data() + 4u * h, &q32, 4);
                    bad = bad || b;
                }
            } else {
                for (uint32_t k = lane; k < n; k += 64u) bad = bad || merge_bad_byte(cfg, quals[k]);
            }
        }
    }
    out[0] = out[1] = out[3] = 0u;
    out[2] = merge_pre_verdict(cfg, bad, nf, nr);
    if (out[2]) return;
    auto word = [](const std::vector<uint16_t> &h, uint32_t w) { uint64_t v; memcpy(&v, h.data() + 4u * w, 8); return v; };
    auto word_f = [&](uint32_t w) { return word(hf, w); };
    auto word_r = [&](uint32_t w) { return word(hr, w); };
    uint32_t best = 0;
    for (uint32_t lane = 0; lane < 64u; lane++) {
        uint32_t mine = 0;
        for (uint32_t c = cfg.min_overlap + lane; c <= std::min(nf, nr); c += kMergeStride) mine = std::max(mine, merge_candidate(cfg, word_f, word_r, nf, c));
        best = std::max(best, mine);
    }
    if (!best) { out[2] = kMgNoOverlap; return; }
    merge_key_read(best, out[0], out[1]);
    out[3] = nf + nr - out[0];
    for (uint32_t lane = 0; lane < 64u; lane++)
        for (uint32_t at = lane; at < out[3]; at += 64u) {
            uint32_t code, byte;
            merge_base_at(cfg, word_f, word_r, [&qf](uint32_t k) { return (uint32_t)qf[k]; }, [&qr](uint32_t k) { return (uint32_t)qr[k]; }, nf, out[0], at, code, byte);
            mb[at] = (uint8_t)code;
            mq[at] = (uint8_t)byte;
        }
}

// byte, high-bit word and shift of local reference rl in the packed counts of its tile (packed_count_pos)
void emul_packed_count_pos(uint32_t rl, uint32_t *byte, uint32_t *hi_word, uint32_t *hi_shift) { packed_count_pos(rl, *byte, *hi_word, *hi_shift); }

// The taxon profile of a batch as profile_kernel (rtx_profile.hip) accumulates it, query by query with the step the kernel calls
// (profile_step): the path is walked from a_{L-1} up as the kernel's lanes walk it.  one[q]: the id of the query's only exact match where the
// override applies, else kTextNoOverride.  The counters are added to (the caller zeroes them).
void emul_profile(uint64_t nq, const uint8_t *status, const uint32_t *row_count, const uint64_t *row_begin, const uint32_t *row_node,
                  const uint8_t *row_depth, const uint8_t *row_hund, uint32_t D, const uint32_t *parent, const uint8_t *node_depth,
                  const uint32_t *ref_leaf, uint32_t n_nodes, uint32_t n_refs, const uint32_t *one, uint32_t cutoff, uint64_t *clade,
                  uint64_t *direct, uint64_t *conf_sum, uint64_t *totals) {
    const ProfileSrc src{status, row_count, reinterpret_cast<const unsigned long long *>(row_begin), row_node, row_depth, row_hund, D, parent, node_depth, ref_leaf, n_nodes, n_refs};
    for (uint64_t q = 0; q < nq; q++) {
        const ProfileStep st = profile_step(src, q, one[q], cutoff);
        totals[0]++;
        totals[st.kind == kProfClassified ? 1 : (st.kind == kProfUnclassified ? 2 : 3)]++;
        if (st.kind != kProfClassified) continue;
        uint32_t node = st.node;
        for (uint32_t d = st.L; d-- > 0u;) {
            if (node >= n_nodes) break;
            clade[node]++;
            conf_sum[node] += st.at(d);
            if (d + 1u == st.L) direct[node]++;
            node = parent[node];
        }
    }
}

// ---- chimera check (rtx_chimera.hip) --------------------------------------------------------------------------------------------------
// The boundaries b[S + 1] and the padded layout of both directions (off0 / off1 [S + 1]: chimera_layout); returns the entries a list of
// it is allotted (chimera_list_cap), 0 for an S out of range.
uint32_t emul_chimera_layout(uint32_t n_pos, uint32_t S, uint32_t *b, uint32_t *off0, uint32_t *off1) {
    if (S < 2u || S > kChimMaxSegments) return 0u;
    for (uint32_t s = 0; s <= S; s++) b[s] = chimera_boundary(n_pos, S, s);
    const uint32_t rows = chimera_layout(n_pos, S, 0u, off0);
    chimera_layout(n_pos, S, 1u, off1);
    return rows == chimera_list_rows(n_pos, S) && off1[S] == rows ? chimera_list_cap(rows) : 0u;
}
// The list of direction `dir` as chimera_rows_kernel fills it: out[j] = the window of entry j or 0xFFFFFFFF (the zero row), for j < cap.
void emul_chimera_list(uint32_t n_pos, uint32_t S, uint32_t dir, uint32_t cap, uint32_t *out) {
    uint32_t off[kChimMaxSegments + 1];
    chimera_layout(n_pos, S, dir, off);
    for (uint32_t lane = 0; lane < 64u; lane++)
        for (uint32_t j = lane; j < cap; j += 64u) out[j] = chimera_list_window(n_pos, S, dir, off, j);
}
uint32_t emul_chimera_n_pos(uint32_t len) { return chimera_n_pos(len); }
// A checkpoint of chimera_scan_kernel on one tile: counts[8192] (each < 2^planes; 0 behind the references the tile holds) are laid into the
// planes of the 64 lanes by ref_slot, every lane runs chimera_lane_best, then the wave maximum and the minimum over the lanes that hold it.
// *count / *ref (global id, 0xFFFFFFFF: none); returns 0 / -1 as above.
int emul_chimera_checkpoint(const uint16_t *counts, int planes, uint32_t stride_bytes, uint32_t tile, uint32_t *count, uint32_t *ref) {
    return emul_with_planes(planes, [&](auto tag) {
        constexpr int NP = decltype(tag)::value;
        const uint32_t L = tile_lanes(stride_bytes, tile);
        std::vector<std::array<std::array<uint32_t, NP>, 4>> pl(64);
        for (auto &l : pl)
            for (auto &w : l) w.fill(0u);
        for (uint32_t rl = 0; rl < 8192u && (rl >> 3) < L * 16u; rl++) {
            uint32_t word, bit;
            ref_slot(tile * 8192u + rl, stride_bytes, word, bit);
            word -= tile * 256u;
            for (int p = 0; p < NP; p++) pl[word >> 2][word & 3u][p] |= (((uint32_t)counts[rl] >> p) & 1u) << bit;
        }
        uint32_t m[64], r[64], M = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t a[4][NP];
            for (int w = 0; w < 4; w++)
                for (int p = 0; p < NP; p++) a[w][p] = pl[lane][w][p];
            chimera_lane_best<NP>(a, lane, L, m[lane], r[lane]);
            M = std::max(M, m[lane]);
        }
        uint32_t R = kChimNoRef;
        for (uint32_t lane = 0; lane < 64u; lane++) R = std::min(R, M != 0u && m[lane] == M ? tile * 8192u + r[lane] : kChimNoRef);
        *count = M;
        *ref = R;
    });
}
// chimera_reduce_kernel: best [2][S][ntiles][2] (count, reference) as the scan stores them -> the record (twelve words)
void emul_chimera_reduce(uint32_t len, uint32_t n_valid, uint32_t S, uint32_t mindelta, uint32_t ntiles, const uint32_t *best, uint32_t *rec) {
    uint32_t pm[kChimMaxSegments + 1] = {0}, sm[kChimMaxSegments + 1] = {0}, pr[kChimMaxSegments + 1], sr[kChimMaxSegments + 1];
    for (uint32_t s = 0; s <= kChimMaxSegments; s++) pr[s] = sr[s] = kChimNoRef;
    if (n_valid != 0u && len <= kChimMaxQuery)
        for (uint32_t lane = 0; lane < 2u * S; lane++) {
            const uint32_t dir = lane / S, k = lane % S;
            uint32_t bc = 0u, br = kChimNoRef;
            for (uint32_t t = 0; t < ntiles; t++) chimera_take(bc, br, best[((size_t)lane * ntiles + t) * 2u], best[((size_t)lane * ntiles + t) * 2u + 1u]);
            if (dir == 0u) { pm[k + 1u] = bc; pr[k + 1u] = br; }
            else { sm[S - 1u - k] = bc; sr[S - 1u - k] = br; }
        }
    const ChimRec r = chimera_record(len, n_valid, S, mindelta, pm, pr, sm, sr);
    std::memcpy(rec, &r, sizeof r);
}

// ---- de novo chimera check (rtx_denovo.hip) ------------------------------------------------------------------------------------------
// The prefix mask of `lim` over a tile of the stage's bitmap over n_parents entries: out[64][4], lane by lane (denovo_allow); returns the
// lanes of the tile.
uint32_t emul_denovo_allow(uint32_t n_parents, uint32_t tile, uint32_t lim, uint32_t *out) {
    const uint32_t L = tile_lanes(denovo_stride_bytes(n_parents), tile);
    for (uint32_t lane = 0; lane < 64u; lane++) denovo_allow(lane, L, tile, lim, out + lane * 4u);
    return L;
}
// ---- denoising (rtx_unoise.hip) ----------------------------------------------------------------------------------------------------------
// One lane of unoise_pair_kernel: x is the pattern (the bit rows of its codes laid out as the wave lays them out in LDS), y the text as
// packed words.  d(x, y) if it is at most k, else 0xFFFFFFFF -- also when the lengths differ by more than k (the kernel's length test)
// or k is above 16.  Codes are the low four bits of a byte.
uint32_t emul_unoise_distance(const uint8_t *x, uint32_t nx, const uint8_t *y, uint32_t ny, uint32_t k) {
    if (k > kUnoiseMaxDiffs || (nx > ny ? nx - ny : ny - nx) > k) return kUnoiseNoDist;
    const uint32_t nw = unoise_peq_words(nx);
    std::vector<uint64_t> peq((size_t)16 * nw, 0), text((ny + 15u) / 16u + 1u, 0);
    for (uint32_t i = 0; i < nx; i++) {
        const uint32_t b = unoise_peq_bit(i);
        peq[(size_t)(x[i] & 15u) * nw + (b >> 6)] |= 1ull << (b & 63u);
    }
    unoise_pack(y, ny, text.data());
    bool finished = false;
    return unoise_distance(nx, ny, k, [&](uint32_t c, uint32_t j) { return unoise_eq(peq.data() + (size_t)c * nw, j); }, [&](uint32_t t) { return text[t]; }, finished);
}
uint32_t emul_unoise_allowed(uint64_t wp, uint64_t we, uint32_t alpha, uint32_t max_diffs) { return unoise_allowed(wp, we, alpha, max_diffs); }

// A checkpoint of denovo_scan_kernel on one tile: emul_chimera_checkpoint with the planes masked by live[8192] (0 / 1 per local entry, laid
// into the lanes by ref_slot as the live row is) AND the prefix mask of lim.
int emul_denovo_checkpoint(const uint16_t *counts, const uint8_t *live, int planes, uint32_t n_parents, uint32_t tile, uint32_t lim, uint32_t *count, uint32_t *ref) {
    return emul_with_planes(planes, [&](auto tag) {
        constexpr int NP = decltype(tag)::value;
        const uint32_t stride_bytes = denovo_stride_bytes(n_parents), L = tile_lanes(stride_bytes, tile);
        std::vector<std::array<std::array<uint32_t, NP>, 4>> pl(64);
        std::vector<std::array<uint32_t, 4>> lv(64);
        for (auto &l : pl)
            for (auto &w : l) w.fill(0u);
        for (auto &l : lv) l.fill(0u);
        for (uint32_t rl = 0; rl < 8192u && (rl >> 3) < L * 16u; rl++) {
            uint32_t word, bit;
            ref_slot(tile * 8192u + rl, stride_bytes, word, bit);
            word -= tile * 256u;
            for (int p = 0; p < NP; p++) pl[word >> 2][word & 3u][p] |= (((uint32_t)counts[rl] >> p) & 1u) << bit;
            lv[word >> 2][word & 3u] |= (live[rl] ? 1u : 0u) << bit;
        }
        uint32_t m[64], r[64], M = 0;
        for (uint32_t lane = 0; lane < 64u; lane++) {
            uint32_t a[4][NP], allow[4];
            for (int w = 0; w < 4; w++)
                for (int p = 0; p < NP; p++) a[w][p] = pl[lane][w][p];
            denovo_allow(lane, L, tile, lim, allow);
            for (int w = 0; w < 4; w++) allow[w] &= lv[lane][w];
            denovo_lane_best<NP>(a, allow, lane, L, m[lane], r[lane]);
            M = std::max(M, m[lane]);
        }
        uint32_t R = kChimNoRef;
        for (uint32_t lane = 0; lane < 64u; lane++) R = std::min(R, M != 0u && m[lane] == M ? tile * 8192u + r[lane] : kChimNoRef);
        *count = M;
        *ref = R;
    });
}

}  // extern "C"

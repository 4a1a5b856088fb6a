// The OTUs of a run on the host (rtx_otu; raxtax_hip.h, "OTUs of a run"): the result object that rtx_otu_cluster (rtx_otu.hip) and
// rtx_otu_cluster_host fill, the host restatement of the definition, the per-OTU sums and the text.  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "host_tally.hpp"

// What a graft result (rtx_otu_graft, rtx_otu_graft_host; raxtax_hip.h, "Fastidious grafting") carries beside its clustering
struct rtx_graft_info {
    uint64_t boundary = 0, old_otus = 0;
    uint64_t heavy_otus = 0, light_otus = 0, heavy_rows = 0, light_rows = 0;
    uint64_t variants = 0, candidates = 0, confirmed = 0;  // the filter's: 0 for a host result
    uint32_t bloom_log2 = 0, test_passes = 0;              // likewise
    std::vector<uint32_t> parent, old_to_new;              // [n_rows], [old_otus]
    std::vector<uint32_t> light, child, par, heavy, into;  // the grafts, sorted by the old light OTU
    std::vector<uint64_t> size;                            // the size of the old light OTU
    double seconds[5] = {0, 0, 0, 0, 0};                   // upload, Bloom, test, verify, resolve and download
};

// What a denoising result (rtx_otu_unoise, rtx_otu_unoise_host; raxtax_hip.h, "Denoising (UNOISE)") carries beside its clustering
struct rtx_unoise_info {
    rtx_unoise_params params{};                    // as used (max_diffs filled in)
    std::vector<uint8_t> status;                   // [n_rows] RTX_UNOISE_*
    std::vector<uint32_t> parent, dist, lim;       // [n_rows]
    std::vector<uint64_t> weight;                  // [n_rows] w[r], for the text
    uint64_t n_status[4] = {0, 0, 0, 0};
    uint32_t tiers = 0, launches = 0;              // the device's: 0 for a host result
    uint64_t pairs = 0, pairs_length = 0, pairs_finished = 0;
    double seconds[4] = {0, 0, 0, 0};              // upload, pair kernels, bookkeeping, download
};

struct rtx_otu {
    std::unique_ptr<rtx_graft_info> graft;         // a graft result has one
    std::unique_ptr<rtx_unoise_info> unoise;       // a denoising result has one
    uint64_t n_rows = 0, n_otus = 0;
    uint32_t columns = 1;
    std::vector<uint32_t> otu, seed;               // [n_rows], [n_otus]
    std::vector<uint64_t> members, sizes, counts;  // [n_otus], [n_otus], [n_otus x columns]
    std::vector<uint32_t> link_a, link_b;          // a < b, sorted by (a, b)
    uint32_t rounds = 0, link_passes = 0;
    uint64_t long_rows = 0;
    double seconds[4] = {0, 0, 0, 0};              // upload, link passes, label rounds and numbering, download (rtx_otu_times)
};

namespace rtx {

// The checks the two entries share: the table and `out` are there, differences is 0 or 1, flags 0, at most 2^31 - 2 rows; the table laid out
// into *view and the parameters (NULL: defaults) into *p.  RTX_ERR_INVALID with the error text set, `who` in front.
int otu_open(const char *who, rtx_tally_table *table, const rtx_otu_params *params, rtx_otu **out, rtx_tally_view *view, rtx_otu_params *p);
// o.otu holds the OTU of every row, numbered in the order of the seeds: seed, members, sizes and counts from it and the rows of the table
void otu_sums(rtx_otu &o, const rtx_tally_view &view);
// the second half of it alone: o.otu and o.seed are given (a graft result keeps the seeds of the surviving OTUs, and a grafted row may outrank one)
void otu_totals(rtx_otu &o, const rtx_tally_view &view);

// The checks the two graft entries share: table, object and `out` are there, the table has the object's rows, flags 0, bloom_log2 0 or
// 5 .. 40; the table laid out into *view and the parameters with their defaults filled in (boundary, max_bloom_bytes) into *p.
int graft_open(const char *who, rtx_tally_table *table, rtx_otu *otu, const rtx_graft_params *params, rtx_otu **out, rtx_tally_view *view, rtx_graft_params *p);
// one flag per row: its OTU is heavy (sizes[k] >= boundary); the counts of both kinds into g
void graft_heavy(const rtx_otu &in, uint64_t boundary, std::vector<uint8_t> &heavy, rtx_graft_info &g);
// The result from the parents (parent[x] for every row, all ones: none): the grafts, the numbering, otu', the sums; links, rounds, link_passes
// and long_rows of `in`.  `out` holds its graft info already (the counters).
void graft_build(const rtx_otu &in, const rtx_tally_view &view, const std::vector<uint8_t> &heavy, std::vector<uint32_t> parent, rtx_otu &out);

}  // namespace rtx

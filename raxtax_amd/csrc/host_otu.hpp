// The OTUs of a run on the host (rtx_otu; raxtax_hip.h, "OTUs of a run"): the result object that rtx_otu_cluster (rtx_otu.hip) and
// rtx_otu_cluster_host fill, the host restatement of the definition, the per-OTU sums and the text.  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <vector>

#include "host_tally.hpp"

struct rtx_otu {
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

}  // namespace rtx

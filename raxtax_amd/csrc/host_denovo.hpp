// The de novo chimera check of a run on the host (rtx_denovo; raxtax_hip.h, "de novo chimera check of a run"): the result object that
// rtx_denovo_check (rtx_denovo.hip) and rtx_denovo_check_host fill, the entries and their lim, the host restatement of the definition and
// the text.  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <vector>

#include "host_otu.hpp"

struct rtx_denovo {
    uint64_t n_entries = 0, n_rows = 0;
    bool otu_mode = false;
    rtx_denovo_params params{};
    std::vector<uint32_t> row, otu, lim;  // [n_entries]; otu is empty without an OTU object
    std::vector<uint64_t> weight;
    std::vector<rtx_chimera_rec> rec;
    uint64_t n_checked = 0, n_flagged = 0, scans = 0;
    uint32_t rounds = 0;
    double seconds[4] = {0, 0, 0, 0};     // upload and bitmap, scans, the rounds' bookkeeping, download (rtx_denovo_times)
};

namespace rtx {

// The checks the two entries share (RTX_ERR_INVALID with the error text set, `who` in front); the table laid out into *view, the
// parameters (NULL: defaults; max_parents 0: the default) into *p.
int denovo_open(const char *who, rtx_tally_table *table, rtx_otu *otu, const rtx_denovo_params *params, rtx_denovo **out, rtx_tally_view *view, rtx_denovo_params *p);
// row, otu, weight and lim of every entry into d; d.rec sized and preset to "not checked"
void denovo_entries(rtx_denovo &d, const rtx_tally_view &view, const rtx_otu *otu, const rtx_denovo_params &p);
// the record of an entry that has no scan: the status and nothing else
rtx_chimera_rec denovo_blank(uint32_t status);
// n_checked and n_flagged from d.rec
void denovo_totals(rtx_denovo &d);

}  // namespace rtx

// Denoising on the host (raxtax_hip.h, "Denoising (UNOISE)"): the checks, lim and the tiers of the device path and the result from the statuses;
// host_unoise.cpp also holds the host restatement of the definition and the text.  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <vector>

#include "host_otu.hpp"  // rtx_unoise_info: what such an rtx_otu carries beside its clustering

namespace rtx {

// The checks the two entries share: table and `out` are there, alpha 1 .. 8, minsize at least 1, max_diffs at most 16 (0: 16), flags 0, at
// most 2^31 - 2 rows; the table laid out into *view, the parameters (NULL: defaults) into *p.  RTX_ERR_INVALID with the error text set.
int unoise_open(const char *who, rtx_tally_table *table, const rtx_unoise_params *params, rtx_otu **out, rtx_tally_view *view, rtx_unoise_params *p);
// lim(e) = #{p : (w[p] >> (alpha + 1)) >= w[e]} for every row (weights never increase along the table: one walk)
void unoise_lim(const rtx_tally_view &view, uint32_t alpha, std::vector<uint32_t> &lim);
// The tiers: begin[t] .. begin[t + 1], begin[t + 1] the first row with (w[begin[t]] >> (alpha + 1)) >= w[row]; the last entry is n_rows.
void unoise_tiers(const rtx_tally_view &view, uint32_t alpha, std::vector<uint64_t> &begin);
// The result from status, parent and dist of every row (in o.unoise, with params and lim): the OTUs, their sums, the status counts, long_rows.
// RTX_ERR_HIP (the device's statuses are checked here too) when an absorbed row names a parent that is no ZOTU below lim.
int unoise_build(const char *who, rtx_otu &o, const rtx_tally_view &view);

}  // namespace rtx

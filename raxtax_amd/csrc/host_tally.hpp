// The table of distinct reads on the host (rtx_tally_table; raxtax_hip.h, "distinct reads of a run"): what rtx_tally_read downloads, what
// rtx_tally_table_add accumulates as the host restatement of rtx_tally_add, their sum and their text.  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_stage.hpp"

// Entries in the order of first appearance; the sorted rows of the view are laid out when somebody asks (and again after an add).
struct rtx_tally_table {
    uint32_t columns = 1;      // max(1, n_samples)
    uint32_t n_samples = 0;
    std::vector<std::string> seqs;                    // [entries] one code per byte
    std::vector<uint64_t> counts;                     // [entries x columns]
    std::unordered_map<std::string, uint64_t> index;  // sequence -> entry
    uint64_t reads = 0, overflow_reads = 0;
    // the view
    bool laid_out = false;
    std::vector<uint8_t> v_bases;
    std::vector<uint64_t> v_off, v_counts, v_sizes, v_first;
};

namespace rtx {

// the entry of a sequence, appended with zero counts if it is new
uint64_t tally_table_entry(rtx_tally_table &t, const uint8_t *seq, uint64_t len);
// The checks rtx_tally_add and rtx_tally_table_add share: monotone offsets, the samples of the reads that count, and the counted weight of
// the chunk (*counted) on top of `so_far` within 2^32 - 1.  RTX_ERR_INVALID with the error text set, `who` in front.
int tally_check_chunk(const char *who, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample, const uint32_t *weight, uint32_t columns,
                      uint64_t so_far, uint64_t *counted);
// the two-pass protocol of the formatters (rtx_profile_format): the bytes of `text`, into buf when it is there and holds them
int64_t hand_out(const char *who, const std::string &text, char *buf, uint64_t cap);

}  // namespace rtx

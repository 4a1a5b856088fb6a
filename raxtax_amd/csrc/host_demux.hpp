// Sample demultiplexing, host side (host_demux.cpp): a checked tag list as the kernel and rtx_demux_read take it.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "rtx_internal.hpp"
#include "rtx_math.hpp"

namespace rtx {

struct DemuxSet {
    std::vector<DemuxTag> tags;  // the 5' ones, then the 3' ones (reversed), each end in the order of the caller's list
    uint32_t n5 = 0, n3 = 0, max_mismatches = 0, max_offset = 0;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;  // (demux_table_slot, sample), sorted by slot
    uint32_t sample_of(uint32_t i5, uint32_t i3) const;  // kDemuxNone: no such pair
    std::vector<uint32_t> dense_table() const;           // demux_table_size entries
};

// the checks of rtx_demux_create, in its order: RTX_OK and the set, or RTX_ERR_INVALID with the offender named
int demux_build(const char *who, const rtx_demux_tag *tags, uint32_t n_tags, const rtx_demux_pair *pairs, uint32_t n_pairs,
                const rtx_demux_params *params, DemuxSet &out);

}  // namespace rtx

// Paired-end merging: the host functions that rtx_merge.hip shares with host_merge.cpp (rtx_math.hpp has the arithmetic).
#pragma once

#include <cstdint>

#include "raxtax_hip.h"
#include "rtx_math.hpp"

namespace rtx {

int merge_check_params(const char *who, const rtx_merge_params *p);  // RTX_OK, or RTX_ERR_INVALID with the field named
void merge_cfg_init(MergeCfg &c, const rtx_merge_params &p);         // (checked before)
// the key of a FASTQ label that the two mates of a pair share: up to its first blank, a final /1 (mate 1) or /2 (mate 2) taken off
void merge_label_key(const char *label, int mate, const char *&begin, uint64_t &len);

}  // namespace rtx

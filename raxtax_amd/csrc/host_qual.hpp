// The quality filter's host functions that rtx_qual.hip shares with host_qual.cpp (rtx_math.hpp has the arithmetic).
#pragma once

#include <cstdint>

#include "raxtax_hip.h"
#include "rtx_math.hpp"

namespace rtx {

void qual_cfg_init(QualCfg &c, const rtx_qual_params &p);  // the parameters as the integers that are compared (checked before: qual_check_params)
// dst[i] = quals[i] | 0x80 where bases[i] is none of 1, 2, 4, 8; returns the OR of the quality bytes (bit 7: a byte of 128 or more)
uint8_t qual_stage(const uint8_t *bases, const uint8_t *quals, uint64_t n, uint8_t *dst);

}  // namespace rtx

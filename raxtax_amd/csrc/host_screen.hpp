// The contaminant screen's host objects that rtx_screen.hip and host_front.cpp share with host_screen.cpp (rtx_math.hpp has the arithmetic).
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "raxtax_hip.h"
#include "rtx_math.hpp"

namespace rtx {

// The table of a set (include/raxtax_hip.h has its layout), immutable once built
struct ScreenSetData {
    std::vector<ScreenSlot> slots;  // m = 1 << log2m
    uint32_t log2m = 0;
    uint64_t n_keys = 0, max_disp = 0, n_wrapped = 0, fingerprint = 0;
    ScreenTable table() const { return ScreenTable{slots.data(), log2m}; }
};

int screen_check_params(const char *who, const rtx_screen_params *p);  // RTX_OK, or RTX_ERR_INVALID with the field named
uint64_t screen_fingerprint(const ScreenSetData &set, const rtx_screen_params &p);  // of the keys and the two parameters; never 0

}  // namespace rtx

// A set is shared by whoever holds it: the caller's object, the handles it was set on (rtx_index_set_screen)
struct rtx_screen_set {
    std::shared_ptr<const rtx::ScreenSetData> data;
};

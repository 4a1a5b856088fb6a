// The consensus taxonomy of the OTUs on the host (rtx_otu_taxonomy; raxtax_hip.h, "Consensus taxonomy of the OTUs"): the result object that
// rtx_otu_taxonomy (rtx_otutax.hip) and rtx_otu_taxonomy_host fill, the checks and the member lists they share, the host restatement of the
// definition, the text, and the records of a download (rtx_result_best_lineages).  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <vector>

#include "rtx_internal.hpp"

struct rtx_otutax {
    uint64_t n_rows = 0, n_otus = 0;
    uint32_t n_nodes = 0, agree_pct = 51, stride = 1;
    std::vector<uint64_t> sizes, members, classified;  // [n_otus]
    std::vector<uint32_t> depth, node;                 // [n_otus]
    std::vector<uint8_t> seed_rel;                     // [n_otus]
    std::vector<uint64_t> clade, conf;                 // [n_otus x stride]
    uint64_t packed_waves = 0, big_otus = 0;           // the device's plan
    double seconds[4] = {0, 0, 0, 0};                  // checks, plan and upload; path kernel; consensus kernels; download (rtx_otu_taxonomy_times)
};

namespace rtx {

// What a call is given, checked (otutax_open), with what both entries derive from it
struct OtuTaxInput {
    uint64_t n_rows = 0, n_otus = 0;
    const uint32_t *otu = nullptr, *seed = nullptr;
    const uint64_t *weight = nullptr;
    rtx_lineage_records rec{};
    uint32_t n_nodes = 0;
    const uint32_t *parent = nullptr;
    uint32_t agree_pct = 51;
    uint32_t max_l = 1;                  // the deepest L present, at least 1: the stride of paths and results
    std::vector<uint64_t> mem_off;       // [n_otus + 1] the members of OTU k: mem_row[mem_off[k] .. mem_off[k + 1]), in rank order
    std::vector<uint32_t> mem_row;       // [n_rows]
    std::vector<uint64_t> sizes;         // [n_otus] S_k
};

// Every refusal of the definition (RTX_ERR_INVALID with the error text set, `who` in front), then the member lists by a counting sort of otu[]
// and the sizes.  *out is set to null first.
int otutax_open(const char *who, uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed, const rtx_lineage_records *rec,
                const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out, OtuTaxInput &in);
// the fields both entries fill alike: counts, sizes, members, the arrays at their lengths and zero
void otutax_init(rtx_otutax &t, const OtuTaxInput &in);

}  // namespace rtx

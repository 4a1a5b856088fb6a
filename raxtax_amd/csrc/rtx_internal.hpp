// Internal declarations shared by the host-side C++ and the HIP translation unit of
// libraxtax_hip.so.  Not part of the ABI (include/raxtax_hip.h is).
#pragma once

#include <atomic>
#include <cstdint>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "raxtax_hip.h"

namespace rtx {

void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

constexpr uint32_t kNoNode = 0xFFFFFFFFu;

// Host thread budget (host_threads.cpp): CPUs of the affinity mask capped by the cgroup CPU quota -- what
// std::thread::available_parallelism gives the reference's rayon pool (main.rs:40-57) -- and a worker count for a pool that wants
// up to `want` threads while `sharers` handles of this process (rtx_raxtax_multi) and host_share() ranks on this host
// (rtx_set_host_share / LOCAL_WORLD_SIZE) work side by side.  Never std::thread::hardware_concurrency(): it ignores the quota.
unsigned available_parallelism();
unsigned host_share();
unsigned host_threads(unsigned want, unsigned sharers = 1);

// (rtx_api_index.hip) the device of a handle; a handle that shares its device with another one driven beside it runs on one stream
int index_device(const rtx_index *index);
void index_set_shared_device(rtx_index *index, bool shared);
uint32_t index_swap_min_subs(rtx_index *index, uint32_t v);  // returns the previous value
uint32_t index_swap_run_ahead(rtx_index *index, uint32_t v);
bool index_strand(const rtx_index *index);  // RTX_OPT_STRAND
bool index_nearest(const rtx_index *index);  // RTX_OPT_NEAREST
bool index_identity(const rtx_index *index);  // RTX_OPT_IDENTITY
bool index_profile(const rtx_index *index, uint32_t *cutoff_hundredths, uint32_t *flags);  // a taxon profile is open (rtx_index_profile_begin), with what
bool index_derep(const rtx_index *index);  // RTX_OPT_DEREP
// primer trimming (host_trim.cpp / rtx_trim.hip): a pattern with its codes owned; the list a handle holds (rtx_index_set_primers; empty: off)
struct TrimPrimer {
    std::vector<uint8_t> codes;
    uint32_t end = 0, max_errors = 0, window = 0;
    bool operator==(const TrimPrimer &o) const { return codes == o.codes && end == o.end && max_errors == o.max_errors && window == o.window; }
};
int trim_check_patterns(const char *who, const rtx_trim_pattern *pats, uint32_t n);  // RTX_OK, or RTX_ERR_INVALID with the pattern named
const std::vector<TrimPrimer> &index_primers(const rtx_index *index);
// sample demultiplexing (host_demux.cpp / rtx_demux.hip): a tag list with its codes owned, as a handle holds it (rtx_index_set_tags; no tags: off)
struct DemuxList {
    std::vector<std::vector<uint8_t>> codes;  // per tag
    std::vector<uint32_t> end;
    std::vector<rtx_demux_pair> pairs;
    rtx_demux_params params{0u, 0u};
    bool empty() const { return codes.empty(); }
    bool operator==(const DemuxList &o) const {
        if (codes != o.codes || end != o.end || pairs.size() != o.pairs.size() || params.max_mismatches != o.params.max_mismatches || params.max_offset != o.params.max_offset) return false;
        for (size_t i = 0; i < pairs.size(); i++)
            if (pairs[i].tag5 != o.pairs[i].tag5 || pairs[i].tag3 != o.pairs[i].tag3 || pairs[i].sample != o.pairs[i].sample) return false;
        return true;
    }
};
const DemuxList &index_tags(const rtx_index *index);
uint32_t index_profile_samples(const rtx_index *index);  // the samples of the open profile (rtx_index_profile_begin_samples), 0: none
// quality filter (host_qual.cpp / rtx_qual.hip): the checks of a parameter struct (RTX_OK, or RTX_ERR_INVALID with the field named), whether it
// filters anything, the error table (computed once), and the setting a handle holds (rtx_index_set_quality; false: off)
int qual_check_params(const char *who, const rtx_qual_params *p);
bool qual_params_on(const rtx_qual_params &p);
bool qual_params_equal(const rtx_qual_params &a, const rtx_qual_params &b);
const uint64_t *qual_table();
bool index_quality(const rtx_index *index, rtx_qual_params *params);
// chimera check (rtx_chimera.hip): the checks of a parameter struct (RTX_OK, or RTX_ERR_INVALID with the field named) and the setting a
// handle holds (rtx_index_set_chimera; false: off)
int chimera_check_params(const char *who, const rtx_chimera_params *p);
bool index_chimera(const rtx_index *index, rtx_chimera_params *params);
// contaminant screen (host_screen.cpp / rtx_screen.hip): the set and the parameters a handle holds (rtx_index_set_screen; null: off)
const rtx_screen_set *index_screen(const rtx_index *index, rtx_screen_params *params);
// distinct reads of a run (rtx_tally.hip): the object a handle holds (rtx_index_set_tally; null: off), its device and its samples
rtx_tally *index_tally(const rtx_index *index);
int tally_device(const rtx_tally *tally);
uint32_t tally_samples(const rtx_tally *tally);
bool index_device_text(const rtx_index *index);  // RTX_OPT_DEVICE_TEXT  // RTX_OPT_RUN_AHEAD, returns the previous value
bool hw_queues_for_run_ahead();  // (host_threads.cpp) GPU_MAX_HW_QUEUES reads six or more: transfers do not share a hardware queue with kernels

#ifndef RTX_NODE_TYPES_DEFINED
#define RTX_NODE_TYPES_DEFINED
enum NodeType : uint8_t { kInner = 0, kTaxon = 1, kSequence = 2 };  // src/tree.rs:181-186
#endif

struct Node {  // src/tree.rs:188-194, children as arena indices
    std::string label;
    uint64_t lo = 0, hi = 0;  // confidence_range
    NodeType type = kInner;
    std::vector<uint32_t> children;
};

struct BytesHash {
    size_t operator()(std::string_view s) const noexcept;
};

// Breadth-first flattening handed to the device (see rtx_nodes_view).
struct FlatNodes {
    std::vector<uint32_t> begin, end, first_child, n_children, parent, depth;
    std::vector<uint8_t> type;
    uint32_t size() const { return (uint32_t)begin.size(); }
    uint32_t max_depth = 0;
};

// Builds parent/depth from first_child/n_children; validates the arrays.  Returns false
// (with set_error) if they do not describe a BFS-ordered tree rooted at node 0.
bool derive_flat_nodes(uint64_t n_refs, uint32_t n_nodes, const uint32_t *begin, const uint32_t *end,
                       const uint32_t *first_child, const uint32_t *n_children, const uint8_t *type,
                       FlatNodes &out);

}  // namespace rtx

namespace rtx {
inline uint64_t next_tree_uid() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1);
}
}  // namespace rtx

// Host mirror of `Tree` (src/tree.rs:36-43).
struct rtx_tree {
    const uint64_t uid = rtx::next_tree_uid();  // distinct for every tree of the process (a freed tree's address may come back)
    uint64_t n = 0;         // input sequences
    uint64_t num_tips = 0;  // Tree.num_tips
    std::vector<std::string> lineages;  // sorted (tree.rs:53-54,128-129)
    std::vector<uint64_t> orig_idx;     // sorted index -> input index
    std::vector<uint8_t> seq_bytes;     // sequences in sorted order
    std::vector<uint64_t> seq_off;
    std::vector<uint64_t> csr_off;      // 65537, Tree.k_mer_map
    std::vector<uint32_t> postings;
    std::unordered_map<std::string_view, std::vector<uint32_t>, rtx::BytesHash> sequences;  // Tree.sequences
    std::vector<rtx::Node> nodes;       // arena, root = 0 (Tree.root)
    rtx::FlatNodes flat;
};

struct rtx_queries {
    std::vector<std::string> labels;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> base_off{0};
    std::vector<uint8_t> quals;  // FASTQ: the quality bytes as they stand in the file, indexed like bases (rtx_queries_quals)
    bool fastq = false;
    bool merged = false;         // made by rtx_merge_queries: the per-pair report (rtx_queries_merge_report), indexed like labels
    std::vector<uint32_t> mg_nf, mg_nr, mg_overlap, mg_diffs, mg_verdict;
};

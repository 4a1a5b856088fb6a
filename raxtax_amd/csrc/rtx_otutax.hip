// The consensus taxonomy of the OTUs on the device (rtx_otu_taxonomy; raxtax_hip.h, "Consensus taxonomy of the OTUs"): per OTU the walk from the
// root to the deepest node that P percent of the OTU's reads reach, P > 50, with the exact clade and conf sums of every level.
//   1 path      a lane per row: path[r][0 .. L) from node[r] up over node_parent (stride = the deepest L of the call).  The paths are chains
//               of one tree, so a member is on the consensus path down to level d iff its node at level d - 1 is the consensus node there:
//               one compare, no state per member.
//   2 consensus the host lays the members out per OTU (rank order) and packs consecutive OTUs of at most 64 members into one wave while
//               their members total at most 64 -- most OTUs of a run are singletons -- so that a packed wave reads one contiguous range of
//               the member list and the segment heads fall where the OTU changes from one lane to the next; every larger OTU takes a
//               workgroup of 256 threads of its own.  Per level d:
//                 first pass   every member still on the path names (path[r][d], w_r); the pairs are reduced to one candidate by a
//                              one-counter majority summary (Boyer-Moore / Misra-Gries): equal candidates add their weights, different ones
//                              leave the heavier with the difference, equal weights leave nothing.  Packed: a segmented scan over the wave
//                              with shuffles.  Workgroup: a strided loop, a wave reduction, one LDS step across the four waves.
//                 second pass  the candidate's clade and conf, summed exactly in 64 bits, then clade x 100 >= P x S_k; the walk stops where
//                              it fails.
//               If a majority exists (a node with more than half of the weight that takes part, and P x S_k is more than half of S_k, which
//               is at least that weight) it is the candidate whatever the order of the merges; if none exists every candidate fails the exact
//               test.  Either way the result does not depend on the scheduling.  The loop over the levels ends when no OTU of the wave is
//               still walking (wave-uniform; in a workgroup every thread holds the same sums).
//               seed_rel comes from the seed row's path in the same launch: the lane that writes an OTU's result compares level by level.
//               No atomics: one lane per OTU writes that OTU's result.
#include "host_otutax.hpp"
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kTaxThreads = 256;
constexpr uint32_t kPackMax = 64;  // members of a packed wave, and of an OTU that may be packed

struct OtuTaxParams {
    uint32_t n_rows, n_otus, n_nodes, stride, hund_stride, pct;
    const uint32_t *parent;    // [n_nodes]
    const uint32_t *node;      // [n_rows] the records
    const uint8_t *kind, *L;   // [n_rows]
    const uint8_t *hund;       // [n_rows][hund_stride]
    const uint64_t *weight;    // [n_rows]
    uint32_t *path;            // [n_rows][stride]
    const uint64_t *mem_off;   // [n_otus + 1]
    const uint32_t *mem_row;   // [n_rows]
    const uint32_t *otu;       // [n_rows]
    const uint64_t *sizes;     // [n_otus]
    const uint32_t *seed;      // [n_otus]
    const uint2 *waves;        // [n_waves] the OTUs [x, y) of a packed wave
    uint32_t n_waves;
    const uint32_t *big;       // [n_big] the OTUs with a workgroup of their own
    uint32_t *out_depth, *out_node;   // [n_otus]
    uint8_t *out_rel;                 // [n_otus]
    unsigned long long *out_classified, *out_clade, *out_conf;  // [n_otus], [n_otus][stride] twice (zeroed)
};

__global__ __launch_bounds__(kTaxThreads) void otutax_path_kernel(OtuTaxParams p) {
    const uint32_t r = blockIdx.x * kTaxThreads + threadIdx.x;
    if (r >= p.n_rows) return;
    uint32_t d = min((uint32_t)p.L[r], p.stride);
    if (d == 0u) return;  // (no path: the node is not read)
    uint32_t v = p.node[r];
    uint32_t *path = p.path + (size_t)r * p.stride;
    while (d-- > 0u) {
        path[d] = v;
        v = v < p.n_nodes ? p.parent[v] : kNone;  // (the host has checked the depth of every node: never out of the table)
    }
}

// the one-counter summary: (candidate, weight), kNone with 0 for nothing
struct Summary {
    uint32_t c;
    unsigned long long n;
};
__device__ __forceinline__ Summary merge(Summary a, Summary b) {
    if (a.c == b.c) return Summary{a.c, a.n + b.n};
    if (a.n == b.n) return Summary{kNone, 0ull};
    return a.n > b.n ? Summary{a.c, a.n - b.n} : Summary{b.c, b.n - a.n};
}
__device__ __forceinline__ Summary summary_of(bool on, uint32_t c, unsigned long long w) { return on ? Summary{c, w} : Summary{kNone, 0ull}; }

// Inclusive scans over the lanes of a segment [start, lane]: the last lane of a segment holds the segment's total
__device__ __forceinline__ unsigned long long seg_scan_sum(unsigned long long v, uint32_t lane, uint32_t start) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= start + d) v += o;
    }
    return v;
}
__device__ __forceinline__ Summary seg_scan_summary(Summary v, uint32_t lane, uint32_t start) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        Summary o;
        o.c = (uint32_t)__shfl_up((int)v.c, d, 64);
        o.n = __shfl_up(v.n, d, 64);
        if (lane >= start + d) v = merge(o, v);
    }
    return v;
}

// what the seed row says of the consensus so far (the writing lane alone): it diverges once its node at a level is not the consensus node
struct SeedWatch {
    uint32_t ls;
    const uint32_t *path;
    bool diverged;
    __device__ void open(const OtuTaxParams &p, uint32_t k) {
        const uint32_t s = p.seed[k];
        ls = p.L[s];
        path = p.path + (size_t)s * p.stride;
        diverged = false;
    }
    __device__ void level(uint32_t d, uint32_t cons) {
        if (d < ls && path[d] != cons) diverged = true;
    }
    __device__ uint32_t rel(uint32_t depth) const { return diverged ? 3u : (ls == depth ? 0u : (ls > depth ? 1u : 2u)); }
};

// A packed wave: the lanes take the members of the OTUs [k0, k1) in the order of the member list, at most 64
__global__ __launch_bounds__(kTaxThreads) void otutax_packed_kernel(OtuTaxParams p) {
    const uint32_t lane = rtx::lane_id();
    const uint32_t wv = blockIdx.x * (kTaxThreads / 64u) + (threadIdx.x >> 6);
    if (wv >= p.n_waves) return;  // (wave-uniform)
    const uint2 ks = p.waves[wv];
    const uint64_t m0 = p.mem_off[ks.x], m1 = p.mem_off[ks.y];
    const bool active = m0 + lane < m1;
    uint32_t r = 0, k = kNone, l = 0;
    unsigned long long w = 0, size = 0;
    bool classified = false;
    if (active) {
        r = p.mem_row[m0 + lane];
        k = p.otu[r];
        l = p.L[r];
        w = p.weight[r];
        size = p.sizes[k];
        classified = p.kind[r] == RTX_LIN_CLASSIFIED;
    }
    const uint32_t k_before = (uint32_t)__shfl_up((int)k, 1u, 64);
    const bool head = active && (lane == 0u || k != k_before);
    const unsigned long long heads = __ballot(head), actives = __ballot(active);
    // the segment of the lane: from the last head at or below it to the lane in front of the next head (or the last active lane)
    const unsigned long long below = heads & (~0ull >> (63u - lane));
    const uint32_t start = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
    const unsigned long long above = lane == 63u ? 0ull : (heads | ~actives) & (~0ull << (lane + 1u));
    const uint32_t last = above ? (uint32_t)__ffsll((long long)above) - 2u : 63u;
    const uint32_t *path = p.path + (size_t)r * p.stride;
    const uint8_t *hund = p.hund + (size_t)r * p.hund_stride;

    const unsigned long long n_cls = __shfl(seg_scan_sum(classified ? w : 0ull, lane, start), (int)last, 64);
    SeedWatch sw{0u, nullptr, false};
    if (head) sw.open(p, k);
    bool walking = active;
    uint32_t depth = 0, cons = 0;  // the consensus so far: `depth` levels, the last of them `cons`
    for (uint32_t d = 0; d < p.stride && __ballot(walking); d++) {
        const bool alive = walking && l > d && (d == 0u || path[d - 1u] == cons);
        const uint32_t mine = alive ? path[d] : kNone;
        Summary s = seg_scan_summary(summary_of(alive, mine, w), lane, start);
        const uint32_t cand = (uint32_t)__shfl((int)s.c, (int)last, 64);
        const bool on = alive && mine == cand;
        const unsigned long long clade = __shfl(seg_scan_sum(on ? w : 0ull, lane, start), (int)last, 64);
        const unsigned long long conf = __shfl(seg_scan_sum(on ? w * hund[d] : 0ull, lane, start), (int)last, 64);
        const bool pass = walking && cand != kNone && clade * 100ull >= (unsigned long long)p.pct * size;
        if (pass) {
            if (head) {
                p.out_clade[(size_t)k * p.stride + d] = clade;
                p.out_conf[(size_t)k * p.stride + d] = conf;
                sw.level(d, cand);
            }
            depth = d + 1u;
            cons = cand;
        } else {
            walking = false;
        }
    }
    if (head) {
        p.out_depth[k] = depth;
        p.out_node[k] = cons;
        p.out_rel[k] = (uint8_t)sw.rel(depth);
        p.out_classified[k] = n_cls;
    }
}

__device__ __forceinline__ unsigned long long wave_sum_all(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// A workgroup per OTU of more than 64 members: every thread ends up with the same sums, so the walk is uniform over the workgroup
__global__ __launch_bounds__(kTaxThreads) void otutax_big_kernel(OtuTaxParams p) {
    __shared__ uint32_t lds_c[4];
    __shared__ unsigned long long lds_n[4], lds_clade[4], lds_conf[4];
    const uint32_t lane = rtx::lane_id(), wave = threadIdx.x >> 6;
    const uint32_t k = p.big[blockIdx.x];
    const uint64_t m0 = p.mem_off[k], n = p.mem_off[k + 1] - m0;
    const unsigned long long size = p.sizes[k];
    {
        unsigned long long c = 0;
        for (uint64_t i = threadIdx.x; i < n; i += kTaxThreads) {
            const uint32_t r = p.mem_row[m0 + i];
            if (p.kind[r] == RTX_LIN_CLASSIFIED) c += p.weight[r];
        }
        c = wave_sum_all(c);
        if (lane == 0u) lds_clade[wave] = c;
        __syncthreads();
        c = (lds_clade[0] + lds_clade[1]) + (lds_clade[2] + lds_clade[3]);
        if (threadIdx.x == 0u) p.out_classified[k] = c;
        __syncthreads();
    }
    SeedWatch sw{0u, nullptr, false};
    if (threadIdx.x == 0u) sw.open(p, k);
    uint32_t depth = 0, cons = 0;
    for (uint32_t d = 0; d < p.stride; d++) {
        Summary s{kNone, 0ull};
        for (uint64_t i = threadIdx.x; i < n; i += kTaxThreads) {
            const uint32_t r = p.mem_row[m0 + i];
            const uint32_t *path = p.path + (size_t)r * p.stride;
            if (p.L[r] > d && (d == 0u || path[d - 1u] == cons)) s = merge(s, Summary{path[d], p.weight[r]});
        }
#pragma unroll
        for (uint32_t o = 32; o >= 1u; o >>= 1) {  // (lane 0 ends up with the wave's summary)
            Summary t;
            t.c = (uint32_t)__shfl_down((int)s.c, o, 64);
            t.n = __shfl_down(s.n, o, 64);
            s = merge(s, t);
        }
        if (lane == 0u) { lds_c[wave] = s.c; lds_n[wave] = s.n; }
        __syncthreads();
        s = merge(merge(Summary{lds_c[0], lds_n[0]}, Summary{lds_c[1], lds_n[1]}), merge(Summary{lds_c[2], lds_n[2]}, Summary{lds_c[3], lds_n[3]}));
        const uint32_t cand = s.c;  // (the same in every thread: the same four summaries merged in the same order)
        if (cand == kNone) break;
        unsigned long long clade = 0, conf = 0;
        for (uint64_t i = threadIdx.x; i < n; i += kTaxThreads) {
            const uint32_t r = p.mem_row[m0 + i];
            const uint32_t *path = p.path + (size_t)r * p.stride;
            if (p.L[r] > d && path[d] == cand) {  // (a chain of one tree: whoever holds the candidate at level d is on the path above it)
                const unsigned long long w = p.weight[r];
                clade += w;
                conf += w * p.hund[(size_t)r * p.hund_stride + d];
            }
        }
        clade = wave_sum_all(clade);
        conf = wave_sum_all(conf);
        if (lane == 0u) { lds_clade[wave] = clade; lds_conf[wave] = conf; }
        __syncthreads();
        clade = (lds_clade[0] + lds_clade[1]) + (lds_clade[2] + lds_clade[3]);
        conf = (lds_conf[0] + lds_conf[1]) + (lds_conf[2] + lds_conf[3]);
        if (clade * 100ull < (unsigned long long)p.pct * size) break;
        if (threadIdx.x == 0u) {
            p.out_clade[(size_t)k * p.stride + d] = clade;
            p.out_conf[(size_t)k * p.stride + d] = conf;
            sw.level(d, cand);
        }
        depth = d + 1u;
        cons = cand;
    }
    if (threadIdx.x == 0u) {
        p.out_depth[k] = depth;
        p.out_node[k] = cons;
        p.out_rel[k] = (uint8_t)sw.rel(depth);
    }
}

struct OtuTaxStage : StageShell {
    DevBuf<uint32_t> d_parent, d_node, d_path, d_mem_row, d_otu, d_seed, d_big, d_depth, d_out_node;
    DevBuf<uint8_t> d_kind, d_l, d_hund, d_rel;
    DevBuf<uint64_t> d_weight, d_mem_off, d_sizes;
    DevBuf<uint2> d_waves;
    DevBuf<unsigned long long> d_sums;  // classified [n_otus] | clade [n_otus][stride] | conf [n_otus][stride]
    PinBuf<uint32_t> h_depth, h_node;
    PinBuf<uint8_t> h_rel;
    PinBuf<unsigned long long> h_sums;
};

int consensus(OtuTaxStage *st, const rtx::OtuTaxInput &in, rtx_otutax &t, double t_begin) {
    const uint64_t n = in.n_rows, no = in.n_otus;
    const uint32_t stride = in.max_l, hs = in.rec.hund_stride;
    hipStream_t s = st->stream;
    int rc;
    // the plan: packed waves over runs of small OTUs, a workgroup for every larger one
    std::vector<uint2> waves;
    std::vector<uint32_t> big;
    for (uint64_t k = 0; k < no;) {
        const uint64_t mk = in.mem_off[k + 1] - in.mem_off[k];
        if (mk > kPackMax) { big.push_back((uint32_t)k++); continue; }
        uint64_t e = k, total = 0;
        while (e < no && in.mem_off[e + 1] - in.mem_off[e] <= kPackMax && total + (in.mem_off[e + 1] - in.mem_off[e]) <= kPackMax) total += in.mem_off[e + 1] - in.mem_off[e], e++;
        waves.push_back(make_uint2((uint32_t)k, (uint32_t)e));  // (e > k: an OTU of at most 64 members fits an empty wave)
        k = e;
    }
    t.packed_waves = waves.size();
    t.big_otus = big.size();
    const size_t n_sums = (size_t)no * (1u + 2u * (size_t)stride);
    if ((rc = st->d_parent.alloc(in.n_nodes)) || (rc = st->d_node.alloc(n)) || (rc = st->d_kind.alloc(n)) || (rc = st->d_l.alloc(n)) || (rc = st->d_hund.alloc(n * hs)) ||
        (rc = st->d_weight.alloc(n)) || (rc = st->d_path.alloc(n * stride)) || (rc = st->d_mem_off.alloc(no + 1)) || (rc = st->d_mem_row.alloc(n)) || (rc = st->d_otu.alloc(n)) ||
        (rc = st->d_sizes.alloc(no)) || (rc = st->d_seed.alloc(no)) || (rc = st->d_waves.alloc(waves.size())) || (rc = st->d_big.alloc(big.size())) ||
        (rc = st->d_depth.alloc(no)) || (rc = st->d_out_node.alloc(no)) || (rc = st->d_rel.alloc(no)) || (rc = st->d_sums.alloc(n_sums)) || (rc = st->h_depth.resize(no)) ||
        (rc = st->h_node.resize(no)) || (rc = st->h_rel.resize(no)) || (rc = st->h_sums.resize(n_sums)))
        return rc;
    // (pageable sources, the plan's vectors among them: they stay alive until the stream is synchronised below, in this scope)
    RTX_HIP(hipMemcpyAsync(st->d_parent.p, in.parent, (size_t)in.n_nodes * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_node.p, in.rec.node, n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_kind.p, in.rec.kind, n, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_l.p, in.rec.L, n, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_hund.p, in.rec.hund, n * hs, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_weight.p, in.weight, n * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_mem_off.p, in.mem_off.data(), (no + 1) * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_mem_row.p, in.mem_row.data(), n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_otu.p, in.otu, n * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_sizes.p, in.sizes.data(), no * 8, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(st->d_seed.p, in.seed, no * 4, hipMemcpyHostToDevice, s));
    if (!waves.empty()) RTX_HIP(hipMemcpyAsync(st->d_waves.p, waves.data(), waves.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
    if (!big.empty()) RTX_HIP(hipMemcpyAsync(st->d_big.p, big.data(), big.size() * 4, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemsetAsync(st->d_sums.p, 0, n_sums * 8, s));
    RTX_HIP(hipMemsetAsync(st->d_path.p, 0, n * stride * 4, s));
    RTX_HIP(hipStreamSynchronize(s));
    const double t1 = now_s();
    t.seconds[0] = t1 - t_begin;

    OtuTaxParams p{};
    p.n_rows = (uint32_t)n;
    p.n_otus = (uint32_t)no;
    p.n_nodes = in.n_nodes;
    p.stride = stride;
    p.hund_stride = hs;
    p.pct = in.agree_pct;
    p.parent = st->d_parent.p;
    p.node = st->d_node.p;
    p.kind = st->d_kind.p;
    p.L = st->d_l.p;
    p.hund = st->d_hund.p;
    p.weight = st->d_weight.p;
    p.path = st->d_path.p;
    p.mem_off = st->d_mem_off.p;
    p.mem_row = st->d_mem_row.p;
    p.otu = st->d_otu.p;
    p.sizes = st->d_sizes.p;
    p.seed = st->d_seed.p;
    p.waves = st->d_waves.p;
    p.n_waves = (uint32_t)waves.size();
    p.big = st->d_big.p;
    p.out_depth = st->d_depth.p;
    p.out_node = st->d_out_node.p;
    p.out_rel = st->d_rel.p;
    p.out_classified = st->d_sums.p;
    p.out_clade = st->d_sums.p + no;
    p.out_conf = st->d_sums.p + no + no * stride;
    hipLaunchKernelGGL(otutax_path_kernel, dim3((unsigned)((n + kTaxThreads - 1u) / kTaxThreads)), dim3(kTaxThreads), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(s));
    const double t2 = now_s();
    t.seconds[1] = t2 - t1;

    if (!waves.empty()) hipLaunchKernelGGL(otutax_packed_kernel, dim3((unsigned)((waves.size() + 3u) / 4u)), dim3(kTaxThreads), 0, s, p);
    if (!big.empty()) hipLaunchKernelGGL(otutax_big_kernel, dim3((unsigned)big.size()), dim3(kTaxThreads), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipStreamSynchronize(s));
    const double t3 = now_s();
    t.seconds[2] = t3 - t2;

    RTX_HIP(hipMemcpyAsync(st->h_depth.data(), st->d_depth.p, no * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_node.data(), st->d_out_node.p, no * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_rel.data(), st->d_rel.p, no, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipMemcpyAsync(st->h_sums.data(), st->d_sums.p, n_sums * 8, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    for (uint64_t k = 0; k < no; k++) {
        if (st->h_depth[k] > stride || st->h_node[k] >= in.n_nodes || st->h_rel[k] > 3u) {
            set_error("rtx_otu_taxonomy: OTU %llu came back with depth %u, node %u, seed_rel %u", (unsigned long long)k, st->h_depth[k], st->h_node[k], st->h_rel[k]);
            return RTX_ERR_HIP;
        }
    }
    t.depth.assign(st->h_depth.data(), st->h_depth.data() + no);
    t.node.assign(st->h_node.data(), st->h_node.data() + no);
    t.seed_rel.assign(st->h_rel.data(), st->h_rel.data() + no);
    const unsigned long long *sums = st->h_sums.data();
    t.classified.assign(sums, sums + no);
    t.clade.assign(sums + no, sums + no + no * stride);
    t.conf.assign(sums + no + no * stride, sums + n_sums);
    t.seconds[3] = now_s() - t3;
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_otu_taxonomy(int device, uint64_t n_rows, const uint32_t *otu, const uint64_t *weight, uint64_t n_otus, const uint32_t *seed,
                                const rtx_lineage_records *records, const rtx_nodes_view *nodes, const rtx_otu_taxonomy_params *params, rtx_otutax **out) {
    const double t0 = now_s();
    rtx::OtuTaxInput in;
    if (const int rc = rtx::otutax_open("rtx_otu_taxonomy", n_rows, otu, weight, n_otus, seed, records, nodes, params, out, in)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto *t = new rtx_otutax();
    rtx::otutax_init(*t, in);
    int rc = RTX_OK;
    if (n_otus) {  // (no OTU: nothing to upload)
        auto *st = new OtuTaxStage();
        rc = st->open(device);
        if (!rc) rc = consensus(st, in, *t, t0);
        destroy(st);
    }
    if (rc) { delete t; return rc; }
    *out = t;
    return RTX_OK;
}

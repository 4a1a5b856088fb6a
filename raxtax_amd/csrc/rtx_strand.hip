// Both-strand mode (RTX_OPT_STRAND) and the peak of a query.  The reference classifies a read in the orientation it is given
// (raxtax.rs:39-64); a read given as its reverse complement shares next to no 8-mer with any reference.  Here the handle appends the
// reverse complement of every query to the batch on the device (revcomp_kernel: query n + q is the twin of q), the batch of 2 n queries
// runs through every stage as it is, and strand_select_kernel keeps, per query, the orientation with the larger PEAK: the largest hit
// count over the references as the probability stage sees them -- the highest non-empty bin of the histogram of prob.rs:13-19
// (peak_kernel, once per sub-batch).  Ties go to the orientation the caller gave.
#include <hip/hip_runtime.h>

#include "rtx_kernels.hpp"

namespace rtx {

// One block per query: twin[len - 1 - i] = complement(query[i]); thread 0 writes the twin's end into the offsets.
__global__ __launch_bounds__(256) void revcomp_kernel(uint8_t *bases, uint64_t *base_off, uint32_t n, uint64_t total) {
    const uint32_t q = blockIdx.x;
    if (q >= n) return;
    const uint64_t b0 = base_off[q], b1 = base_off[q + 1], len = b1 - b0;
    const uint8_t *src = bases + b0;
    uint8_t *dst = bases + total + b0;
    for (uint64_t i = threadIdx.x; i < len; i += 256u) dst[len - 1u - i] = complement_code(src[i]);
    if (threadIdx.x == 0) base_off[(uint64_t)n + 1u + q] = total + b1;
}

void launch_revcomp(hipStream_t s, uint8_t *bases, uint64_t *base_off, uint32_t n, uint64_t total) {
    if (n) hipLaunchKernelGGL(revcomp_kernel, dim3(n), dim3(256), 0, s, bases, base_off, n, total);
}

// One wave per query of the sub-batch: its histogram row from bin t down, 64 bins per step; the first non-empty bin is the peak.
__global__ __launch_bounds__(256) void peak_kernel(PeakParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.nq) return;  // wave-uniform
    const uint32_t *h = p.hist + (size_t)q * p.hstride;
    const uint32_t top = min(p.t[q], p.hstride - 1u);
    uint32_t peak = 0;
    for (uint32_t base = top; base >= 1u; base = base > 64u ? base - 64u : 0u) {  // wave-uniform
        const bool has = lane < base && h[base - lane] != 0u;  // bins base, base - 1, ..., down to 1
        const unsigned long long m = __ballot(has);
        if (m) { peak = base - (uint32_t)(__ffsll(m) - 1); break; }
    }
    if (lane == 0) p.peak[p.perm[p.q0 + q]] = peak;
}

void launch_peak(hipStream_t s, const PeakParams &p) {
    if (p.nq) hipLaunchKernelGGL(peak_kernel, dim3((p.nq + 3u) / 4u), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void strand_select_kernel(StrandParams p) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= p.n) return;
    uint32_t peak = p.status[q] == 0u ? p.peak2[q] : 0u;
    uint32_t c = q;
    if (p.both) {
        const uint32_t tw = p.n + q;
        const uint32_t peak_tw = p.status[tw] == 0u ? p.peak2[tw] : 0u;
        if (peak_tw > peak) { peak = peak_tw; c = tw; }
        p.o_status[q] = p.status[c];
        p.o_t[q] = p.t[c];
        p.o_gs[q] = p.gs[c];
        p.o_row_begin[q] = p.row_begin[c];
        p.o_row_count[q] = p.row_count[c];
    }
    p.strand[q] = c == q ? 0u : 1u;
    p.peak[q] = peak;
    if (p.nearest2) {  // RTX_OPT_NEAREST (rtx_nearest.hip): of the chosen orientation; a peak of 0 (or a status that is not RTX_Q_OK) names no reference
        p.nearest[q] = peak ? p.nearest2[c] : RTX_NO_REF;
        p.ties[q] = peak ? p.ties2[c] : 0u;
    }
}

void launch_strand_select(hipStream_t s, const StrandParams &p) {
    if (p.n) hipLaunchKernelGGL(strand_select_kernel, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
}

}  // namespace rtx

// The nearest reference of a query (RTX_OPT_NEAREST): the lowest reference whose hit count is the query's PEAK, and how many references
// share that count.  The peak is the highest non-empty bin of the histogram of prob.rs:13-19 (as peak_kernel, rtx_strand.hip), the number of
// ties is that bin; only the argmax has to be looked for, and only in ONE tile: every counting epilogue leaves the largest count of its tile
// (HitParams::tile_max; a pruned run zeroes the tiles it does not count), so the lowest tile whose largest count is the peak holds the
// answer.  That tile is scanned in what the query's epilogue left of it: (reference, count) records on the records path, else the query's
// row of the counts buffer, u16 or packed 10 bits per reference.  At most 8 KiB of low bytes and 2 KiB of high bits, or one record segment,
// per query; nothing is proportional to the number of references.  Runs beside peak_kernel, in front of the probability stage.
#include <hip/hip_runtime.h>

#include "rtx_kernels.hpp"
#include "rtx_math.hpp"

namespace rtx {

// One wave per query of the sub-batch.
__global__ __launch_bounds__(256) void nearest_kernel(NearestParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.nq) return;  // wave-uniform
    const uint32_t *h = p.hist + (size_t)q * p.hstride;
    const uint32_t top = min(p.t[q], p.hstride - 1u);
    uint32_t peak = 0;
    for (uint32_t base = top; base >= 1u; base = base > 64u ? base - 64u : 0u) {  // wave-uniform (peak_kernel)
        const bool has = lane < base && h[base - lane] != 0u;
        const unsigned long long m = __ballot(has);
        if (m) { peak = base - (uint32_t)(__ffsll(m) - 1); break; }
    }
    const uint32_t out = p.perm[p.q0 + q];
    uint32_t nearest = RTX_NO_REF, ties = 0;
    // everything below is wave-uniform up to the loads of the scans; `found` leaves through the one store at the end
    uint32_t tile = 0xFFFFFFFFu;
    if (peak) {
        const uint16_t *tmx = p.tile_max + (size_t)q * p.ntiles;
        for (uint32_t T0 = 0; T0 < p.ntiles; T0 += 64u) {
            const unsigned long long m = __ballot(T0 + lane < p.ntiles && (uint32_t)tmx[T0 + lane] == peak);
            if (m) { tile = T0 + (uint32_t)(__ffsll(m) - 1); break; }
        }
    }
    if (tile != 0xFFFFFFFFu) {
        const uint64_t left = p.n_refs - ((uint64_t)tile << 13);
        const uint32_t in_tile = left < 8192u ? (uint32_t)left : 8192u;  // references the tile holds (the last one: fewer)
        uint32_t local = 0xFFFFFFFFu;
        const uint32_t ns = p.rec_nslots ? min((uint32_t)p.rec_nslots[q], kRecMaxSlots) : 0u;
        if (ns) {  // the records path: the segment of the tile, records in ascending reference order
            const uint32_t v = lane < ns ? (uint32_t)p.rec_slots[(size_t)q * kRecMaxSlots + lane] : 0xFFFFFFFFu;
            const unsigned long long b = __ballot(v == tile);
            const uint32_t k = b ? (uint32_t)(__ffsll(b) - 1) : 0xFFFFFFFFu;
            if (k < p.rec_stride) {
                const uint32_t n = min(p.rec_cnt[(size_t)q * kRecMaxSlots + k], p.rec_seg_len);  // (a segment that overflowed holds seg_len records: the run is repeated)
                const uint32_t *seg = p.rec + ((size_t)q * p.rec_stride + k) * p.rec_seg_len;
                for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
                    const uint32_t r = i0 + lane < n ? seg[i0 + lane] : 0u;  // (count 0 is never the peak)
                    const unsigned long long m = __ballot((r >> 13) == peak);
                    if (m) { local = __shfl(r, __ffsll(m) - 1, 64) & 8191u; break; }
                }
            }
        } else {
            const uint32_t crow = p.cnt_row ? p.cnt_row[q] : q;  // 0xFFFFFFFF: the rows of the diet ran out -- nothing was stored, nothing is read
            if (crow < p.cnt_rows) {
                if (p.counts_lo) {  // packed: a lane takes 16 references = 16 low bytes and two high-bit words
                    const uint8_t *lo = p.counts_lo + (size_t)crow * p.npad + ((size_t)tile << 13);
                    const uint16_t *hi = p.counts_hi + (size_t)crow * (p.npad >> 3) + ((size_t)tile << 10);
                    for (uint32_t step = 0; nearest_lane_base(step, 0u, 16u) < in_tile; step++) {
                        const uint32_t b0 = nearest_lane_base(step, lane, 16u);
                        uint32_t m16 = 0;
                        if (b0 < in_tile) {  // (rows are padded to the lanes of the last tile, 128 references each: a lane that begins inside the tile ends inside the row)
                            const uint4 v = *reinterpret_cast<const uint4 *>(lo + b0);
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                            m16 = nearest_match16(w, *reinterpret_cast<const uint32_t *>(hi + (b0 >> 3)), peak, b0, in_tile);
                        }
                        const unsigned long long m = __ballot(m16 != 0u);
                        if (m) {
                            const int src = __ffsll(m) - 1;
                            local = nearest_lane_base(step, (uint32_t)src, 16u) + (uint32_t)(__ffs(__shfl(m16, src, 64)) - 1);
                            break;
                        }
                    }
                } else {  // u16 counts: a lane takes 8 references
                    const uint16_t *cn = p.counts + (size_t)crow * p.npad + ((size_t)tile << 13);
                    for (uint32_t step = 0; nearest_lane_base(step, 0u, 8u) < in_tile; step++) {
                        const uint32_t b0 = nearest_lane_base(step, lane, 8u);
                        uint32_t m8 = 0;
                        if (b0 < in_tile) {
                            const uint4 v = *reinterpret_cast<const uint4 *>(cn + b0);
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                            m8 = nearest_match8(w, peak, b0, in_tile);
                        }
                        const unsigned long long m = __ballot(m8 != 0u);
                        if (m) {
                            const int src = __ffsll(m) - 1;
                            local = nearest_lane_base(step, (uint32_t)src, 8u) + (uint32_t)(__ffs(__shfl(m8, src, 64)) - 1);
                            break;
                        }
                    }
                }
            }
        }
        if (local != 0xFFFFFFFFu) {
            nearest = (tile << 13) + local;
            ties = h[peak];
        }
    }
    if (lane == 0) {
        p.nearest[out] = nearest;
        p.ties[out] = ties;
    }
}

void launch_nearest(hipStream_t s, const NearestParams &p) {
    if (p.nq) hipLaunchKernelGGL(nearest_kernel, dim3((p.nq + 3u) / 4u), dim3(256), 0, s, p);
}

}  // namespace rtx

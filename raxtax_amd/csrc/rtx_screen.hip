// Contaminant screen on the device (rtx_screen_*): the 16-mers of every read looked up in a set of canonical 16-mers (include/raxtax_hip.h
// has the exact semantics and the table's layout; rtx_math.hpp the arithmetic, shared with rtx_screen_read on the host and the x86 emulator).
// Like rtx_qual the stage stands IN FRONT of a handle (host_front.cpp; rtx_index_set_screen): an object of its own with one stream and its own
// buffers, so that the lookup thread of rtx_raxtax can run it on chunk c + 1 while the handle on that device classifies chunk c.
//
// One byte per base of the input ranges travels, the 4-bit code as given: the host's staging is one memcpy per read into pinned memory.
// Every range starts at a multiple of 16 bytes of the staged array (at most 15 bytes of padding per read, never taken as data), so that
// every load is a whole aligned 16-byte piece; a uint32 offset (in pieces) and a uint32 length per read go with it.
//   screen_kernel  a group of 16 lanes per read, four reads per wave, 16 reads per block.  A lane's piece is 16 consecutive window positions:
//                it loads the 16 bytes they start in and the 16 behind them (the 15 bases beyond its piece; the neighbour's piece, from L1),
//                rolls the forward and the reverse-complement word over the 31 bases in registers -- two shifts per base -- with a counter
//                of valid codes that any code but 1, 2, 4, 8 resets, and walks one probe chain per valid window into the table in global
//                memory (8 bytes per slot: a PhiX-sized set is 128 KiB, L2-resident).  A step is 16 pieces = 256 positions of a read: a
//                250-base read takes one step, a 658-base barcode three; nothing is carried from piece to piece, so every lane runs its
//                own steps and keeps its own counts and its first hit.  Behind the loop windows and hits are summed and the lowest
//                hitting position is a minimum over the 16 lanes (DPP row operations, rtx_wave.hpp); its source comes from the lane
//                that holds it.  Lane 0 of the group stores the five results.  Vector stores and plain C++, no atomics.
#include "rtx_stage.hpp"
#include "rtx_wave.hpp"
#include "host_screen.hpp"

namespace {

struct ScreenParams {
    const uint8_t *bytes;          // the staged ranges; read q at 16 * off16[q]
    const uint32_t *off16, *len;   // [n]
    ScreenTable table;
    uint32_t *out;                 // windows | hits | first | source | verdict, [n] each
    uint32_t n, min_hits, min_pct;
};

__global__ __launch_bounds__(256) void screen_kernel(ScreenParams p) {
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (kScreenGroup - 1u);
    const uint32_t q = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (64u / kScreenGroup) + lane / kScreenGroup;
    const bool mine = q < p.n;
    uint32_t len = 0;
    const uint4 *row = nullptr;
    if (mine) {
        len = p.len[q];
        row = reinterpret_cast<const uint4 *>(p.bytes + (size_t)p.off16[q] * kScreenPiece);
    }
    constexpr uint32_t kStep = kScreenGroup * kScreenPiece;
    ScreenAcc acc{0u, 0u, kScreenNone, kScreenNone};
    // (a piece whose first position leaves no room for a window holds none: pos + 16 <= len)
    for (uint32_t pos = gl * kScreenPiece; pos + kScreenK <= len; pos += kStep) {
        const uint32_t k = pos / kScreenPiece;
        const uint4 va = row[k];  // (inside the read's padded range: pos < len)
        ScreenWords b{{0u, 0u, 0u, 0u}};
        if (pos + kScreenPiece < len) {
            const uint4 vb = row[k + 1u];
            b = ScreenWords{{vb.x, vb.y, vb.z, vb.w}};
        }
        screen_piece(p.table, ScreenWords{{va.x, va.y, va.z, va.w}}, b, pos, len, acc);
    }
    // (all 64 lanes are back here: the row operations read every lane of the group)
    const uint32_t windows = rtx::row16_sum_u32(acc.windows), hits = rtx::row16_sum_u32(acc.hits), first = rtx::row16_min_u32(acc.first);
    const uint32_t source = rtx::row16_min_u32(acc.first == first ? acc.source : kScreenNone);  // (positions differ from lane to lane: one holder, or none)
    if (mine && gl == 0u) {
        p.out[q] = windows;
        p.out[(size_t)p.n + q] = hits;
        p.out[2u * (size_t)p.n + q] = first;
        p.out[3u * (size_t)p.n + q] = source;
        p.out[4u * (size_t)p.n + q] = screen_verdict(hits, windows, p.min_hits, p.min_pct);
    }
}

}  // namespace

struct rtx_screen : StageShell {
    rtx_screen_params params{};
    uint32_t log2m = 0;
    DevBuf<ScreenSlot> d_table;
    DevBuf<uint8_t> d_bytes;
    DevBuf<uint32_t> d_in, d_out;             // off16 | len; windows | hits | first | source | verdict
    PinBuf<uint8_t> h_bytes;
    PinBuf<uint32_t> h_in, h_out;
};

namespace rtx {
const rtx_screen_set *index_screen(const rtx_index *index, rtx_screen_params *params) {
    if (params) *params = index->screen;
    return index->screen_set.data ? &index->screen_set : nullptr;
}
}  // namespace rtx

extern "C" {

int rtx_screen_create(int device, const rtx_screen_set *set, const rtx_screen_params *params, rtx_screen **out) {
    if (!out || !params || !set || !set->data) { set_error("rtx_screen_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (const int rc = rtx::screen_check_params("rtx_screen_create", params)) return rc;
    if (const int rc = check_device(device)) return rc;
    auto s = new rtx_screen();
    s->params = *params;
    s->log2m = set->data->log2m;
    if (const int rc = s->open(device)) { delete s; return rc; }
    const std::vector<ScreenSlot> &slots = set->data->slots;
    if (s->d_table.alloc(slots.size()) != RTX_OK ||
        hipMemcpy(s->d_table.p, slots.data(), sizeof(ScreenSlot) * slots.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("rtx_screen_create: the table of %zu slots could not be uploaded", slots.size());
        delete s;
        return RTX_ERR_HIP;
    }
    *out = s;
    return RTX_OK;
}

void rtx_screen_destroy(rtx_screen *s) { destroy(s); }

int rtx_screen_run(rtx_screen *s, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *lo_in, const uint32_t *hi_in,
                   uint32_t *windows, uint32_t *hits, uint32_t *first, uint32_t *source, uint32_t *verdict) {
    if (!s) { set_error("rtx_screen_run: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (n > 0x0FFFFFF0ull) { set_error("rtx_screen_run: %llu reads in one batch (at most 2^28 - 16)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !windows || !hits || !first || !source || !verdict || (lo_in == nullptr) != (hi_in == nullptr)) { set_error("rtx_screen_run: null argument"); return RTX_ERR_INVALID; }
    s->begin();
    int rc;
    if ((rc = s->h_in.resize(2 * n))) return rc;
    uint32_t *h_off = s->h_in.data(), *h_len = h_off + n;
    uint64_t pieces = 0;
    if ((rc = rtx::layout_ranges("rtx_screen_run", n, base_off, lo_in, hi_in, RTX_SCREEN_MAX_READ, kScreenPiece, h_off, h_len, &pieces))) return rc;
    if (pieces && !bases) { set_error("rtx_screen_run: null bases"); return RTX_ERR_INVALID; }
    RTX_HIP(hipSetDevice(s->device));
    const size_t bytes = (size_t)pieces * kScreenPiece;
    if ((rc = s->h_bytes.resize(bytes + 16)) || (rc = s->h_out.resize(5 * n)) || (rc = grow(s->d_bytes, bytes + 16)) || (rc = grow(s->d_in, 2 * n)) ||
        (rc = grow(s->d_out, 5 * n)))
        return rc;
    uint8_t *hb = s->h_bytes.data();
    rtx::parallel_ranges(n, rtx::host_threads(4u), 4096, [&](unsigned, uint64_t a, uint64_t b) {
        for (uint64_t r = a; r < b; r++)
            if (h_len[r]) memcpy(hb + (size_t)h_off[r] * kScreenPiece, bases + base_off[r] + (lo_in ? lo_in[r] : 0u), h_len[r]);
    });
    s->staged();
    hipStream_t st = s->stream;
    if (bytes) RTX_HIP(hipMemcpyAsync(s->d_bytes.p, hb, bytes, hipMemcpyHostToDevice, st));
    RTX_HIP(hipMemcpyAsync(s->d_in.p, h_off, 2 * n * 4, hipMemcpyHostToDevice, st));
    ScreenParams p{};
    p.bytes = s->d_bytes.p;
    p.off16 = s->d_in.p;
    p.len = s->d_in.p + n;
    p.table = ScreenTable{s->d_table.p, s->log2m};
    p.out = s->d_out.p;
    p.n = (uint32_t)n;
    p.min_hits = s->params.min_hits;
    p.min_pct = s->params.min_pct;
    const unsigned per_block = 4u * (64u / kScreenGroup);
    RTX_HIP(hipEventRecord(s->ev0, st));
    hipLaunchKernelGGL(screen_kernel, dim3((unsigned)((n + per_block - 1u) / per_block)), dim3(256), 0, st, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipEventRecord(s->ev1, st));
    RTX_HIP(hipMemcpyAsync(s->h_out.data(), s->d_out.p, 5 * n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = s->wait())) return rc;
    scatter_columns(s->h_out.data(), n, {windows, hits, first, source, verdict});
    s->finish();
    return RTX_OK;
}

int rtx_screen_kernel_time(const rtx_screen *s, float *ms) { return kernel_time("rtx_screen_kernel_time", s, ms); }

int rtx_screen_stage_times(const rtx_screen *s, double seconds[3]) { return stage_times("rtx_screen_stage_times", s, seconds); }

int rtx_index_set_screen(rtx_index *index, const rtx_screen_set *set, const rtx_screen_params *params) {
    if (!index) { set_error("rtx_index_set_screen: null index"); return RTX_ERR_INVALID; }
    if (!set) {  // honoured by the host mirror alone (host_front.cpp): nothing else of the handle changes
        index->screen_set.data.reset();
        index->screen = rtx_screen_params{};
        return RTX_OK;
    }
    if (!set->data) { set_error("rtx_index_set_screen: an empty set"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::screen_check_params("rtx_index_set_screen", params)) return rc;
    index->screen_set.data = set->data;  // (shared: the caller may free the set)
    index->screen = *params;
    return RTX_OK;
}

int rtx_index_screen(const rtx_index *index, rtx_screen_params *params, int *on, uint64_t *fingerprint) {
    if (!index || !params || !on) { set_error("rtx_index_screen: null argument"); return RTX_ERR_INVALID; }
    const rtx_screen_set *set = rtx::index_screen(index, params);
    *on = set ? 1 : 0;
    if (fingerprint) *fingerprint = set ? rtx::screen_fingerprint(*set->data, *params) : 0ull;
    return RTX_OK;
}

}  // extern "C"

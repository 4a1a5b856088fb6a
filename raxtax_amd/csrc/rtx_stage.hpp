// The shell of a front stage object (rtx_trim, rtx_demux, rtx_qual, rtx_screen, rtx_merge, rtx_chimera, rtx_derep): its device, its one stream,
// the event pair around its kernel, its times, and the staging that more than one stage does in the same way.  A stage file keeps what is its
// own: the kernel and its parameters, the launch geometry, the buffer list and the order of what it enqueues.  Not part of the ABI.
#pragma once

#include <initializer_list>

#include "host_stage.hpp"
#include "rtx_index.hpp"

namespace rtxi {

// `device` exists and is a gfx950: RTX_OK with it current, or RTX_ERR_NO_DEVICE (there is no CPU fallback)
inline int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("no usable HIP device (requested %d of %d); libraxtax_hip has no CPU fallback", device, ndev);
        return RTX_ERR_NO_DEVICE;
    }
    RTX_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    RTX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
        return RTX_ERR_NO_DEVICE;
    }
    return RTX_OK;
}

// A buffer that only grows, with headroom, so that batches of one size allocate once
template <class T>
int grow(DevBuf<T> &b, size_t count) {
    if (b.p && count <= b.n) return RTX_OK;
    return b.alloc(count + count / 4 + 64);
}

// One stream (non-blocking, no priority) and buffers that only grow: nothing is freed between runs, a hipFree would stall the handle that
// classifies beside the stage.  A stage derives from the shell; its buffers are its own members.
struct StageShell {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the kernel (rtx_*_kernel_time); rtx_derep never records them: two idle events read simpler than a flag
    float kernel_ms = 0.f;
    double times[3] = {0, 0, 0};              // staging, copies and wait, the whole call (rtx_*_stage_times)
    double t0 = 0, t1 = 0;
    StageShell() = default;
    StageShell(const StageShell &) = delete;
    int open(int dev) {  // (the device is current: check_device, or the handle's)
        device = dev;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) {
            set_error("hipStreamCreate / hipEventCreate failed");
            return RTX_ERR_HIP;
        }
        return RTX_OK;
    }
    ~StageShell() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
    double begin() { return t0 = now_s(); }  // a run starts
    void staged() { t1 = now_s(); }          // the host has laid out what travels
    int wait() {                             // everything enqueued is done; the event pair -> kernel_ms
        RTX_HIP(hipStreamSynchronize(stream));
        (void)hipEventElapsedTime(&kernel_ms, ev0, ev1);
        return RTX_OK;
    }
    void finish() {                          // the results are with the caller -> times
        const double t2 = now_s();
        times[0] = t1 - t0;
        times[1] = std::max(0.0, t2 - t1 - (double)kernel_ms * 1e-3);
        times[2] = t2 - t0;
    }
};

template <class T>
void destroy(T *stage) {
    if (!stage) return;
    (void)hipSetDevice(stage->device);
    delete stage;
}

inline int kernel_time(const char *who, const StageShell *s, float *ms) {
    if (!s || !ms) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    *ms = s->kernel_ms;
    return RTX_OK;
}

inline int stage_times(const char *who, const StageShell *s, double seconds[3]) {
    if (!s || !seconds) { set_error("%s: null argument", who); return RTX_ERR_INVALID; }
    for (int i = 0; i < 3; i++) seconds[i] = s->times[i];
    return RTX_OK;
}

// The first w5 and the last w3 bases of every read (the 3' window reversed) into rows of s5 / s3 bytes (trim_stage_row; a stride of 0: that end
// is not staged), and the reads' lengths
inline void stage_end_rows(uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t w5, uint32_t s5, uint32_t w3, uint32_t s3, uint8_t *h5,
                           uint8_t *h3, uint32_t *h_len) {
    parallel_ranges(n, rtx::host_threads(4u), 4096, [=](unsigned, uint64_t a, uint64_t b) {
        for (uint64_t q = a; q < b; q++) {
            const uint8_t *x = bases + base_off[q];
            const uint64_t len = base_off[q + 1] - base_off[q];
            h_len[q] = (uint32_t)len;
            if (s5) trim_stage_row(x, len, w5, false, h5 + q * s5);
            if (s3) trim_stage_row(x, len, w3, true, h3 + q * s3);
        }
    });
}

// The reads of a batch onto the device as a handle's travel (rtx_ingest.hip): the offsets rebased to 0, the bases two per byte through pinned
// memory and unpacked to one byte per base on the device -- a batch with a byte above 15 is no code and travels as it is -- with 64 zero bytes
// behind the end (em_load_word and the k-mer windows read past it).  The buffers are sized by the caller: total + 64 bytes, n + 1 offsets.
inline int upload_packed_reads(hipStream_t s, uint64_t n, const uint8_t *bases, const uint64_t *base_off, PinBuf<uint8_t> &h_packed, PinBuf<uint64_t> &h_base_off,
                               DevBuf<uint8_t> &d_packed, DevBuf<uint64_t> &d_base_off, DevBuf<uint8_t> &d_bases) {
    const uint64_t total = base_off[n] - base_off[0];
    for (uint64_t q = 0; q <= n; q++) h_base_off[q] = base_off[q] - base_off[0];
    const bool packed = total == 0 || rtx::pack_nibbles_mt(bases + base_off[0], total, h_packed.data(), rtx::host_threads(4u));
    if (!packed) std::memcpy(h_packed.data(), bases + base_off[0], total);
    if (total) RTX_HIP(hipMemcpyAsync(d_packed.p, h_packed.data(), packed ? (total + 1) / 2 : total, hipMemcpyHostToDevice, s));
    RTX_HIP(hipMemcpyAsync(d_base_off.p, h_base_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (packed) {
        rtx::launch_unpack_nibbles(s, d_packed.p, d_bases.p, total, total + 64);
    } else {
        if (total) RTX_HIP(hipMemcpyAsync(d_bases.p, d_packed.p, total, hipMemcpyDeviceToDevice, s));
        RTX_HIP(hipMemsetAsync(d_bases.p + total, 0, 64, s));
    }
    return RTX_OK;
}

// The result columns of n uint32 each, back to back in the pinned buffer, into the caller's arrays
inline void scatter_columns(const uint32_t *h_out, uint64_t n, std::initializer_list<uint32_t *> cols) {
    for (uint32_t *c : cols) {
        std::memcpy(c, h_out, n * 4);
        h_out += n;
    }
}

}  // namespace rtxi

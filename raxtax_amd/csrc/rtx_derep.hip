// Dereplication on the device (rtx_derep_*): which queries of a batch are byte-for-byte copies of an earlier one.  Amplicon runs hold the
// same read many times over (what `vsearch --derep_fulllength` is run for in front of a classifier); the result of a query never depends on
// the rest of its batch, so a copy need not be classified at all.  The stage stands IN FRONT of a handle (host_raxtax.cpp: RTX_OPT_DEREP):
// an object of its own with one stream and its own buffers, so that the lookup thread of rtx_raxtax can run it on chunk c + 1 while the
// handle on that device classifies chunk c.
//
// The bases travel as a handle's do (rtx_ingest.hip: two per byte through pinned memory, unpacked to one byte per base on the device; a
// batch with a byte above 15 as it is), then three kernels:
//   hash     one wave per query: the 64-bit hash of rtx_exact.hip over the 8-byte words of the sequence (em_mix_word / em_finish)
//   insert   one wave per query: linear probing in an open-addressing table of 2^bits >= 2 n slots that hold query + 1.  An empty slot is
//            claimed with a compare-and-swap; an occupant with the same hash and length is compared word by word -- the hash is a
//            pre-filter, the bytes decide, always.  An equal occupant becomes the query's OWNER; a query that claims a slot owns itself.
//            Which copy owns a cluster depends on the scheduling, so every member also lowers cluster_min[owner] to its own index.
//            No wave ever waits for another: a slot goes from empty to occupied once and never changes again, a lost compare-and-swap
//            returns the occupant, the table is at most half full.
//   resolve  rep[q] = cluster_min[owner[q]]: the lowest index with q's sequence, whatever the scheduling was; the queries with
//            rep[q] == q are counted, a ballot and one atomic per wave.
// Identical queries probe the same slots in the same order and slots are never vacated: the second one to arrive meets the first before
// it can meet an empty slot, so a cluster has exactly one owner.
#include <atomic>

#include "rtx_derep_dev.hpp"
#include "rtx_stage.hpp"

namespace {

std::atomic<uint64_t> g_derep_hash_mask{~0ull};  // RTX_DEFAULT_DEREP_HASH_MASK (tests: a hash of two bits, so that every probe ends in the byte compare)

// (the device code of the three steps is in rtx_derep_dev.hpp: rtx_tally.hip runs the last two over the reads its own table does not know)
__global__ __launch_bounds__(256) void derep_hash_kernel(DerepParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.n) return;  // wave-uniform
    const uint64_t b0 = p.base_off[q], len = p.base_off[q + 1] - b0;
    const uint64_t h = derep_hash_read(p.bases + b0, len, lane);
    if (lane == 0) p.hash[q] = h & p.hash_mask;
}

__global__ __launch_bounds__(256) void derep_insert_kernel(DerepParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.n) return;  // wave-uniform
    derep_insert_read(p, q, lane);
}

// (no lane leaves early: the ballot runs over whole waves)
__global__ __launch_bounds__(256) void derep_resolve_kernel(DerepParams p) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool self = false;
    if (q < p.n) {
        const uint32_t r = derep_resolve_read(p, q);
        p.rep[q] = r;
        self = r == q;
    }
    const unsigned long long m = __ballot(self);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(p.rep + p.n, (uint32_t)__popcll(m));
}

}  // namespace

namespace rtxi {
void set_derep_hash_mask(uint64_t mask) { g_derep_hash_mask.store(mask); }
}  // namespace rtxi

struct rtx_derep : StageShell {  // (its events are never recorded: there is no rtx_derep_kernel_time)
    DevBuf<uint8_t> d_packed, d_bases;
    DevBuf<uint64_t> d_base_off, d_hash;
    DevBuf<uint32_t> d_table, d_owner, d_cluster_min, d_rep;
    PinBuf<uint8_t> h_packed;
    PinBuf<uint64_t> h_base_off;
    PinBuf<uint32_t> h_rep;
};

extern "C" {

int rtx_derep_create(int device, rtx_derep **out) {
    if (!out) { set_error("rtx_derep_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    if (const int rc = check_device(device)) return rc;
    auto d = new rtx_derep();
    if (const int rc = d->open(device)) { delete d; return rc; }
    *out = d;
    return RTX_OK;
}

void rtx_derep_destroy(rtx_derep *d) { destroy(d); }

int rtx_derep_run(rtx_derep *d, uint64_t n, const uint8_t *bases, const uint64_t *base_off, uint32_t *rep, uint64_t *n_unique) {
    if (!d || !n_unique) { set_error("rtx_derep_run: null argument"); return RTX_ERR_INVALID; }
    *n_unique = 0;
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFFEull) { set_error("rtx_derep_run: %llu queries in one batch (at most 2^31 - 2)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off || !rep) { set_error("rtx_derep_run: null argument"); return RTX_ERR_INVALID; }
    if (const int rc = rtx::check_reads("rtx_derep_run", n, base_off, bases, ~0ull)) return rc;
    const uint64_t total = base_off[n] - base_off[0];
    RTX_HIP(hipSetDevice(d->device));
    uint32_t bits = 1;
    while ((1ull << bits) < 2ull * n) bits++;
    const size_t slots = (size_t)1 << bits;
    int rc;
    if ((rc = d->h_packed.resize(total + 64)) || (rc = d->h_base_off.resize(n + 1)) || (rc = d->h_rep.resize(n + 1)) || (rc = grow(d->d_packed, total + 64)) ||
        (rc = grow(d->d_bases, total + 64)) || (rc = grow(d->d_base_off, n + 1)) || (rc = grow(d->d_hash, n)) || (rc = grow(d->d_owner, n)) ||
        (rc = grow(d->d_cluster_min, n)) || (rc = grow(d->d_rep, n + 1)) || (rc = d->d_table.alloc(slots)))
        return rc;
    hipStream_t s = d->stream;
    // two bases per byte over PCIe, and 64 zero bytes behind the end: em_load_word reads past it
    if ((rc = upload_packed_reads(s, n, bases, base_off, d->h_packed, d->h_base_off, d->d_packed, d->d_base_off, d->d_bases))) return rc;
    RTX_HIP(hipMemsetAsync(d->d_table.p, 0, slots * 4, s));
    RTX_HIP(hipMemsetAsync(d->d_cluster_min.p, 0xFF, n * 4, s));
    RTX_HIP(hipMemsetAsync(d->d_rep.p + n, 0, 4, s));
    DerepParams p{d->d_bases.p, d->d_base_off.p, (uint32_t)n, d->d_hash.p, d->d_table.p, bits, g_derep_hash_mask.load(),
                  d->d_owner.p, d->d_cluster_min.p, d->d_rep.p};
    const dim3 waves((unsigned)((n + 3u) / 4u)), threads((unsigned)((n + 255u) / 256u));
    hipLaunchKernelGGL(derep_hash_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(derep_insert_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(derep_resolve_kernel, threads, dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipMemcpyAsync(d->h_rep.data(), d->d_rep.p, (n + 1) * 4, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    std::memcpy(rep, d->h_rep.data(), n * 4);
    *n_unique = d->h_rep[n];
    return RTX_OK;
}

}  // extern "C"

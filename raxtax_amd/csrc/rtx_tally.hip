// The distinct reads of a run on the device (rtx_tally_*): every distinct sequence the object was ever given, with a count per sample.  What
// `vsearch --derep_fulllength --sizeout` and `--otutabout` leave; rtx_derep.hip cannot give it, its table lives for one chunk and every
// occupant lies in that chunk's own bases.  This object persists across chunks and calls and OWNS its sequences:
//   table    open addressing, 2^tbits >= 2 x capacity slots of entry + 1 (0: empty), at most half full
//   entry    e_hash (the whole 64 bits: the mask of the day is applied where it is used), e_len, e_off into the arena
//   arena    one byte per base, every entry from a multiple of 8 bytes on and padded to one: em_load_word never leaves the entry
//   count    [entries x columns] uint32, zero behind the entries in use
//   totals   64-bit: what the scan of a chunk found (below) and overflow_reads
// The reads of a chunk travel as in rtx_derep_run.  Per chunk, on the object's one stream, separate launches -- no wave ever waits for another,
// and a slot of either table goes from empty to occupied once:
//   1 lookup   one wave per read: hash, probe the persistent table READ-ONLY; hash and length are a pre-filter, the bytes decide, always.
//              ent[q] = the entry found, or kNew; kSkip for a read of weight 0 or length 0, which nobody looks at again.
//   2 new      the reads with ent == kNew among themselves: the chunk-local insert / resolve of rtx_derep_dev.hpp, rep[q] = the lowest index
//              with q's sequence.  Those with rep[q] == q are the new distinct reads; a scan over (1, padded length) in READ order numbers
//              them: entry ids are the order of first appearance, whatever the scheduling.  A new distinct read is stored if and only if
//              its inclusive scan position fits max_entries and max_bytes (ent[q] = its id), else it overflows (ent[q] = kOverflow).
//      host    the four totals of the scan come back (new distinct reads and their bytes; of these stored); the buffers grow: new
//              allocation, device-to-device copy, the table laid out again from the stored hashes, one thread per entry with a CAS claim.
//   3 append   a stored new distinct read copies its bytes to the arena, writes hash, length, offset and claims an empty slot -- no compare:
//              the new ones differ from each other and from every occupant.  Then every read that counts adds its weight to
//              count[entry][sample] (a copy of a new read: the entry of rep[q]), or to overflow_reads.
#include <atomic>

#include "host_tally.hpp"
#include "rtx_derep_dev.hpp"
#include "rtx_stage.hpp"

namespace {

std::atomic<uint64_t> g_tally_hash_mask{~0ull};  // RTX_DEFAULT_TALLY_HASH_MASK (tests: a hash of two bits, so that every probe ends in the byte compare)

constexpr uint32_t kNew = 0xFFFFFFFFu, kSkip = 0xFFFFFFFEu, kOverflow = 0xFFFFFFFDu;  // ent[q] above every entry id (at most 2^31 - 2)
constexpr uint32_t kNoRep = 0xFFFFFFFFu;                                              // rep[q] of a read that is not new

struct Pair { uint64_t e, b; };  // entries, bytes

struct TallyParams {
    DerepParams d;                    // the chunk: bases, offsets, masked hashes, the chunk-local table, owner, cluster_min, rep
    uint64_t *hash_full;              // [n] the hash before the mask: what an entry keeps
    const uint32_t *sample, *weight;  // [n] or null (column 0, weight 1)
    uint32_t *ent;                    // [n]
    uint64_t *new_off;                // [n] at a new distinct read: its offset in the arena
    Pair *block_sum;                  // [ceil(n / 256)] of the scan
    uint64_t *totals;                 // [0] new distinct reads of the chunk [1] their padded bytes [2] of these stored [3] their bytes; [4] overflow_reads (persists)
    uint32_t *table;
    uint32_t tbits;
    uint64_t *e_hash;
    uint32_t *e_len;
    uint64_t *e_off;
    uint8_t *arena;
    uint32_t *count;
    uint32_t columns;
    uint64_t n_entries, n_bytes, max_entries, max_bytes;  // in use before this chunk, and the caps
};

// Inclusive scan of v over the 256 threads of the block (every thread calls); *total = the block's sum.  lds: 4 Pairs.
__device__ __forceinline__ Pair block_scan_incl(Pair v, Pair *lds, Pair *total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t e = __shfl_up(v.e, d, 64), b = __shfl_up(v.b, d, 64);
        if (lane >= (uint32_t)d) { v.e += e; v.b += b; }
    }
    if (lane == 63u) lds[w] = v;
    __syncthreads();
    Pair add{0, 0}, tot{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const Pair s = lds[k];
        if (k < w) { add.e += s.e; add.b += s.b; }
        tot.e += s.e;
        tot.b += s.b;
    }
    __syncthreads();  // (lds may be written again)
    v.e += add.e;
    v.b += add.b;
    *total = tot;
    return v;
}

__device__ __forceinline__ uint64_t padded(uint64_t len) { return (len + 7u) & ~7ull; }

// claims the first empty slot from the home slot of h on (one thread; the table is at most half full: an empty slot comes)
__device__ __forceinline__ void claim_slot(uint32_t *table, uint32_t tbits, uint64_t h, uint32_t id) {
    const uint32_t mask = (uint32_t)((1ull << tbits) - 1ull);
    uint32_t slot = em_slot(h, tbits);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        if (atomicCAS(table + slot, 0u, id + 1u) == 0u) return;
        slot = (slot + 1u) & mask;
    }
}

__global__ __launch_bounds__(256) void tally_lookup_kernel(TallyParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.d.n) return;  // wave-uniform
    const uint64_t b0 = p.d.base_off[q], len = p.d.base_off[q + 1] - b0;
    const uint32_t w = p.weight ? __builtin_amdgcn_readfirstlane(p.weight[q]) : 1u;
    if (w == 0u || len == 0u) {  // wave-uniform: nobody looks at this read again
        if (lane == 0) { p.ent[q] = kSkip; p.d.hash[q] = 0; p.hash_full[q] = 0; }
        return;
    }
    const uint8_t *seq = p.d.bases + b0;
    const uint64_t hf = derep_hash_read(seq, len, lane), h = hf & p.d.hash_mask;
    const uint32_t mask = (uint32_t)((1ull << p.tbits) - 1ull);
    uint32_t slot = em_slot(h, p.tbits), found = kNew;
    for (uint64_t probe = 0; probe <= mask; probe++) {  // wave-uniform; read-only: nothing is claimed here
        const uint32_t e = __builtin_amdgcn_readfirstlane(p.table[slot]);
        if (e == 0u) break;
        const uint32_t o = e - 1u;
        if ((p.e_hash[o] & p.d.hash_mask) == h && p.e_len[o] == len && !derep_bytes_differ(seq, p.arena + p.e_off[o], len, lane)) { found = o; break; }
        slot = (slot + 1u) & mask;
    }
    if (lane == 0) { p.ent[q] = found; p.d.hash[q] = h; p.hash_full[q] = hf; }
}

__global__ __launch_bounds__(256) void tally_insert_new_kernel(TallyParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.d.n) return;                                           // wave-uniform
    if (__builtin_amdgcn_readfirstlane(p.ent[q]) != kNew) return;     // wave-uniform
    derep_insert_read(p.d, q, lane);
}

// (1, padded length) at a new distinct read, (0, 0) elsewhere
__device__ __forceinline__ Pair first_weight(const TallyParams &p, uint32_t q, bool first) {
    if (!first) return Pair{0, 0};
    return Pair{1, padded(p.d.base_off[q + 1] - p.d.base_off[q])};
}

// (no thread leaves early in the three kernels of the scan: the block scans as a whole)
__global__ __launch_bounds__(256) void tally_resolve_kernel(TallyParams p) {
    __shared__ Pair lds[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool first = false;
    if (q < p.d.n) {
        uint32_t r = kNoRep;
        if (p.ent[q] == kNew) r = derep_resolve_read(p.d, q);
        p.d.rep[q] = r;
        first = r == q;
    }
    Pair tot;
    (void)block_scan_incl(first_weight(p, q, first), lds, &tot);
    if (threadIdx.x == 0) p.block_sum[blockIdx.x] = tot;
}

// one block: the block sums become their exclusive scan, the totals of the chunk go to totals[0 .. 1]
__global__ __launch_bounds__(256) void tally_scan_blocks_kernel(TallyParams p, uint32_t n_blocks) {
    __shared__ Pair lds[4];
    Pair carry{0, 0};
    for (uint32_t base = 0; base < n_blocks; base += 256u) {  // block-uniform
        const uint32_t i = base + threadIdx.x;
        const Pair v = i < n_blocks ? p.block_sum[i] : Pair{0, 0};
        Pair tot;
        const Pair inc = block_scan_incl(v, lds, &tot);
        if (i < n_blocks) p.block_sum[i] = Pair{carry.e + inc.e - v.e, carry.b + inc.b - v.b};
        carry.e += tot.e;
        carry.b += tot.b;
    }
    if (threadIdx.x == 0) { p.totals[0] = carry.e; p.totals[1] = carry.b; }
}

// every new distinct read learns its entry id and arena offset, or that it overflows; totals[2 .. 3] = what is stored of the chunk
__global__ __launch_bounds__(256) void tally_number_kernel(TallyParams p) {
    __shared__ Pair lds[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const bool first = q < p.d.n && p.d.rep[q] == q;
    const Pair v = first_weight(p, q, first);
    Pair tot;
    Pair inc = block_scan_incl(v, lds, &tot);
    const Pair base = p.block_sum[blockIdx.x];
    inc.e += base.e;
    inc.b += base.b;
    // the scan runs in read order and both positions only rise: the stored reads are a prefix of the new distinct reads
    const bool stored = first && p.n_entries + inc.e <= p.max_entries && p.n_bytes + inc.b <= p.max_bytes;
    if (first) {
        p.ent[q] = stored ? (uint32_t)(p.n_entries + inc.e - 1u) : kOverflow;
        p.new_off[q] = p.n_bytes + inc.b - v.b;
    }
    const unsigned long long m = __ballot(stored);
    if (m && (threadIdx.x & 63u) == 63u - (uint32_t)__clzll((long long)m)) {  // the last stored read of the wave holds its largest positions
        atomicMax((unsigned long long *)p.totals + 2, (unsigned long long)inc.e);
        atomicMax((unsigned long long *)p.totals + 3, (unsigned long long)inc.b);
    }
}

__global__ __launch_bounds__(256) void tally_append_kernel(TallyParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= p.d.n) return;  // wave-uniform
    const uint32_t id = __builtin_amdgcn_readfirstlane(p.ent[q]);
    if (__builtin_amdgcn_readfirstlane(p.d.rep[q]) != q || id >= kOverflow) return;  // wave-uniform: not a new distinct read, or not stored
    const uint64_t b0 = p.d.base_off[q], len = p.d.base_off[q + 1] - b0, off = p.new_off[q];
    const uint8_t *seq = p.d.bases + b0;
    uint64_t *dst = reinterpret_cast<uint64_t *>(p.arena + off);  // (8-byte aligned: every offset is a sum of padded lengths)
    const uint64_t nw = (len + 7u) >> 3;
    for (uint64_t j = lane; j < nw; j += 64) dst[j] = em_load_word(seq, len, j);  // (the padding of the last word is zero)
    if (lane == 0) {
        const uint64_t hf = p.hash_full[q];
        p.e_hash[id] = hf;
        p.e_len[id] = (uint32_t)len;
        p.e_off[id] = off;
        claim_slot(p.table, p.tbits, hf & p.d.hash_mask, id);
    }
}

// (no lane leaves early: the sum runs over whole waves)
__global__ __launch_bounds__(256) void tally_count_kernel(TallyParams p) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    uint64_t over = 0;
    if (q < p.d.n) {
        uint32_t e = p.ent[q];
        if (e != kSkip) {
            const uint32_t r = p.d.rep[q];
            if (r != kNoRep) e = p.ent[r];  // a new read: the entry of its first copy (tally_number_kernel), or kOverflow
            const uint32_t w = p.weight ? p.weight[q] : 1u;
            if (e == kOverflow) over = w;
            else atomicAdd(p.count + (uint64_t)e * p.columns + (p.sample ? p.sample[q] : 0u), w);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) over += __shfl_xor(over, d, 64);
    if ((threadIdx.x & 63u) == 0u && over) atomicAdd((unsigned long long *)p.totals + 4, (unsigned long long)over);
}

// a zeroed table laid out from the stored hashes: one thread per entry
__global__ __launch_bounds__(256) void tally_rehash_kernel(uint32_t *table, uint32_t tbits, const uint64_t *e_hash, uint64_t hash_mask, uint32_t n_entries) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_entries) claim_slot(table, tbits, e_hash[i] & hash_mask, i);
}

uint32_t table_bits(uint64_t capacity) {
    uint32_t bits = 3;
    while ((1ull << bits) < 2ull * capacity) bits++;
    return bits;
}

}  // namespace

namespace rtxi {
void set_tally_hash_mask(uint64_t mask) { g_tally_hash_mask.store(mask); }
}  // namespace rtxi

struct rtx_tally : StageShell {
    rtx_tally_params params{};
    uint32_t columns = 1;
    // the object's state on the device, and what the host knows of it (exact: it reads the scan's totals at every add)
    DevBuf<uint32_t> d_table, d_e_len, d_count;
    DevBuf<uint64_t> d_e_hash, d_e_off, d_totals;
    DevBuf<uint8_t> d_arena;
    uint32_t tbits = 0;
    uint64_t cap_e = 0, cap_b = 0, n_entries = 0, n_bytes = 0, counted = 0;
    uint64_t table_mask = ~0ull;  // the mask the table was laid out under
    // a chunk
    DevBuf<uint8_t> d_packed, d_bases;
    DevBuf<uint64_t> d_base_off, d_hash, d_hash_full, d_new_off;
    DevBuf<uint32_t> d_ctable, d_owner, d_cluster_min, d_rep, d_ent, d_sw;
    DevBuf<Pair> d_block_sum;
    PinBuf<uint8_t> h_packed;
    PinBuf<uint64_t> h_base_off, h_totals;
    PinBuf<uint32_t> h_sw;
};

namespace {

int lay_out_table(rtx_tally *t, uint64_t mask) {
    RTX_HIP(hipMemsetAsync(t->d_table.p, 0, ((size_t)1 << t->tbits) * 4, t->stream));
    if (t->n_entries) {
        hipLaunchKernelGGL(tally_rehash_kernel, dim3((unsigned)((t->n_entries + 255u) / 256u)), dim3(256), 0, t->stream, t->d_table.p, t->tbits, t->d_e_hash.p, mask, (uint32_t)t->n_entries);
        RTX_HIP(hipGetLastError());
    }
    t->table_mask = mask;
    return RTX_OK;
}

// Room for need_e entries and need_b bytes (both within the caps): doubling, a new allocation, the part in use copied on the object's stream
template <class T>
int regrow(rtx_tally *t, DevBuf<T> &buf, size_t count, size_t used, bool zero_rest) {
    DevBuf<T> nb;
    if (const int rc = nb.alloc(count)) return rc;
    if (used) RTX_HIP(hipMemcpyAsync(nb.p, buf.p, used * sizeof(T), hipMemcpyDeviceToDevice, t->stream));
    if (zero_rest) RTX_HIP(hipMemsetAsync(nb.p + used, 0, (count - used) * sizeof(T), t->stream));
    RTX_HIP(hipStreamSynchronize(t->stream));  // (the old buffer is freed below)
    std::swap(buf.p, nb.p);
    std::swap(buf.n, nb.n);
    return RTX_OK;
}

int ensure_room(rtx_tally *t, uint64_t need_e, uint64_t need_b) {
    int rc;
    if (need_e > t->cap_e) {
        const uint64_t cap = std::min<uint64_t>(t->params.max_entries, std::max<uint64_t>(need_e, 2u * t->cap_e));
        const uint32_t bits = table_bits(cap);
        if ((rc = regrow(t, t->d_e_hash, cap, t->n_entries, false)) || (rc = regrow(t, t->d_e_len, cap, t->n_entries, false)) || (rc = regrow(t, t->d_e_off, cap, t->n_entries, false)) ||
            (rc = regrow(t, t->d_count, cap * t->columns, t->n_entries * t->columns, true)))
            return rc;
        t->cap_e = cap;
        if (bits != t->tbits) {
            t->d_table.release();
            if ((rc = t->d_table.alloc((size_t)1 << bits))) return rc;
            t->tbits = bits;
            if ((rc = lay_out_table(t, t->table_mask))) return rc;
        }
    }
    if (need_b > t->cap_b) {
        const uint64_t cap = std::min<uint64_t>(t->params.max_bytes, std::max<uint64_t>(need_b, 2u * t->cap_b));
        if ((rc = regrow(t, t->d_arena, cap + 64, t->n_bytes, false))) return rc;
        t->cap_b = cap;
    }
    return RTX_OK;
}

}  // namespace

namespace rtx {
int tally_device(const rtx_tally *t) { return t ? t->device : -1; }
uint32_t tally_samples(const rtx_tally *t) { return t ? t->params.n_samples : 0u; }
rtx_tally *index_tally(const rtx_index *index) { return index ? index->tally : nullptr; }
}  // namespace rtx

extern "C" {

int rtx_tally_create(int device, const rtx_tally_params *params, rtx_tally **out) {
    if (!out) { set_error("rtx_tally_create: null argument"); return RTX_ERR_INVALID; }
    *out = nullptr;
    rtx_tally_params p{};
    if (params) p = *params;
    if (!p.max_entries) p.max_entries = RTX_TALLY_DEFAULT_MAX_ENTRIES;
    if (!p.max_bytes) p.max_bytes = RTX_TALLY_DEFAULT_MAX_BYTES;
    if (!p.initial_entries) p.initial_entries = RTX_TALLY_DEFAULT_INITIAL_ENTRIES;
    if (!p.initial_bytes) p.initial_bytes = RTX_TALLY_DEFAULT_INITIAL_BYTES;
    const uint32_t columns = std::max(1u, p.n_samples);
    if (p.max_entries > 0x7FFFFFFEull) { set_error("rtx_tally_create: max_entries %llu (at most 2^31 - 2)", (unsigned long long)p.max_entries); return RTX_ERR_INVALID; }
    if (p.max_entries * columns > (1ull << 40)) {
        set_error("rtx_tally_create: %llu entries x %u columns: more than 2^40 cells", (unsigned long long)p.max_entries, columns);
        return RTX_ERR_INVALID;
    }
    if (const int rc = check_device(device)) return rc;
    auto t = new rtx_tally();
    t->params = p;
    t->columns = columns;
    int rc = t->open(device);
    if (!rc) rc = t->d_totals.alloc(8);
    if (!rc) rc = t->h_totals.resize(8);
    if (!rc && hipMemsetAsync(t->d_totals.p, 0, 64, t->stream) != hipSuccess) { set_error("rtx_tally_create: hipMemsetAsync failed"); rc = RTX_ERR_HIP; }
    // the first allocation: small, within the caps; the (empty) table for it
    if (!rc) rc = ensure_room(t, std::max<uint64_t>(1, std::min(p.initial_entries, p.max_entries)), std::max<uint64_t>(8, std::min(p.initial_bytes, p.max_bytes)));
    if (rc) { destroy(t); return rc; }
    *out = t;
    return RTX_OK;
}

void rtx_tally_destroy(rtx_tally *t) {
    if (t && t->stream) { (void)hipSetDevice(t->device); (void)hipStreamSynchronize(t->stream); }  // (an add returns with its last step enqueued)
    destroy(t);
}

int rtx_tally_info(const rtx_tally *t, uint64_t *entries, uint64_t *bytes, uint64_t *entry_capacity, uint64_t *byte_capacity, uint64_t *counted) {
    if (!t) { set_error("rtx_tally_info: null argument"); return RTX_ERR_INVALID; }
    if (entries) *entries = t->n_entries;
    if (bytes) *bytes = t->n_bytes;
    if (entry_capacity) *entry_capacity = t->cap_e;
    if (byte_capacity) *byte_capacity = t->cap_b;
    if (counted) *counted = t->counted;
    return RTX_OK;
}

int rtx_tally_add(rtx_tally *t, uint64_t n, const uint8_t *bases, const uint64_t *base_off, const uint32_t *sample, const uint32_t *weight) {
    if (!t) { set_error("rtx_tally_add: null argument"); return RTX_ERR_INVALID; }
    if (n == 0) return RTX_OK;
    if (n > 0x7FFFFFFEull) { set_error("rtx_tally_add: %llu reads in one chunk (at most 2^31 - 2)", (unsigned long long)n); return RTX_ERR_INVALID; }
    if (!base_off) { set_error("rtx_tally_add: null argument"); return RTX_ERR_INVALID; }
    uint64_t chunk_weight = 0;
    if (const int rc = rtx::tally_check_chunk("rtx_tally_add", n, bases, base_off, sample, weight, t->columns, t->counted, &chunk_weight)) return rc;
    if (chunk_weight == 0) return RTX_OK;  // (no read of the chunk counts: nothing to enqueue)
    const uint64_t total = base_off[n] - base_off[0];
    RTX_HIP(hipSetDevice(t->device));
    hipStream_t s = t->stream;
    int rc;
    const uint64_t mask = g_tally_hash_mask.load();
    if (mask != t->table_mask && (rc = lay_out_table(t, mask))) return rc;
    uint32_t bits = 1;
    while ((1ull << bits) < 2ull * n) bits++;
    const size_t slots = (size_t)1 << bits;
    const uint32_t n_blocks = (uint32_t)((n + 255u) / 256u);
    const bool sw = sample || weight;
    if ((rc = t->h_packed.resize(total + 64)) || (rc = t->h_base_off.resize(n + 1)) || (rc = t->h_sw.resize(sw ? 2 * n : 1)) || (rc = grow(t->d_packed, total + 64)) ||
        (rc = grow(t->d_bases, total + 64)) || (rc = grow(t->d_base_off, n + 1)) || (rc = grow(t->d_hash, n)) || (rc = grow(t->d_hash_full, n)) || (rc = grow(t->d_new_off, n)) ||
        (rc = grow(t->d_owner, n)) || (rc = grow(t->d_cluster_min, n)) || (rc = grow(t->d_rep, n)) || (rc = grow(t->d_ent, n)) || (rc = grow(t->d_sw, sw ? 2 * n : 1)) ||
        (rc = grow(t->d_block_sum, n_blocks)) || (rc = grow(t->d_ctable, slots)))
        return rc;
    if ((rc = upload_packed_reads(s, n, bases, base_off, t->h_packed, t->h_base_off, t->d_packed, t->d_base_off, t->d_bases))) return rc;
    if (sw) {  // sample | weight, one copy
        for (uint64_t q = 0; q < n; q++) { t->h_sw[q] = sample ? sample[q] : 0u; t->h_sw[n + q] = weight ? weight[q] : 1u; }
        RTX_HIP(hipMemcpyAsync(t->d_sw.p, t->h_sw.data(), 2 * n * 4, hipMemcpyHostToDevice, s));
    }
    RTX_HIP(hipMemsetAsync(t->d_ctable.p, 0, slots * 4, s));
    RTX_HIP(hipMemsetAsync(t->d_cluster_min.p, 0xFF, n * 4, s));
    RTX_HIP(hipMemsetAsync(t->d_totals.p, 0, 32, s));  // (overflow_reads behind them stays)
    TallyParams p{};
    p.d = DerepParams{t->d_bases.p, t->d_base_off.p, (uint32_t)n, t->d_hash.p, t->d_ctable.p, bits, mask, t->d_owner.p, t->d_cluster_min.p, t->d_rep.p};
    p.hash_full = t->d_hash_full.p;
    p.sample = sample ? t->d_sw.p : nullptr;
    p.weight = weight ? t->d_sw.p + n : nullptr;
    p.ent = t->d_ent.p;
    p.new_off = t->d_new_off.p;
    p.block_sum = t->d_block_sum.p;
    p.totals = t->d_totals.p;
    p.columns = t->columns;
    p.n_entries = t->n_entries;
    p.n_bytes = t->n_bytes;
    p.max_entries = t->params.max_entries;
    p.max_bytes = t->params.max_bytes;
    auto state = [&] {  // (the buffers of the object may have moved)
        p.table = t->d_table.p; p.tbits = t->tbits; p.e_hash = t->d_e_hash.p; p.e_len = t->d_e_len.p; p.e_off = t->d_e_off.p; p.arena = t->d_arena.p; p.count = t->d_count.p;
    };
    state();
    const dim3 waves((unsigned)((n + 3u) / 4u)), threads(n_blocks);
    hipLaunchKernelGGL(tally_lookup_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(tally_insert_new_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(tally_resolve_kernel, threads, dim3(256), 0, s, p);
    hipLaunchKernelGGL(tally_scan_blocks_kernel, dim3(1), dim3(256), 0, s, p, n_blocks);
    hipLaunchKernelGGL(tally_number_kernel, threads, dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    RTX_HIP(hipMemcpyAsync(t->h_totals.data(), t->d_totals.p, 32, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    const uint64_t new_e = t->h_totals[0], stored_e = t->h_totals[2], stored_b = t->h_totals[3];
    if (stored_e > new_e || t->n_entries + stored_e > t->params.max_entries || t->n_bytes + stored_b > t->params.max_bytes) {
        set_error("rtx_tally_add: the scan of the chunk stores %llu of %llu new reads in %llu bytes: outside the caps", (unsigned long long)stored_e, (unsigned long long)new_e,
                  (unsigned long long)stored_b);
        return RTX_ERR_HIP;  // (before anything is written through these numbers)
    }
    if ((rc = ensure_room(t, t->n_entries + stored_e, t->n_bytes + stored_b))) return rc;
    state();
    if (stored_e) hipLaunchKernelGGL(tally_append_kernel, waves, dim3(256), 0, s, p);
    hipLaunchKernelGGL(tally_count_kernel, threads, dim3(256), 0, s, p);
    RTX_HIP(hipGetLastError());
    t->n_entries += stored_e;
    t->n_bytes += stored_b;
    t->counted += chunk_weight;
    return RTX_OK;
}

int rtx_tally_read(rtx_tally *t, rtx_tally_table **table) {
    if (!t || !table) { set_error("rtx_tally_read: null argument"); return RTX_ERR_INVALID; }
    *table = nullptr;
    RTX_HIP(hipSetDevice(t->device));
    hipStream_t s = t->stream;
    const uint64_t ne = t->n_entries, nb = t->n_bytes, nc = t->columns;
    std::vector<uint32_t> len(ne), count(ne * nc);
    std::vector<uint64_t> off(ne);
    std::vector<uint8_t> arena(nb);
    uint64_t totals[8] = {0};
    if (ne) {
        RTX_HIP(hipMemcpyAsync(len.data(), t->d_e_len.p, ne * 4, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipMemcpyAsync(off.data(), t->d_e_off.p, ne * 8, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipMemcpyAsync(count.data(), t->d_count.p, ne * nc * 4, hipMemcpyDeviceToHost, s));
        RTX_HIP(hipMemcpyAsync(arena.data(), t->d_arena.p, nb, hipMemcpyDeviceToHost, s));
    }
    RTX_HIP(hipMemcpyAsync(totals, t->d_totals.p, 64, hipMemcpyDeviceToHost, s));
    RTX_HIP(hipStreamSynchronize(s));
    rtx_tally_table *out = nullptr;
    if (const int rc = rtx_tally_table_create(t->params.n_samples, &out)) return rc;
    for (uint64_t e = 0; e < ne; e++) {
        if (off[e] + len[e] > nb || rtx::tally_table_entry(*out, arena.data() + off[e], len[e]) != e) {
            rtx_tally_table_destroy(out);
            set_error("rtx_tally_read: entry %llu lies outside the arena or repeats an earlier one", (unsigned long long)e);
            return RTX_ERR_HIP;
        }
        for (uint64_t c = 0; c < nc; c++) out->counts[e * nc + c] = count[e * nc + c];
    }
    out->reads = t->counted;
    out->overflow_reads = totals[4];
    *table = out;
    return RTX_OK;
}

int rtx_index_set_tally(rtx_index *index, rtx_tally *tally) {
    if (!index) { set_error("rtx_index_set_tally: null index"); return RTX_ERR_INVALID; }
    if (tally && tally->device != index->device) {  // honoured by the host mirror alone (host_front.cpp): nothing else of the handle changes
        set_error("rtx_index_set_tally: the tally is on device %d, the handle on device %d", tally->device, index->device);
        return RTX_ERR_INVALID;
    }
    index->tally = tally;
    return RTX_OK;
}

rtx_tally *rtx_index_tally(const rtx_index *index) { return rtx::index_tally(index); }

}  // extern "C"

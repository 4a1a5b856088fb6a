// The read front of the host mirror (host_raxtax.cpp): what the lookup thread does to a chunk of reads before a handle classifies it.
//
//   stage (in this order)          on when                       reads    replaces   object per
//   tags      rtx_demux_run        rtx_index_set_tags            given    in ..      device
//   primers   rtx_trim_run         rtx_index_set_primers         in       src ..     device   (one cut for primers, quality and contaminants)
//   quality   rtx_qual_run         rtx_index_set_quality         in       src ..     device
//   contaminants rtx_screen_run    rtx_index_set_screen          in       src ..     device   (the same cut: no further copy)
//   copies    rtx_derep_run        RTX_OPT_DEREP                 src      dev        device
//   chimeras  rtx_chimera_run      rtx_index_set_chimera         dev      dev        handle   (it borrows the handle's bitmap)
//   distinct reads rtx_tally_add   rtx_index_set_tally           src      --         handle   (the caller's object: it outlives the call)
//
// A chunk holds four views of its reads (Reads).  Each starts as the one before it; the stage that cuts replaces it and every later one:
//   given  the caller's arrays
//   in     the tags cut, a read that is not assigned empty: trim and qual read it, and their callbacks measure raw_len on it
//   src    primers and low quality cut, a discarded read or a contaminant empty: derep reads it, and so do the `.tsv` sequence column and qlen of the align callback
//   dev    the distinct reads (dev.n of them), a flagged one empty: what the handle and the host lookup are given
// Every cut but the gather of the distinct reads goes through cut(): a chunk in which nothing is cut goes on as it came, without a copy.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "host_stage.hpp"
#include "rtx_internal.hpp"

namespace rtx_front {

// Runs fn(a, b) over contiguous ranges of [0, n) on up to `nt` threads.
template <class F>
void parallel_ranges(uint64_t n, unsigned nt, F fn) {
    rtx::parallel_ranges(n, nt, 256, [&fn](unsigned, uint64_t a, uint64_t b) { fn(a, b); });
}

// Bytes without a value yet (RTX_OPT_DEREP: the distinct reads of a chunk).  Not a std::vector: resize() would zero 86 MB per chunk on the
// one thread that dereplicates, which was most of the stage; the buffers travel between the chunks of a call through a pool, so that
// only the first few of them fault their pages in.
struct ByteBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n) {
        if (n <= cap) return true;
        free(p);
        cap = n + n / 8 + 64;
        p = static_cast<uint8_t *>(malloc(cap));
        if (!p) cap = 0;
        return p != nullptr;
    }
    ByteBuf() = default;
    ByteBuf(const ByteBuf &) = delete;
    ByteBuf(ByteBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ByteBuf &operator=(ByteBuf &&o) noexcept {
        if (this != &o) { free(p); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~ByteBuf() { free(p); }
};

// The buffers of cut reads between the sender (done with a chunk) and the lookup thread (a later chunk).
struct BufPool {
    std::mutex mu;
    std::vector<ByteBuf> free_bufs;
    void take(ByteBuf &b) {  // a used buffer if there is one
        std::lock_guard<std::mutex> g(mu);
        if (!free_bufs.empty()) { b = std::move(free_bufs.back()); free_bufs.pop_back(); }
    }
    void give(ByteBuf &b) {
        std::lock_guard<std::mutex> g(mu);
        if (b.p) free_bufs.push_back(std::move(b));
    }
};

// n reads: read i is bases[off[i] .. off[i + 1]), its qualities (where the view has them) quals[off[i] .. off[i + 1])
struct Reads {
    const uint8_t *bases = nullptr, *quals = nullptr;
    const uint64_t *off = nullptr;
    uint64_t n = 0;
    uint64_t len(uint64_t i) const { return off[i + 1] - off[i]; }
    uint32_t len32(uint64_t i) const { return (uint32_t)std::min<uint64_t>(len(i), 0xFFFFFFFFull); }
};

// The storage of a view that a stage cut: the kept ranges back to back, off[n + 1] from 0
struct Cut {
    ByteBuf bases, quals;
    std::vector<uint64_t> off;
};

// `to` = the ranges [lo[i], keep_hi[i]) of the reads of `from`, with their qualities if with_quals.  Where every range is its whole read nothing
// is copied and `to` is `from`.  Otherwise the ranges are laid out in `out` (buffers from the pool).  RTX_ERR_OOM sets `oom` as the error text.
int cut(const Reads &from, const uint32_t *lo, const uint32_t *keep_hi, bool with_quals, Cut &out, BufPool &pool, const char *oom, Reads &to);

// `to` = the reads uniq[0 .. nu) (ascending) of `from`, back to back in `out`: runs of neighbours move in one memcpy, on up to nt threads
int gather(const Reads &from, const uint32_t *uniq, uint64_t nu, Cut &out, BufPool &pool, unsigned nt, Reads &to);

// What the rtx_raxtax_last_* functions report of a call: the front's counters and busy seconds per stage (zeros for a stage that is off), and
// the busy seconds of the pipeline's stages (host lookup, device, format, sender) with its number of chunks.
struct FrontTotals {
    struct { uint64_t queries, assigned, reasons[5]; double busy; } demux;
    struct { uint64_t queries, with5, with3, emptied; double busy; } trim;
    struct { uint64_t queries, passed, truncated, reasons[7]; double busy; } qual;
    struct { uint64_t queries, screened, contaminants; double busy; } screen;
    struct { uint64_t queries, distinct; double busy; } derep;
    struct { uint64_t queries, checked, flagged; double busy; } chim;
    struct { uint64_t queries, counted, added; double busy; } tally;
    double busy[4];
    uint64_t n_chunks;
};

// The front's arrays of one chunk: the views, what the stages said per query of the caller (empty: that stage is off), and the storage of the cuts.
struct FrontChunk {
    Reads given, in, src, dev;
    std::vector<uint32_t> dx_sample, dx_lo, dx_hi, dx_hit, dx_info;  // rtx_demux_run
    std::vector<uint32_t> lo, hi, hit;                               // rtx_trim_run (the whole read without primers), filled with either of primers and quality on
    std::vector<uint32_t> q_hi, q_verdict, keep_hi;                  // rtx_qual_run on [lo, hi); keep_hi (quality or screen on): the end of what goes on -- q_hi, or lo for a discarded read
    std::vector<uint64_t> q_ee;
    std::vector<uint32_t> s_windows, s_hits, s_first, s_source, s_verdict;  // rtx_screen_run on [lo, keep_hi): a contaminant's keep_hi becomes lo
    std::vector<uint32_t> slot;  // RTX_OPT_DEREP: the position of query i's representative in `dev`; empty: i itself (no copies, or the option off)
    std::vector<uint32_t> size;  // [dev.n] copies of every distinct read: its weight in an open profile
    std::vector<rtx_chimera_rec> chim;  // [dev.n] rtx_chimera_run; query i's record is that of its representative
    Cut x, t, u, c;              // the storage of in, src, dev (distinct reads) and dev (flagged reads emptied)
    uint64_t at(uint64_t i) const { return slot.empty() ? i : slot[i]; }
    void release(BufPool &pool) {  // the buffers go back to the pool, everything else is freed
        for (Cut *k : {&x, &t, &u, &c}) { pool.give(k->bases); pool.give(k->quals); }
        *this = {};
    }
};

// The stage objects of a call: one per distinct device, shared by the handles of that device, or one per handle.
template <class T, void (*Destroy)(T *)>
struct StageSet {
    std::vector<T *> of;   // per handle
    std::vector<T *> own;
    StageSet() = default;
    StageSet(const StageSet &) = delete;
    ~StageSet() { for (T *p : own) Destroy(p); }
    template <class Create>  // create(d, &object) -> RTX_OK or an error
    int open(rtx_index *const *indices, uint32_t n_dev, bool per_device, Create create) {
        of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            for (uint32_t e = 0; per_device && e < d && !of[d]; e++)
                if (rtx::index_device(indices[e]) == rtx::index_device(indices[d])) of[d] = of[e];
            if (of[d]) continue;
            const int rc = create(d, &of[d]);
            if (rc) return rc;
            own.push_back(of[d]);
        }
        return RTX_OK;
    }
};

// RTX_ERR_INVALID with `msg` as the error text unless get(handle d) is get(handle 0) for every d
template <class Get, class Same = std::equal_to<>>
int agree(rtx_index *const *indices, uint32_t n_dev, Get get, const char *msg, Same same = Same()) {
    for (uint32_t d = 1; d < n_dev; d++)
        if (!same(get(indices[d]), get(indices[0]))) { rtx::set_error("%s", msg); return RTX_ERR_INVALID; }
    return RTX_OK;
}

// The front of a call: which stages are on (the same on every handle) and their objects.
struct Front {
    bool demux = false, trim = false, qual = false, screen = false, derep = false, chim = false, tally = false;
    uint32_t prof_samples = 0;  // the samples of the open profile (rtx_index_profile_begin_samples): the same on every handle
    StageSet<rtx_demux, rtx_demux_destroy> demuxes;
    StageSet<rtx_trim, rtx_trim_destroy> trims;
    StageSet<rtx_qual, rtx_qual_destroy> quals;
    StageSet<rtx_screen, rtx_screen_destroy> screens;
    StageSet<rtx_derep, rtx_derep_destroy> dereps;
    StageSet<rtx_chimera, rtx_chimera_destroy> chims;
    std::vector<rtx_tally *> tallies;  // per handle, the callers' (rtx_index_set_tally): not owned
    // checks that the handles agree on every stage and creates the objects; has_quals: the call brings quality strings, prof: a taxon profile is open
    int open(rtx_index *const *indices, uint32_t n_dev, bool has_quals, bool prof);
    bool any() const { return demux || trim || qual || screen || derep || chim || tally; }
    // chunk `fc` (given set, the other views as given) through the stages that are on, with the objects of handle d
    int run(uint32_t d, FrontChunk &fc, BufPool &pool, unsigned nt, FrontTotals &tot) const;
};

}  // namespace rtx_front

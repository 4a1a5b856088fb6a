// Host mirror of raxtax() (src/raxtax.rs:14-97): exact-match lookup, device classification in
// batches, single-exact-match override, formatting, one message per query to the sender.
#include "host_raxtax.hpp"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>

#include "rtx_internal.hpp"

namespace {

// Runs fn(i) for i in [0, n) on up to `nt` threads (contiguous ranges).
template <class F>
void parallel_ranges(uint64_t n, unsigned nt, F fn) {
    nt = (unsigned)std::min<uint64_t>(nt, (n + 255) / 256);
    if (nt <= 1) { fn(0, n); return; }
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; i++) th.emplace_back(fn, n * i / nt, n * (i + 1) / nt);
    for (auto &t : th) t.join();
}

// A few worker threads that live as long as a run of the pipeline: run(n, fn) hands fn(0) .. fn(n - 1) to them and returns when all are
// done (sixteen std::thread per chunk were half a millisecond of the format stage per chunk: created one after the other).
class WorkerPool {
public:
    explicit WorkerPool(unsigned n) {
        for (unsigned i = 0; i < n; i++) th_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run(unsigned n, const std::function<void(unsigned)> &fn) {
        if (n == 0) return;
        if (th_.empty() || n == 1) { for (unsigned r = 0; r < n; r++) fn(r); return; }
        std::unique_lock<std::mutex> g(mu_);
        job_ = &fn;
        n_jobs_ = n;
        next_ = done_ = 0;
        cv_.notify_all();
        cv_done_.wait(g, [&] { return done_ == n_jobs_; });
        job_ = nullptr;
        n_jobs_ = 0;
    }
private:
    void loop() {
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
            cv_.wait(g, [&] { return stop_ || (job_ && next_ < n_jobs_); });
            if (stop_) return;
            const unsigned r = next_++;
            const std::function<void(unsigned)> *job = job_;
            g.unlock();
            (*job)(r);
            g.lock();
            if (++done_ == n_jobs_) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, cv_done_;
    const std::function<void(unsigned)> *job_ = nullptr;
    unsigned n_jobs_ = 0, next_ = 0, done_ = 0;
    bool stop_ = false;
};

struct LastTiming { double busy[4]; uint64_t n_chunks; };
std::mutex g_timing_mu;
LastTiming g_timing{{0, 0, 0, 0}, 0};
struct LastDerep { uint64_t queries, distinct; double busy; };  // rtx_raxtax_last_derep (under g_timing_mu)
LastDerep g_derep{0, 0, 0.0};
struct LastTrim { uint64_t queries, with5, with3, emptied; double busy; };  // rtx_raxtax_last_trim (under g_timing_mu)
LastTrim g_trim{0, 0, 0, 0, 0.0};
struct LastQual { uint64_t queries, passed, truncated, reasons[7]; double busy; };  // rtx_raxtax_last_qual (under g_timing_mu)
LastQual g_qual{0, 0, 0, {0, 0, 0, 0, 0, 0, 0}, 0.0};
struct LastChim { uint64_t queries, checked, flagged; double busy; };  // rtx_raxtax_last_chimera (under g_timing_mu)
LastChim g_chim{0, 0, 0, 0.0};
struct LastDemux { uint64_t queries, assigned, reasons[5]; double busy; };  // rtx_raxtax_last_demux (under g_timing_mu)
LastDemux g_demux{0, 0, {0, 0, 0, 0, 0}, 0.0};

// (label, out_lines, tsv_lines or null) as C strings: what the C ABI's callback takes; false = the sink is closed
using RawSender = std::function<bool(const char *, const char *, const char *)>;
// (label, strand, peak, t) of the query whose message follows (rtx_query_info_fn); empty: nobody asked
// ... with the nearest reference and its ties behind them (rtx_query_hit_fn; RTX_NO_REF and 0 with RTX_OPT_NEAREST off)
// ... and the alignment identity: distance and query length (rtx_query_align_fn; RTX_NO_DIST and the length with RTX_OPT_IDENTITY off)
using RawInfo = std::function<bool(const char *, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t)>;
// (label, length as given, lo, hi, hit) of every query, directly before its RawInfo call (rtx_query_trim_fn); empty: nobody asked
using RawTrim = std::function<bool(const char *, uint32_t, uint32_t, uint32_t, uint32_t)>;
// (label, length as given, lo, hi, expected errors, verdict) of every query, directly after its RawTrim call (rtx_query_qual_fn)
using RawQual = std::function<bool(const char *, uint32_t, uint32_t, uint32_t, uint64_t, uint32_t)>;
// (label, record) of every query, directly after its RawQual call (rtx_query_chimera_fn)
using RawChim = std::function<bool(const char *, const rtx_chimera_rec *)>;
// (label, length as given, sample, lo, hi, hit, info) of every query, directly before its RawTrim call (rtx_query_demux_fn)
using RawDemux = std::function<bool(const char *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t)>;

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

// One chunk of queries travelling through the stages of run().
struct Chunk {
    uint64_t q0 = 0, nq = 0;
    std::vector<uint32_t> exact_ids;   // tree.sequences.get(query) per query, raxtax.rs:42
    std::vector<uint64_t> exact_off;
    std::vector<uint8_t> differ;       // raxtax.rs:43-53: exact matches with different parents
    std::vector<uint8_t> status;       // res.status / res.t copied by the format stage: the sender must not read `res`, whose host set the
    std::vector<uint32_t> t;           // handle reuses once this chunk is formatted
    std::vector<uint8_t> strand;       // rtx_batch_strands, copied by the device stage (both strands, or an info callback)
    std::vector<uint32_t> peak;
    std::vector<uint32_t> nearest, ties;  // rtx_batch_nearest, copied with them (RTX_OPT_NEAREST and an info callback)
    std::vector<uint32_t> dist;           // rtx_batch_identity, the same (RTX_OPT_IDENTITY)
    // The messages of the chunk: every formatting thread appends the NUL-terminated `.out` (and `.tsv`) text of its queries to an arena
    // of its own; msg_off[i] locates query i's text in the arena of the thread that took it (a std::string per message was a malloc in
    // the format thread and a free in the sender's, per query: half of the format stage)
    struct Arena {
        char *p = nullptr;
        size_t cap = 0, len = 0;
        char *room(size_t need) {  // a pointer behind the text so far with `need` bytes of room
            if (len + need > cap) {
                size_t c = cap ? cap + cap / 2 : (size_t)1 << 20;
                while (c < len + need) c += c / 2;
                char *np = static_cast<char *>(realloc(p, c));
                if (!np) return nullptr;
                p = np;
                cap = c;
            }
            return p + len;
        }
        void release() { free(p); p = nullptr; cap = len = 0; }
        ~Arena() { free(p); }
        Arena() = default;
        Arena(const Arena &) = delete;
        Arena(Arena &&o) noexcept : p(o.p), cap(o.cap), len(o.len) { o.p = nullptr; o.cap = o.len = 0; }
        Arena &operator=(Arena &&o) noexcept {
            if (this != &o) { free(p); p = o.p; cap = o.cap; len = o.len; o.p = nullptr; o.cap = o.len = 0; }
            return *this;
        }
    };
    std::vector<Arena> out_arena, tsv_arena;   // one per formatting thread
    std::vector<uint64_t> msg_off, tsv_off;    // [nq] offset of the query's text in its thread's arena
    std::vector<uint32_t> msg_arena;           // [nq] which arena
    // RTX_OPT_DEREP: the handle is given the distinct reads of the chunk alone, and whatever comes back per query is read through slot[]
    uint64_t nu = 0;                   // queries handed to the handle: nq, or the distinct reads of a chunk that has copies
    const uint8_t *dev_bases = nullptr;  // what every device call of the chunk (and the host lookup) is given: the caller's arrays,
    const uint64_t *dev_off = nullptr;   // or u_bases / u_off ([nu + 1], from 0: rtx_batch_prefetch wants contiguous offsets)
    std::vector<uint32_t> slot;        // [nq] position of query i's representative among the distinct reads; empty: i itself (no copies, or the option off)
    std::vector<uint32_t> size;        // [nu] copies of every distinct read: its weight in an open profile
    ByteBuf u_bases;
    std::vector<uint64_t> u_off;
    // sample demultiplexing (rtx_index_set_tags): rtx_demux_run per query of the caller (empty: off), and the reads of the chunk as the stages
    // behind it are given them -- the caller's arrays (in_off = base_off + q0), or, where a tag was cut or a read was not assigned, the kept
    // ranges back to back (x_bases / x_quals / x_off, [nq + 1] from 0).  Query i: in_bases + in_off[i], its qualities in_quals + in_off[i].
    const uint8_t *in_bases = nullptr, *in_quals = nullptr;
    const uint64_t *in_off = nullptr;
    std::vector<uint32_t> dx_sample, dx_lo, dx_hi, dx_hit, dx_info;
    ByteBuf x_bases, x_quals;
    std::vector<uint64_t> x_off;
    // primer trimming (rtx_index_set_primers): the reads of the chunk as everything downstream sees them -- the caller's arrays, or, where a
    // primer was found in the chunk, the kept ranges back to back (t_bases / t_off, [nq + 1] from 0).  Query i: src_bases + src_off[i].
    const uint8_t *src_bases = nullptr;
    const uint64_t *src_off = nullptr;
    std::vector<uint32_t> lo, hi, hit;  // [nq] rtx_trim_run, per query of the caller (empty: primers and quality filter are off)
    // quality filter (rtx_index_set_quality): rtx_qual_run on [lo, hi), per query of the caller (empty: off); keep_hi: the end of what goes
    // downstream -- q_hi, or lo for a discarded read (the empty read)
    std::vector<uint32_t> q_hi, q_verdict, keep_hi;
    std::vector<uint64_t> q_ee;
    ByteBuf t_bases;
    std::vector<uint64_t> t_off;
    // chimera check (rtx_index_set_chimera): rtx_chimera_run on the reads handed to the handle, [nu] (empty: off) -- query i's record is that of
    // its representative; where a read was flagged the handle is given c_bases / c_off ([nu + 1] from 0) with the flagged reads emptied
    std::vector<rtx_chimera_rec> chim;
    ByteBuf c_bases;
    std::vector<uint64_t> c_off;
    rtx_text_view text{};              // RTX_OPT_DEVICE_TEXT: the messages as the device formatted them (valid as long as `res`)
    rtx_result_view res{};
    int stage = 0;                     // 1: exact matches looked up (or left to the device), 2: classified, 3: formatted, 4: sent
};

// raxtax() (src/raxtax.rs:14-97) as a pipeline over chunks of `chunk_size` queries on one or several device handles -- the
// reference's `par_chunks(chunk_size)` (raxtax.rs:35-36) with GPUs in the place of rayon workers.  Chunk c belongs to handle
// c mod n_dev; per handle
//   device thread : classification of its chunks, one after the other  (rtx_classify_batch, raxtax.rs:42,55-71)
//   format thread : lineage check of the exact matches (raxtax.rs:43-53), override + formatting (raxtax.rs:73-84), chunk by chunk
// and for all of them
//   lookup thread : exact-match ids (host hash map, raxtax.rs:42) -- only for handles without the device lookup
//                   (rtx_index_has_exact_lookup): otherwise the ids come back with the results of the device stage
//                   Under RTX_OPT_DEREP it first finds the copies of the chunk on the device (rtx_derep_run, a stream of its own beside
//                   the handle's) and cuts the chunk down to its distinct reads: the handle classifies those, the format thread and
//                   the sender go on per query of the caller (Chunk::slot)
//                   With tags set (rtx_index_set_tags) it first assigns the reads of the chunk to their samples (rtx_demux_run, the same
//                   kind of stage) and cuts the tags off: every stage below is given the cut reads (Chunk::in_bases), a read that is
//                   not assigned goes on as the empty read
//                   With primers set (rtx_index_set_primers) it trims the reads of the chunk before that (rtx_trim_run, the same kind of
//                   stage): the copies are looked for among the trimmed reads, and everything downstream sees those (Chunk::src_bases)
//                   With a quality filter set (rtx_index_set_quality) the ranges the primers left are filtered next (rtx_qual_run, again
//                   such a stage); both ranges are applied in one rtx_trim_apply, a discarded read goes on as the empty read
//                   With the chimera check set (rtx_index_set_chimera) the reads that go to the handle -- behind the dereplication, so a
//                   distinct read is checked once -- run through rtx_chimera_run (a stage object per handle: it borrows that handle's
//                   bitmap); a flagged read goes on as the empty read through one more rtx_trim_apply, exactly as a discarded one
//   calling thread: the sender, one message per query in INPUT order (raxtax.rs:85-87): chunk 0, 1, 2 ... as they become ready.
// A handle keeps two result sets, so the view of its k-th chunk stays valid until its (k + 2)-th is classified.
int run(rtx_index *const *indices, uint32_t n_dev, const rtx_tree *tree, uint64_t n_queries, const char *const *labels,
        const uint8_t *bases, const uint64_t *base_off, bool skip_exact_matches, bool raw_confidence, uint64_t chunk_size,
        const RawSender &sender, bool tsv, const RawInfo &info = RawInfo(), const RawTrim &trim_cb = RawTrim(), const uint8_t *quals = nullptr,
        const RawQual &qual_cb = RawQual(), const RawChim &chim_cb = RawChim(), const RawDemux &demux_cb = RawDemux()) {
    if (!indices || n_dev == 0 || !tree || !base_off || !labels) { rtx::set_error("rtx_raxtax: null argument"); return RTX_ERR_INVALID; }
    for (uint32_t d = 0; d < n_dev; d++) {
        if (!indices[d]) { rtx::set_error("rtx_raxtax: null index handle"); return RTX_ERR_INVALID; }
        if (rtx_index_num_refs(indices[d]) != tree->num_tips) { rtx::set_error("index and tree disagree on num_tips"); return RTX_ERR_INVALID; }
        for (uint32_t e = 0; e < d; e++)
            if (indices[e] == indices[d]) { rtx::set_error("rtx_raxtax_multi: the same handle twice (calls on one handle must be serialised)"); return RTX_ERR_INVALID; }
    }
    if (chunk_size == 0 || chunk_size > n_queries) chunk_size = std::max<uint64_t>(1, (n_queries + n_dev - 1) / n_dev);
    const uint32_t flags = (skip_exact_matches ? RTX_SKIP_EXACT_MATCHES : 0u) | (raw_confidence ? RTX_RAW_CONFIDENCE : 0u);
    const uint64_t n_chunks = (n_queries + chunk_size - 1) / chunk_size;
    // thread budget: this process's share of the host's CPUs (rtx::host_threads), split over the handles driven here
    const unsigned nt_lookup = rtx::host_threads(4u), nt_format = rtx::host_threads(16u, n_dev);
    std::vector<uint8_t> dev_lookup(n_dev), dev_text(n_dev);
    bool any_host_lookup = false;
    // RTX_OPT_STRAND: every handle classifies both orientations, or none does; the exact matches then come from the device (those of a
    // reverse complement belong to the same lookup) and the text from the host (the device formats the given orientation only)
    const bool both = rtx::index_strand(indices[0]);
    for (uint32_t d = 0; d < n_dev; d++) {
        if (rtx::index_strand(indices[d]) != both) { rtx::set_error("rtx_raxtax_multi: the handles disagree on RTX_OPT_STRAND"); return RTX_ERR_INVALID; }
        if (both && !rtx_index_has_exact_lookup(indices[d])) { rtx::set_error("RTX_OPT_STRAND needs the exact-match lookup of the device (a handle built from the reference sequences)"); return RTX_ERR_STATE; }
    }
    const bool want_strands = both || (bool)info;
    const bool near = rtx::index_nearest(indices[0]);  // RTX_OPT_NEAREST: on every handle, or on none
    for (uint32_t d = 0; d < n_dev; d++)
        if (rtx::index_nearest(indices[d]) != near) { rtx::set_error("rtx_raxtax_multi: the handles disagree on RTX_OPT_NEAREST"); return RTX_ERR_INVALID; }
    const bool ident = rtx::index_identity(indices[0]);  // RTX_OPT_IDENTITY: the same
    for (uint32_t d = 0; d < n_dev; d++)
        if (rtx::index_identity(indices[d]) != ident) { rtx::set_error("rtx_raxtax_multi: the handles disagree on RTX_OPT_IDENTITY"); return RTX_ERR_INVALID; }
    // an open taxon profile (rtx_index_profile_begin): on every handle or on none, with one cutoff, and with the flags of this call
    uint32_t prof_cutoff = 0, prof_flags = 0;
    const bool prof = rtx::index_profile(indices[0], &prof_cutoff, &prof_flags);
    for (uint32_t d = 1; d < n_dev; d++) {
        uint32_t c = 0, f = 0;
        if (rtx::index_profile(indices[d], &c, &f) != prof || (prof && (c != prof_cutoff || f != prof_flags))) {
            rtx::set_error("rtx_raxtax_multi: the handles disagree on their taxon profile (open on all or on none, one cutoff, one set of flags)");
            return RTX_ERR_INVALID;
        }
    }
    if (prof && prof_flags != flags) {
        rtx::set_error("rtx_raxtax: the open taxon profile has flags %#x, the call %#x (skip_exact_matches / raw_confidence must match)", prof_flags, flags);
        return RTX_ERR_INVALID;
    }
    // RTX_OPT_DEREP: on every handle, or on none.  One stage object (rtx_derep.hip) per distinct device for the duration of the call: the
    // lookup thread runs chunk c through the object of handle c mod n_dev's device while that handle still classifies an earlier chunk.
    const bool derep = rtx::index_derep(indices[0]);
    for (uint32_t d = 0; d < n_dev; d++)
        if (rtx::index_derep(indices[d]) != derep) { rtx::set_error("rtx_raxtax_multi: the handles disagree on RTX_OPT_DEREP"); return RTX_ERR_INVALID; }
    struct Dereps {
        std::vector<rtx_derep *> of;  // per handle; handles of one device share an object
        std::vector<rtx_derep *> own;
        ~Dereps() { for (auto *p : own) rtx_derep_destroy(p); }
    } dereps;
    if (derep) {
        dereps.of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            for (uint32_t e = 0; e < d && !dereps.of[d]; e++)
                if (rtx::index_device(indices[e]) == rtx::index_device(indices[d])) dereps.of[d] = dereps.of[e];
            if (dereps.of[d]) continue;
            const int rc = rtx_derep_create(rtx::index_device(indices[d]), &dereps.of[d]);
            if (rc) return rc;
            dereps.own.push_back(dereps.of[d]);
        }
    }
    // Tags (rtx_index_set_tags): the same list on every handle.  One stage object (rtx_demux.hip) per distinct device, as for derep.
    const rtx::DemuxList &taglist = rtx::index_tags(indices[0]);
    const bool demux = !taglist.empty();
    for (uint32_t d = 1; d < n_dev; d++)
        if (!(rtx::index_tags(indices[d]) == taglist)) { rtx::set_error("rtx_raxtax_multi: the handles disagree on their tags (rtx_index_set_tags)"); return RTX_ERR_INVALID; }
    const uint32_t prof_samples = rtx::index_profile_samples(indices[0]);
    for (uint32_t d = 1; d < n_dev; d++)
        if (rtx::index_profile_samples(indices[d]) != prof_samples) { rtx::set_error("rtx_raxtax_multi: the handles disagree on the samples of their taxon profile (rtx_index_profile_begin_samples)"); return RTX_ERR_INVALID; }
    if (demux && derep && prof) {
        rtx::set_error("rtx_raxtax: tags (rtx_index_set_tags) together with RTX_OPT_DEREP and an open taxon profile: copies from different samples would be counted as one read");
        return RTX_ERR_INVALID;
    }
    struct Demuxes {
        std::vector<rtx_demux *> of;  // per handle; handles of one device share an object
        std::vector<rtx_demux *> own;
        ~Demuxes() { for (auto *p : own) rtx_demux_destroy(p); }
    } demuxes;
    if (demux) {
        std::vector<rtx_demux_tag> tags(taglist.codes.size());
        for (size_t i = 0; i < tags.size(); i++) tags[i] = {taglist.codes[i].data(), (uint32_t)taglist.codes[i].size(), taglist.end[i]};
        demuxes.of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            for (uint32_t e = 0; e < d && !demuxes.of[d]; e++)
                if (rtx::index_device(indices[e]) == rtx::index_device(indices[d])) demuxes.of[d] = demuxes.of[e];
            if (demuxes.of[d]) continue;
            const int rc = rtx_demux_create(rtx::index_device(indices[d]), tags.data(), (uint32_t)tags.size(), taglist.pairs.data(), (uint32_t)taglist.pairs.size(),
                                            &taglist.params, &demuxes.of[d]);
            if (rc) return rc;
            demuxes.own.push_back(demuxes.of[d]);
        }
    }
    // Primers (rtx_index_set_primers): the same list on every handle.  One stage object (rtx_trim.hip) per distinct device, as for derep.
    const std::vector<rtx::TrimPrimer> &primers = rtx::index_primers(indices[0]);
    const bool trim = !primers.empty();
    for (uint32_t d = 1; d < n_dev; d++)
        if (!(rtx::index_primers(indices[d]) == primers)) { rtx::set_error("rtx_raxtax_multi: the handles disagree on their primers (rtx_index_set_primers)"); return RTX_ERR_INVALID; }
    struct Trims {
        std::vector<rtx_trim *> of;  // per handle; handles of one device share an object
        std::vector<rtx_trim *> own;
        ~Trims() { for (auto *p : own) rtx_trim_destroy(p); }
    } trims;
    if (trim) {
        std::vector<rtx_trim_pattern> pats(primers.size());
        for (size_t i = 0; i < primers.size(); i++) pats[i] = {primers[i].codes.data(), (uint32_t)primers[i].codes.size(), primers[i].end, primers[i].max_errors, primers[i].window};
        trims.of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            for (uint32_t e = 0; e < d && !trims.of[d]; e++)
                if (rtx::index_device(indices[e]) == rtx::index_device(indices[d])) trims.of[d] = trims.of[e];
            if (trims.of[d]) continue;
            const int rc = rtx_trim_create(rtx::index_device(indices[d]), pats.data(), (uint32_t)pats.size(), &trims.of[d]);
            if (rc) return rc;
            trims.own.push_back(trims.of[d]);
        }
    }
    // Quality filter (rtx_index_set_quality): the same setting on every handle, and the call brings the quality strings.  One stage object
    // (rtx_qual.hip) per distinct device, as for the primers.
    rtx_qual_params qparams{};
    const bool qual = rtx::index_quality(indices[0], &qparams);
    for (uint32_t d = 1; d < n_dev; d++) {
        rtx_qual_params other{};
        if (rtx::index_quality(indices[d], &other) != qual || (qual && !rtx::qual_params_equal(other, qparams))) {
            rtx::set_error("rtx_raxtax_multi: the handles disagree on their quality filter (rtx_index_set_quality)");
            return RTX_ERR_INVALID;
        }
    }
    if (qual && !quals) { rtx::set_error("rtx_raxtax: a quality filter is set (rtx_index_set_quality) and the call brings no quality strings (rtx_raxtax_multi_ex5)"); return RTX_ERR_INVALID; }
    struct Quals {
        std::vector<rtx_qual *> of;  // per handle; handles of one device share an object
        std::vector<rtx_qual *> own;
        ~Quals() { for (auto *p : own) rtx_qual_destroy(p); }
    } qualstages;
    if (qual) {
        qualstages.of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            for (uint32_t e = 0; e < d && !qualstages.of[d]; e++)
                if (rtx::index_device(indices[e]) == rtx::index_device(indices[d])) qualstages.of[d] = qualstages.of[e];
            if (qualstages.of[d]) continue;
            const int rc = rtx_qual_create(rtx::index_device(indices[d]), &qparams, &qualstages.of[d]);
            if (rc) return rc;
            qualstages.own.push_back(qualstages.of[d]);
        }
    }
    // Chimera check (rtx_index_set_chimera): the same setting on every handle.  One stage object (rtx_chimera.hip) per HANDLE: it reads that
    // handle's bitmap.  Not with RTX_OPT_STRAND (rtx_chimera_create refuses it: a read is checked in the orientation given).
    rtx_chimera_params cparams{};
    const bool chim = rtx::index_chimera(indices[0], &cparams);
    for (uint32_t d = 1; d < n_dev; d++) {
        rtx_chimera_params other{};
        if (rtx::index_chimera(indices[d], &other) != chim || (chim && (other.segments != cparams.segments || other.mindelta != cparams.mindelta))) {
            rtx::set_error("rtx_raxtax_multi: the handles disagree on their chimera check (rtx_index_set_chimera)");
            return RTX_ERR_INVALID;
        }
    }
    struct Chims {
        std::vector<rtx_chimera *> of;  // per handle
        ~Chims() { for (auto *p : of) rtx_chimera_destroy(p); }
    } chims;
    if (chim) {
        chims.of.assign(n_dev, nullptr);
        for (uint32_t d = 0; d < n_dev; d++) {
            const int rc = rtx_chimera_create(indices[d], &cparams, &chims.of[d]);
            if (rc) return rc;
        }
    }
    for (uint32_t d = 0; d < n_dev; d++) {
        dev_lookup[d] = rtx_index_has_exact_lookup(indices[d]) != 0;
        any_host_lookup = any_host_lookup || !dev_lookup[d];
        // RTX_OPT_DEVICE_TEXT: the messages come from the device (rtx_text.hip), set up for this tree and these flags
        // (not under RTX_OPT_DEREP: a device line carries one label, a distinct read has as many as it has copies)
        dev_text[d] = rtx::index_device_text(indices[d]) && !both && !derep;
        if (dev_text[d]) {
            const int rc = rtx_index_text_setup(indices[d], tree, flags | (tsv ? RTX_TEXT_TSV : 0u));
            if (rc) return rc;
        }
    }

    // chunks follow one another through rtx_batch_download_then_run (the last sub-batch of a chunk is finalised beside the next chunk): two
    // large sub-batches per chunk instead of four small ones (RTX_OPT_MIN_SUB_BATCHES); the handles get their setting back below
    struct MinSubs {  // (the caller's own RTX_OPT_MIN_SUB_BATCHES comes back, and the handle's last batch stays what it was: ADVICE r5)
        rtx_index *const *ix; uint32_t n;
        std::vector<uint32_t> was;
        MinSubs(rtx_index *const *i, uint32_t k, uint64_t n_chunks) : ix(i), n(n_chunks > 1 ? k : 0), was(n) { for (uint32_t d = 0; d < n; d++) was[d] = rtx::index_swap_min_subs(ix[d], 2); }
        ~MinSubs() { for (uint32_t d = 0; d < n; d++) (void)rtx::index_swap_min_subs(ix[d], was[d]); }
    } min_subs_guard(indices, n_dev, n_chunks);
    // ... and chunk c + 1 is enqueued before the last sub-batch of chunk c has finished (RTX_OPT_RUN_AHEAD: the two streams of a handle do not
    // drain between chunks); not for handles that share a device (one stream each, below), and only with hardware queues to spare (host_threads.cpp)
    struct RunAhead {
        rtx_index *const *ix; uint32_t n;
        std::vector<uint32_t> was;
        RunAhead(rtx_index *const *i, uint32_t k, uint64_t n_chunks) : ix(i), n(n_chunks > 1 && rtx::hw_queues_for_run_ahead() ? k : 0), was(n) { for (uint32_t d = 0; d < n; d++) { was[d] = rtx::index_swap_run_ahead(ix[d], 1); if (was[d] > 1u) (void)rtx::index_swap_run_ahead(ix[d], was[d]); } }  // (2: the test aid stays)
        ~RunAhead() { for (uint32_t d = 0; d < n; d++) (void)rtx::index_swap_run_ahead(ix[d], was[d]); }
    } run_ahead_guard(indices, n_dev, n_chunks);
    // handles that share a device (rehearsals of the multi-GPU path on one GPU) run on one stream each for the duration of the call
    struct SharedDevice {
        rtx_index *const *ix; uint32_t n;
        SharedDevice(rtx_index *const *i, uint32_t k) : ix(i), n(k) {
            for (uint32_t d = 0; d < n; d++)
                for (uint32_t e = 0; e < n; e++)
                    if (e != d && rtx::index_device(ix[e]) == rtx::index_device(ix[d])) rtx::index_set_shared_device(ix[d], true);
        }
        ~SharedDevice() { for (uint32_t d = 0; d < n; d++) rtx::index_set_shared_device(ix[d], false); }
    } shared_guard(indices, n_dev);
    std::vector<Chunk> chunks(n_chunks);
    for (uint64_t c = 0; c < n_chunks; c++) {
        chunks[c].q0 = c * chunk_size;
        chunks[c].nq = chunks[c].nu = std::min<uint64_t>(chunk_size, n_queries - chunks[c].q0);
        chunks[c].dev_bases = chunks[c].src_bases = bases;
        chunks[c].dev_off = chunks[c].src_off = base_off + chunks[c].q0;
        chunks[c].in_bases = bases;
        chunks[c].in_off = base_off + chunks[c].q0;
        chunks[c].in_quals = quals;
    }
    // busy seconds of the stages (rtx_raxtax_last_timing: which stage bounds an end-to-end run)
    double busy_lookup = 0, busy_send = 0, busy_derep = 0, busy_trim = 0, busy_qual = 0, busy_chim = 0;
    uint64_t chim_queries = 0, chim_checked = 0, chim_flagged = 0;
    uint64_t qual_queries = 0, qual_passed = 0, qual_truncated = 0, qual_reasons[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t derep_queries = 0, derep_distinct = 0;
    uint64_t trim_queries = 0, trim_with5 = 0, trim_with3 = 0, trim_emptied = 0;
    double busy_demux = 0;
    uint64_t demux_queries = 0, demux_assigned = 0, demux_reasons[5] = {0, 0, 0, 0, 0};
    std::vector<double> busy_device(n_dev, 0.0), busy_format(n_dev, 0.0);
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    std::mutex mu;
    std::condition_variable cv;
    int failed = RTX_OK;          // first error of any stage (under mu)
    std::string failed_msg;
    bool warnings = false;
    auto fail = [&](int rc, const std::string &msg) {
        std::lock_guard<std::mutex> g(mu);
        if (failed == RTX_OK) { failed = rc; failed_msg = msg; }
        cv.notify_all();
    };
    // blocks until chunk c has reached `stage`; false if the run has failed meanwhile
    auto wait_stage = [&](uint64_t c, int stage) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return failed != RTX_OK || chunks[c].stage >= stage; });
        return failed == RTX_OK;
    };
    auto set_stage = [&](uint64_t c, int stage) {
        std::lock_guard<std::mutex> g(mu);
        chunks[c].stage = stage;
        cv.notify_all();
    };
    const uint64_t ahead = 2ull * n_dev;  // chunks a stage may run ahead of the next one
    std::mutex pool_mu;
    std::vector<Chunk::Arena> arena_pool;  // message arenas between the sender (done with a chunk) and the format threads (next chunk)
    std::vector<ByteBuf> bases_pool;       // ... and the arrays of distinct reads (RTX_OPT_DEREP) and of trimmed reads (primers) between the sender and the lookup thread

    std::thread lookup([&] {
        for (uint64_t c = 0; c < n_chunks; c++) {
            Chunk &ch = chunks[c];
            if (!demux && !derep && !trim && !qual && !chim && dev_lookup[c % n_dev]) { set_stage(c, 1); continue; }  // Tree.sequences.get runs on the device, inside rtx_classify_batch
            if (c >= ahead && !wait_stage(c - ahead, 2)) return;
            if (demux) {  // the sample of every read of the chunk, on the device (a stream of its own beside the handle's); then the reads without their tags
                const double t_x0 = now();
                for (auto *v : {&ch.dx_sample, &ch.dx_lo, &ch.dx_hi, &ch.dx_hit, &ch.dx_info}) v->resize(ch.nq);
                int rc = rtx_demux_run(demuxes.of[c % n_dev], ch.nq, bases, base_off + ch.q0, ch.dx_sample.data(), ch.dx_lo.data(), ch.dx_hi.data(), ch.dx_hit.data(),
                                       ch.dx_info.data());
                std::vector<uint32_t> keep_hi(ch.nq);  // a read that is not assigned goes on empty
                bool any = false;
                uint64_t kept = 0;
                if (!rc)
                    for (uint64_t i = 0; i < ch.nq; i++) {
                        const uint32_t v = ch.dx_info[i] & 0xFFu;
                        keep_hi[i] = v == RTX_DEMUX_OK ? ch.dx_hi[i] : ch.dx_lo[i];
                        kept += keep_hi[i] - ch.dx_lo[i];
                        any = any || ch.dx_lo[i] != 0u || keep_hi[i] != base_off[ch.q0 + i + 1] - base_off[ch.q0 + i];
                        demux_assigned += v == RTX_DEMUX_OK;
                        if (v < 5u) demux_reasons[v]++;
                    }
                if (!rc && any) {  // (a chunk in which nothing was cut goes on as it came, without a copy)
                    {
                        std::lock_guard<std::mutex> g(pool_mu);
                        if (!bases_pool.empty()) { ch.x_bases = std::move(bases_pool.back()); bases_pool.pop_back(); }
                        if (quals && !bases_pool.empty()) { ch.x_quals = std::move(bases_pool.back()); bases_pool.pop_back(); }
                    }
                    if (!ch.x_bases.reserve(kept + 1) || (quals && !ch.x_quals.reserve(kept + 1))) { fail(RTX_ERR_OOM, "no memory for the demultiplexed reads of a chunk"); return; }
                    ch.x_off.resize(ch.nq + 1);
                    rc = rtx_trim_apply(ch.nq, bases, base_off + ch.q0, ch.dx_lo.data(), keep_hi.data(), ch.x_bases.p, ch.x_off.data());
                    if (!rc && quals) rc = rtx_trim_apply(ch.nq, quals, base_off + ch.q0, ch.dx_lo.data(), keep_hi.data(), ch.x_quals.p, ch.x_off.data());
                    if (!rc) {
                        ch.dev_bases = ch.src_bases = ch.in_bases = ch.x_bases.p;
                        ch.dev_off = ch.src_off = ch.in_off = ch.x_off.data();
                        if (quals) ch.in_quals = ch.x_quals.p;
                    }
                }
                if (rc) { fail(rc, rtx_last_error()); return; }
                demux_queries += ch.nq;
                busy_demux += now() - t_x0;
                if (!derep && !trim && !qual && !chim && dev_lookup[c % n_dev]) { set_stage(c, 1); continue; }
            }
            if (trim || qual) {  // the primers of the chunk's reads, then their quality, on the device (streams of their own beside the handle's); then the kept ranges
                const double t_t0 = now();
                ch.lo.resize(ch.nq);
                ch.hi.resize(ch.nq);
                ch.hit.resize(ch.nq);
                int rc = RTX_OK;
                if (trim) {
                    rc = rtx_trim_run(trims.of[c % n_dev], ch.nq, ch.in_bases, ch.in_off, ch.lo.data(), ch.hi.data(), ch.hit.data());
                    if (!rc)
                        for (uint64_t i = 0; i < ch.nq; i++) {
                            const uint64_t len = ch.in_off[i + 1] - ch.in_off[i];
                            const bool f5 = (ch.hit[i] & 0xFFu) != RTX_TRIM_NO_PATTERN, f3 = ((ch.hit[i] >> 16) & 0xFFu) != RTX_TRIM_NO_PATTERN;
                            trim_with5 += f5;
                            trim_with3 += f3;
                            trim_emptied += len != 0 && ch.hi[i] == ch.lo[i];
                        }
                } else {
                    for (uint64_t i = 0; i < ch.nq; i++) {
                        ch.lo[i] = 0u;
                        ch.hi[i] = (uint32_t)std::min<uint64_t>(ch.in_off[i + 1] - ch.in_off[i], 0xFFFFFFFFull);
                        ch.hit[i] = RTX_TRIM_NO_PATTERN | RTX_TRIM_NO_PATTERN << 16;
                    }
                }
                const double t_q0 = now();
                if (!rc && qual) {  // every read's range as the primers left it; a discarded read goes on empty
                    ch.q_hi.resize(ch.nq);
                    ch.q_verdict.resize(ch.nq);
                    ch.q_ee.resize(ch.nq);
                    ch.keep_hi.resize(ch.nq);
                    rc = rtx_qual_run(qualstages.of[c % n_dev], ch.nq, ch.in_bases, ch.in_quals, ch.in_off, ch.lo.data(), ch.hi.data(), ch.q_hi.data(), ch.q_ee.data(),
                                      ch.q_verdict.data());
                    if (!rc)
                        for (uint64_t i = 0; i < ch.nq; i++) {
                            const uint32_t v = ch.q_verdict[i];
                            ch.keep_hi[i] = v ? ch.lo[i] : ch.q_hi[i];
                            qual_passed += v == 0u;
                            qual_truncated += v == 0u && ch.q_hi[i] < ch.hi[i];
                            for (uint32_t b = 0; b < 7u; b++) qual_reasons[b] += (v >> b) & 1u;
                        }
                }
                const std::vector<uint32_t> &keep_hi = qual ? ch.keep_hi : ch.hi;
                bool any = false;
                if (!rc)
                    for (uint64_t i = 0; i < ch.nq && !any; i++) any = ch.lo[i] != 0u || keep_hi[i] != ch.in_off[i + 1] - ch.in_off[i];
                if (!rc && any) {  // (a chunk in which nothing was cut goes on as it came, without a copy)
                    uint64_t kept = 0;
                    for (uint64_t i = 0; i < ch.nq; i++) kept += keep_hi[i] - ch.lo[i];
                    {
                        std::lock_guard<std::mutex> g(pool_mu);
                        if (!bases_pool.empty()) { ch.t_bases = std::move(bases_pool.back()); bases_pool.pop_back(); }
                    }
                    if (!ch.t_bases.reserve(kept + 1)) { fail(RTX_ERR_OOM, "no memory for the trimmed reads of a chunk"); return; }
                    ch.t_off.resize(ch.nq + 1);
                    rc = rtx_trim_apply(ch.nq, ch.in_bases, ch.in_off, ch.lo.data(), keep_hi.data(), ch.t_bases.p, ch.t_off.data());
                    if (!rc) {
                        ch.dev_bases = ch.src_bases = ch.t_bases.p;
                        ch.dev_off = ch.src_off = ch.t_off.data();
                    }
                }
                if (rc) { fail(rc, rtx_last_error()); return; }
                if (trim) { trim_queries += ch.nq; busy_trim += (qual ? t_q0 : now()) - t_t0; }
                if (qual) { qual_queries += ch.nq; busy_qual += now() - t_q0; }
                if (!derep && !chim && dev_lookup[c % n_dev]) { set_stage(c, 1); continue; }
            }
            if (derep) {  // the copies of the chunk, on the device (a stream of its own beside the handle's); then the map's host side
                const double t_r0 = now();
                std::vector<uint32_t> rep(ch.nq);
                uint64_t nu = 0;
                int rc = rtx_derep_run(dereps.of[c % n_dev], ch.nq, ch.src_bases, ch.src_off, rep.data(), &nu);
                if (!rc && nu < ch.nq) {  // (a chunk without copies goes on as it came)
                    std::vector<uint32_t> uniq(ch.nq);
                    ch.slot.resize(ch.nq);
                    ch.size.resize(ch.nq);
                    rc = rtx_derep_plan(ch.nq, rep.data(), uniq.data(), ch.slot.data(), ch.size.data(), &nu);
                    if (!rc) {
                        ch.size.resize(nu);
                        ch.u_off.assign(nu + 1, 0);
                        for (uint64_t u = 0; u < nu; u++) ch.u_off[u + 1] = ch.u_off[u] + (ch.src_off[uniq[u] + 1] - ch.src_off[uniq[u]]);
                        {
                            std::lock_guard<std::mutex> g(pool_mu);
                            if (!bases_pool.empty()) { ch.u_bases = std::move(bases_pool.back()); bases_pool.pop_back(); }
                        }
                        if (!ch.u_bases.reserve(ch.u_off[nu] + 1)) { fail(RTX_ERR_OOM, "no memory for the distinct reads of a chunk"); return; }
                        // runs of neighbouring distinct reads that are neighbours in the input as well (most of a chunk with few copies) move in one memcpy
                        parallel_ranges(nu, nt_lookup, [&](uint64_t a, uint64_t b) {
                            for (uint64_t u = a; u < b;) {
                                uint64_t v = u + 1;
                                while (v < b && uniq[v] == uniq[v - 1] + 1u) v++;
                                if (ch.u_off[v] > ch.u_off[u]) memcpy(ch.u_bases.p + ch.u_off[u], ch.src_bases + ch.src_off[uniq[u]], ch.u_off[v] - ch.u_off[u]);
                                u = v;
                            }
                        });
                        ch.nu = nu;
                        ch.dev_bases = ch.u_bases.p;
                        ch.dev_off = ch.u_off.data();
                    }
                }
                if (rc) { fail(rc, rtx_last_error()); return; }
                derep_queries += ch.nq;
                derep_distinct += ch.nu;
                busy_derep += now() - t_r0;
                if (!chim && dev_lookup[c % n_dev]) { set_stage(c, 1); continue; }
            }
            if (chim) {  // the reads that go to the handle, on the device (a stream of its own beside the handle's); a flagged one goes on empty
                const double t_c0 = now();
                ch.chim.resize(ch.nu);
                int rc = rtx_chimera_run(chims.of[c % n_dev], ch.nu, ch.dev_bases, ch.dev_off, ch.chim.data());
                bool any = false;
                for (uint64_t u = 0; u < ch.nu && !rc && !any; u++) any = ch.chim[u].flag != 0u;
                if (!rc && any) {  // (a chunk without a flagged read goes on as it came, without a copy)
                    std::vector<uint32_t> lo(ch.nu, 0u), hi(ch.nu);
                    uint64_t kept = 0;
                    for (uint64_t u = 0; u < ch.nu; u++) {  // (a flagged read has at most RTX_CHIMERA_MAX_QUERY bases; a longer one is not checked and is not cut here)
                        const uint64_t len = ch.dev_off[u + 1] - ch.dev_off[u];
                        if (!ch.chim[u].flag && len > 0xFFFFFFFFull) { rc = RTX_ERR_INVALID; rtx::set_error("rtx_raxtax: a read of 2^32 bases or more with the chimera check set"); break; }
                        hi[u] = ch.chim[u].flag ? 0u : (uint32_t)len;
                        kept += hi[u];
                    }
                    if (!rc) {
                        {
                            std::lock_guard<std::mutex> g(pool_mu);
                            if (!bases_pool.empty()) { ch.c_bases = std::move(bases_pool.back()); bases_pool.pop_back(); }
                        }
                        if (!ch.c_bases.reserve(kept + 1)) { fail(RTX_ERR_OOM, "no memory for the checked reads of a chunk"); return; }
                        ch.c_off.resize(ch.nu + 1);
                        rc = rtx_trim_apply(ch.nu, ch.dev_bases, ch.dev_off, lo.data(), hi.data(), ch.c_bases.p, ch.c_off.data());
                    }
                    if (!rc) {
                        ch.dev_bases = ch.c_bases.p;
                        ch.dev_off = ch.c_off.data();
                    }
                }
                if (rc) { fail(rc, rtx_last_error()); return; }
                chim_queries += ch.nq;
                chim_checked += ch.nu;
                for (uint64_t i = 0; i < ch.nq; i++) chim_flagged += ch.chim[ch.slot.empty() ? i : ch.slot[i]].flag != 0u;
                busy_chim += now() - t_c0;
                if (dev_lookup[c % n_dev]) { set_stage(c, 1); continue; }
            }
            const double t_l0 = now();
            std::vector<const uint32_t *> ptr(ch.nu);
            std::vector<uint32_t> cnt(ch.nu);
            parallel_ranges(ch.nu, nt_lookup, [&](uint64_t a, uint64_t b) {
                for (uint64_t i = a; i < b; i++) {
                    const uint32_t *ids = nullptr;
                    cnt[i] = (uint32_t)rtx_tree_exact_matches(tree, ch.dev_bases + ch.dev_off[i], ch.dev_off[i + 1] - ch.dev_off[i], &ids);
                    ptr[i] = ids;
                }
            });
            ch.exact_off.assign(ch.nu + 1, 0);
            for (uint64_t i = 0; i < ch.nu; i++) ch.exact_off[i + 1] = ch.exact_off[i] + cnt[i];
            ch.exact_ids.resize(ch.exact_off[ch.nu]);
            for (uint64_t i = 0; i < ch.nu; i++) std::copy(ptr[i], ptr[i] + cnt[i], ch.exact_ids.begin() + ch.exact_off[i]);
            busy_lookup += now() - t_l0;
            set_stage(c, 1);
        }
    });

    // The device stage of a handle: activate -> run -> STAGE THE NEXT CHUNK -> download.  The queries of chunk c + n_dev are packed (two
    // bases per byte, pinned memory) and cross PCIe on the handle's transfer stream while the kernels of chunk c run
    // (rtx_batch_prefetch / rtx_batch_activate): the reference's workers pick up their next chunk without a pause either (raxtax.rs:35-36).
    auto stage_chunk = [&](uint32_t d, uint64_t c) -> int {
        Chunk &ch = chunks[c];
        if (dev_text[d]) {  // the labels travel with the chunk (the same input set)
            const int rc = rtx_batch_prefetch_labels(indices[d], ch.nq, labels + ch.q0);
            if (rc) return rc;
        }
        if (prof && !ch.size.empty()) {  // a distinct read counts with its copies in the open profile (the same input set as well)
            const int rc = rtx_batch_prefetch_weights(indices[d], ch.nu, ch.size.data());
            if (rc) return rc;
        }
        if (prof_samples && demux) {  // the sample of every read for the per-sample counters (no dereplication beside them: nu == nq)
            const int rc = rtx_batch_prefetch_samples(indices[d], ch.nq, ch.dx_sample.data());
            if (rc) return rc;
        }
        if (dev_lookup[d]) return rtx_batch_prefetch(indices[d], ch.nu, ch.dev_bases, ch.dev_off, nullptr, nullptr);
        return rtx_batch_prefetch(indices[d], ch.nu, ch.dev_bases, ch.dev_off, ch.exact_ids.empty() ? nullptr : ch.exact_ids.data(), ch.exact_off.data());
    };
    auto device_loop = [&](uint32_t d) {
        bool running = false;  // the kernels of chunk c have been enqueued already (behind the download of the chunk before it)
        for (uint64_t c = d; c < n_chunks; c += n_dev) {
            if (!wait_stage(c, 1)) return;
            // the result set of this handle's second-last chunk is reused now (device text: the sender reads the text of that set itself)
            if (c >= ahead && !wait_stage(c - ahead, dev_text[d] ? 4 : 3)) return;
            Chunk &ch = chunks[c];
            const double t_d0 = now();
            int rc = RTX_OK;
            if (!running) {  // the handle's first chunk
                rc = stage_chunk(d, c);
                if (!rc) rc = rtx_batch_activate(indices[d]);
                if (!rc) rc = rtx_batch_run(indices[d], flags);
            }
            running = false;
            const uint64_t nxt = c + n_dev;
            bool staged = false;
            if (!rc && nxt < n_chunks) {
                if (!wait_stage(nxt, 1)) return;   // its exact-match ids (host lookup), ready long ago as a rule
                rc = stage_chunk(d, nxt);
                staged = !rc;
            }
            // the device goes on with the next chunk as soon as the last records of this one have left it: the host's finalisation of
            // the last sub-batch (and this thread's bookkeeping) no longer stand between two chunks (rtx_batch_download_then_run)
            if (!rc) rc = staged ? rtx_batch_download_then_run(indices[d], &ch.res, flags) : rtx_batch_download(indices[d], &ch.res);
            if (rc == RTX_RETRY_CHUNK) {  // the run-ahead was abandoned (this chunk outgrew a buffer with the next one enqueued already): this chunk on its own
                rc = dev_text[d] ? rtx_batch_prefetch_labels(indices[d], ch.nq, labels + ch.q0) : RTX_OK;
                if (!rc && prof && !ch.size.empty()) rc = rtx_batch_prefetch_weights(indices[d], ch.nu, ch.size.data());
                if (!rc && prof_samples && demux) rc = rtx_batch_prefetch_samples(indices[d], ch.nq, ch.dx_sample.data());
                if (!rc) rc = dev_lookup[d] ? rtx_batch_upload(indices[d], ch.nu, ch.dev_bases, ch.dev_off, nullptr, nullptr)
                                   : rtx_batch_upload(indices[d], ch.nu, ch.dev_bases, ch.dev_off, ch.exact_ids.empty() ? nullptr : ch.exact_ids.data(), ch.exact_off.data());
                if (!rc) rc = rtx_batch_run(indices[d], flags);
                if (!rc) rc = rtx_batch_download(indices[d], &ch.res);
                staged = false;  // (the next chunk is staged, activated and run at the head of the loop)
            }
            if (!rc && staged) running = true;
            if (!rc && dev_text[d]) rc = rtx_batch_text(indices[d], &ch.text);
            if (!rc && dev_lookup[d]) {
                const uint64_t *xo = nullptr;
                const uint32_t *xi = nullptr;
                rc = rtx_batch_exact_matches(indices[d], &xo, &xi);
                if (!rc) {  // copied: the format thread reads them while the next chunk is classified
                    ch.exact_off.assign(xo, xo + ch.nu + 1);
                    ch.exact_ids.assign(xi, xi + xo[ch.nu]);
                }
            }
            if (!rc && want_strands) {
                const uint8_t *st = nullptr;
                const uint32_t *pk = nullptr;
                rc = rtx_batch_strands(indices[d], &st, &pk);
                if (!rc) {  // (per query of the caller, as everything the sender reads)
                    if (ch.slot.empty()) {
                        ch.strand.assign(st, st + ch.nq);
                        ch.peak.assign(pk, pk + ch.nq);
                    } else {
                        ch.strand.resize(ch.nq);
                        ch.peak.resize(ch.nq);
                        for (uint64_t i = 0; i < ch.nq; i++) { ch.strand[i] = st[ch.slot[i]]; ch.peak[i] = pk[ch.slot[i]]; }
                    }
                }
            }
            if (!rc && near && info) {
                const uint32_t *nr = nullptr, *ti = nullptr;
                rc = rtx_batch_nearest(indices[d], &nr, &ti);
                if (!rc) {
                    if (ch.slot.empty()) {
                        ch.nearest.assign(nr, nr + ch.nq);
                        ch.ties.assign(ti, ti + ch.nq);
                    } else {
                        ch.nearest.resize(ch.nq);
                        ch.ties.resize(ch.nq);
                        for (uint64_t i = 0; i < ch.nq; i++) { ch.nearest[i] = nr[ch.slot[i]]; ch.ties[i] = ti[ch.slot[i]]; }
                    }
                }
            }
            if (!rc && ident && info) {
                const uint32_t *di = nullptr;
                rc = rtx_batch_identity(indices[d], &di, nullptr);
                if (!rc) {
                    if (ch.slot.empty()) {
                        ch.dist.assign(di, di + ch.nq);
                    } else {  // (a copy has its representative's bases, and so its distance)
                        ch.dist.resize(ch.nq);
                        for (uint64_t i = 0; i < ch.nq; i++) ch.dist[i] = di[ch.slot[i]];
                    }
                }
            }
            if (rc) { fail(rc, rtx_last_error()); return; }
            busy_device[d] += now() - t_d0;
            set_stage(c, 2);
        }
    };

    auto format_loop = [&](uint32_t d) {
        WorkerPool pool(nt_format > 1 ? nt_format : 0);
        for (uint64_t c = d; c < n_chunks; c += n_dev) {
            if (!wait_stage(c, 2)) return;
            if (c >= 2 * ahead && !wait_stage(c - 2 * ahead, 4)) return;  // bounded memory: the sender is at most 4 chunks per handle behind
            Chunk &ch = chunks[c];
            const double t_f0 = now();
            ch.differ.assign(ch.nq, 0);
            if (ch.slot.empty()) {
                ch.status.assign(ch.res.status, ch.res.status + ch.nq);
                ch.t.assign(ch.res.t, ch.res.t + ch.nq);
            } else {
                ch.status.resize(ch.nq);
                ch.t.resize(ch.nq);
                for (uint64_t i = 0; i < ch.nq; i++) { ch.status[i] = ch.res.status[ch.slot[i]]; ch.t[i] = ch.res.t[ch.slot[i]]; }
            }
            ch.msg_off.assign(ch.nq, 0);
            ch.msg_arena.assign(ch.nq, 0);
            if (tsv) ch.tsv_off.assign(ch.nq, 0);
            const unsigned nt_f = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt_format, (ch.nq + 255) / 256));
            ch.out_arena.clear();
            ch.tsv_arena.clear();
            {   // arenas the sender is done with come back through the pool: a fresh megabyte per thread and chunk was a page fault per 4 KB of text
                std::lock_guard<std::mutex> g(pool_mu);
                for (unsigned r = 0; r < nt_f * (tsv ? 2u : 1u); r++) {
                    std::vector<Chunk::Arena> &dst = r < nt_f ? ch.out_arena : ch.tsv_arena;
                    if (!arena_pool.empty()) { dst.push_back(std::move(arena_pool.back())); arena_pool.pop_back(); }
                    else dst.emplace_back();
                    dst.back().len = 0;
                }
            }
            std::atomic<int> rc_fmt{0};
            auto format_range = [&](unsigned r) {
                const uint64_t a = ch.nq * r / nt_f, b = ch.nq * (r + 1) / nt_f;
                // (worked on as locals and handed back: the arenas of neighbouring threads share cache lines in the vector, and `len` moves per query)
                Chunk::Arena oa = std::move(ch.out_arena[r]), tsv_local;
                if (tsv) tsv_local = std::move(ch.tsv_arena[r]);
                Chunk::Arena *ta = tsv ? &tsv_local : nullptr;
                struct Back {
                    Chunk &c; unsigned r; Chunk::Arena &o, *t;
                    ~Back() { c.out_arena[r] = std::move(o); if (t) c.tsv_arena[r] = std::move(*t); }
                } back{ch, r, oa, ta};
                std::vector<uint8_t> rc_seq;  // a minus-strand query prints the orientation that was classified (the `.tsv` sequence column)
                // The rows of a view lie in the PROCESSING order of the batch and the queries are formatted in input order: every row array
                // (confidences: 256 bytes per row, lineage, depth, local signal) and the lineage string are cache misses per query -- what
                // the stage waited for (0.6 us per query on sixteen threads where the arithmetic needs 0.2).  Three prefetch stages ahead of
                // the formatting: the row arrays of query i + 24, the string object of i + 16 (its index has arrived), the characters of i + 8.
                // (j, i: queries of the caller; the view is read at their representative's position at(.), RTX_OPT_DEREP)
                const uint32_t *const slot = ch.slot.empty() ? nullptr : ch.slot.data();
                auto at = [slot](uint64_t j) -> uint64_t { return slot ? slot[j] : j; };
                auto row_of = [&](uint64_t j) { return ch.res.row_begin[at(j)]; };
                auto has_rows = [&](uint64_t j) { const uint64_t s = at(j); return ch.res.status[s] == RTX_Q_OK && ch.res.row_count[s] != 0; };
                auto stage1 = [&](uint64_t j) {
                    if (j >= b || !has_rows(j)) return;
                    const uint64_t r = row_of(j);
                    __builtin_prefetch(ch.res.row_conf + r * (ch.res.row_conf_stride ? ch.res.row_conf_stride : RTX_MAX_DEPTH));
                    __builtin_prefetch(ch.res.row_lineage + r);
                    __builtin_prefetch(ch.res.row_depth + r);
                    __builtin_prefetch(ch.res.row_local_signal + r);
                };
                auto stage2 = [&](uint64_t j) {
                    if (j >= b) return;
                    __builtin_prefetch(labels[ch.q0 + j]);  // (the labels are the caller's strings, one allocation each)
                    if (!has_rows(j)) return;
                    __builtin_prefetch(&tree->lineages[ch.res.row_lineage[row_of(j)]]);
                };
                auto stage3 = [&](uint64_t j) {
                    if (j >= b || !has_rows(j)) return;
                    const std::string &l = tree->lineages[ch.res.row_lineage[row_of(j)]];
                    __builtin_prefetch(l.data());
                    __builtin_prefetch(l.data() + 64);
                };
                const bool pre = !dev_text[d];  // (the prefetches serve the host formatter)
                if (pre) {
                    for (uint64_t j = a; j < std::min<uint64_t>(b, a + 24); j++) stage1(j);
                    for (uint64_t j = a; j < std::min<uint64_t>(b, a + 16); j++) stage2(j);
                    for (uint64_t j = a; j < std::min<uint64_t>(b, a + 8); j++) stage3(j);
                }
                for (uint64_t i = a; i < b; i++) {
                    if (pre) {
                        stage1(i + 24);
                        stage2(i + 16);
                        stage3(i + 8);
                    }
                    const uint64_t q = ch.q0 + i, s = at(i);
                    const uint64_t ne = ch.exact_off[s + 1] - ch.exact_off[s];
                    if (!skip_exact_matches && ne > 1) {  // raxtax.rs:43-53 (the info! lines go to the log in the CLI)
                        const uint32_t *ids = ch.exact_ids.data() + ch.exact_off[s];
                        auto parent = [&](uint32_t id) {
                            const std::string &l = tree->lineages[id];
                            const size_t k = l.rfind(',');
                            return k == std::string::npos ? std::string_view() : std::string_view(l).substr(0, k);
                        };
                        for (uint64_t j = 1; j < ne; j++)
                            if (parent(ids[j]) != parent(ids[0])) { ch.differ[i] = 1; break; }
                    }
                    if (dev_text[d] || ch.res.status[s] != RTX_Q_OK) continue;  // (device text: the lines are formatted already)
                    const uint64_t len = ch.src_off[i + 1] - ch.src_off[i];  // (the read as it was classified: trimmed, with primers set)
                    const uint64_t rows = ch.res.row_count[s];
                    const size_t need = (rows + 1) * (strlen(labels[q]) + 4096 + 8 * RTX_MAX_DEPTH) + len + 64;
                    char *ob = oa.room(need);
                    char *tb = ta ? ta->room(need + rows * len) : nullptr;
                    if (!ob || (ta && !tb)) { rc_fmt = RTX_ERR_OOM; return; }
                    int64_t tsv_len = 0;
                    const uint8_t *seq = ch.src_bases + ch.src_off[i];
                    if (tb && both && ch.strand[i]) {
                        rc_seq.resize(len + 1);
                        (void)rtx_revcomp(seq, len, rc_seq.data());
                        seq = rc_seq.data();
                    }
                    const int64_t n = rtx_format_query(tree, &ch.res, s, labels[q], seq, len,
                                                       ch.exact_ids.data() + ch.exact_off[s], ne, flags, ob, need,
                                                       tb, tb ? need + rows * len : 0, &tsv_len);
                    if (n < 0) { rc_fmt = (int)n; return; }
                    ch.msg_arena[i] = r;
                    ch.msg_off[i] = oa.len;
                    oa.len += (size_t)n + 1;  // (rtx_format_query terminates its text)
                    if (ta) { ch.tsv_off[i] = ta->len; ta->len += (size_t)tsv_len + 1; }
                }
            };
            pool.run(nt_f, format_range);
            if (rc_fmt) { fail(rc_fmt, "formatting a result failed"); return; }
            busy_format[d] += now() - t_f0;
            set_stage(c, 3);
        }
    };

    std::vector<std::thread> workers;
    for (uint32_t d = 0; d < n_dev; d++) {
        workers.emplace_back(device_loop, d);
        workers.emplace_back(format_loop, d);
    }
    // the sender: messages in input order
    for (uint64_t c = 0; c < n_chunks; c++) {
        if (!wait_stage(c, 3)) break;
        Chunk &ch = chunks[c];
        const double t_s0 = now();
        bool closed = false;
        for (uint64_t i = 0; i < ch.nq && !closed; i++) {
            const uint64_t q = ch.q0 + i;
            if (ch.differ[i]) {
                fprintf(stderr, "[WARN ] Exact matches for %s differ above the leafs of the lineage tree!\n", labels[q]);
                warnings = true;
            }
            if (demux_cb) {  // every query, also one without a message (a read that is not assigned)
                const uint32_t raw = (uint32_t)std::min<uint64_t>(base_off[q + 1] - base_off[q], 0xFFFFFFFFull);
                const bool on = !ch.dx_info.empty();
                if (!demux_cb(labels[q], raw, on ? ch.dx_sample[i] : RTX_DEMUX_NONE, on ? ch.dx_lo[i] : 0u, on ? ch.dx_hi[i] : raw,
                              on ? ch.dx_hit[i] : (RTX_DEMUX_NO_TAG | RTX_DEMUX_NO_TAG << 16), on ? ch.dx_info[i] : 0u)) { closed = true; break; }
            }
            if (trim_cb) {  // every query, also one without a message (an emptied read)
                const uint32_t raw = (uint32_t)std::min<uint64_t>(ch.in_off[i + 1] - ch.in_off[i], 0xFFFFFFFFull);
                const bool on = !ch.lo.empty();
                if (!trim_cb(labels[q], raw, on ? ch.lo[i] : 0u, on ? ch.hi[i] : raw, on ? ch.hit[i] : (RTX_TRIM_NO_PATTERN | RTX_TRIM_NO_PATTERN << 16))) { closed = true; break; }
            }
            if (qual_cb) {  // likewise
                const uint32_t raw = (uint32_t)std::min<uint64_t>(ch.in_off[i + 1] - ch.in_off[i], 0xFFFFFFFFull);
                const bool ranged = !ch.lo.empty(), on = !ch.q_hi.empty();
                if (!qual_cb(labels[q], raw, ranged ? ch.lo[i] : 0u, on ? ch.q_hi[i] : (ranged ? ch.hi[i] : raw), on ? ch.q_ee[i] : 0ull, on ? ch.q_verdict[i] : 0u)) { closed = true; break; }
            }
            if (chim_cb) {  // likewise; a copy takes its representative's record
                static const rtx_chimera_rec none{RTX_CHIM_OK, 0u, 0u, RTX_NO_REF, 0u, 0u, 0u, RTX_NO_REF, 0u, RTX_NO_REF, 0u, 0u};
                if (!chim_cb(labels[q], ch.chim.empty() ? &none : &ch.chim[ch.slot.empty() ? i : ch.slot[i]])) { closed = true; break; }
            }
            if (ch.status[i] != RTX_Q_OK) {
                // the reference aborts here (prob.rs:21/162); report and skip the query instead
                if (ch.status[i] == RTX_Q_ALL_KMERS) fprintf(stderr, "[ERROR] query %s holds every 8-mer (t = 65536): the reference asserts t < 65536 (raxtax.rs:56)\n", labels[q]);
                else fprintf(stderr, "[ERROR] query %s has too few valid 8-mers (%u) to be classified\n", labels[q], ch.t[i]);
                continue;
            }
            bool ok;
            if (info && !info(labels[q], ch.strand[i], ch.peak[i], ch.t[i], near ? ch.nearest[i] : RTX_NO_REF, near ? ch.ties[i] : 0u,
                              ident ? ch.dist[i] : RTX_NO_DIST, (uint32_t)std::min<uint64_t>(ch.src_off[i + 1] - ch.src_off[i], 0xFFFFFFFFull))) { closed = true; break; }
            if (dev_text[c % n_dev]) {
                ok = sender(labels[q], ch.text.out + ch.text.out_off[i], tsv ? ch.text.tsv + ch.text.tsv_off[i] : nullptr);
            } else {
                const uint32_t r = ch.msg_arena[i];
                ok = sender(labels[q], ch.out_arena[r].p + ch.msg_off[i], tsv ? ch.tsv_arena[r].p + ch.tsv_off[i] : nullptr);
            }
            if (!ok) closed = true;
        }
        if (closed) { fail(RTX_ERR_SENDER, "result sink closed"); break; }  // sender.send(..)?, raxtax.rs:87
        std::vector<uint32_t>().swap(ch.exact_ids);
        std::vector<uint64_t>().swap(ch.exact_off);
        std::vector<uint8_t>().swap(ch.differ);
        std::vector<uint8_t>().swap(ch.status);
        std::vector<uint32_t>().swap(ch.t);
        std::vector<uint8_t>().swap(ch.strand);
        std::vector<uint32_t>().swap(ch.peak);
        std::vector<uint32_t>().swap(ch.nearest);
        std::vector<uint32_t>().swap(ch.ties);
        std::vector<uint32_t>().swap(ch.slot);
        std::vector<uint32_t>().swap(ch.size);
        std::vector<uint64_t>().swap(ch.u_off);
        std::vector<uint32_t>().swap(ch.lo);
        std::vector<uint32_t>().swap(ch.hi);
        std::vector<uint32_t>().swap(ch.hit);
        std::vector<uint32_t>().swap(ch.q_hi);
        std::vector<uint32_t>().swap(ch.q_verdict);
        std::vector<uint32_t>().swap(ch.keep_hi);
        std::vector<uint64_t>().swap(ch.q_ee);
        std::vector<uint64_t>().swap(ch.t_off);
        std::vector<rtx_chimera_rec>().swap(ch.chim);
        std::vector<uint64_t>().swap(ch.c_off);
        for (auto *v : {&ch.dx_sample, &ch.dx_lo, &ch.dx_hi, &ch.dx_hit, &ch.dx_info}) std::vector<uint32_t>().swap(*v);
        std::vector<uint64_t>().swap(ch.x_off);
        {
            std::lock_guard<std::mutex> g(pool_mu);
            if (ch.x_bases.p) bases_pool.push_back(std::move(ch.x_bases));
            if (ch.x_quals.p) bases_pool.push_back(std::move(ch.x_quals));
            if (ch.u_bases.p) bases_pool.push_back(std::move(ch.u_bases));
            if (ch.t_bases.p) bases_pool.push_back(std::move(ch.t_bases));
            if (ch.c_bases.p) bases_pool.push_back(std::move(ch.c_bases));
            for (auto &a : ch.out_arena) arena_pool.push_back(std::move(a));
            for (auto &a : ch.tsv_arena) arena_pool.push_back(std::move(a));
        }
        std::vector<Chunk::Arena>().swap(ch.out_arena);
        std::vector<Chunk::Arena>().swap(ch.tsv_arena);
        std::vector<uint64_t>().swap(ch.msg_off);
        std::vector<uint64_t>().swap(ch.tsv_off);
        std::vector<uint32_t>().swap(ch.msg_arena);
        busy_send += now() - t_s0;
        set_stage(c, 4);
    }
    lookup.join();
    for (auto &t : workers) t.join();
    {
        double bd = 0, bf = 0;
        for (uint32_t d = 0; d < n_dev; d++) { bd = std::max(bd, busy_device[d]); bf = std::max(bf, busy_format[d]); }
        std::lock_guard<std::mutex> g(g_timing_mu);
        g_timing = {{any_host_lookup ? busy_lookup : 0.0, bd, bf, busy_send}, n_chunks};
        g_derep = {derep_queries, derep_distinct, busy_derep};
        g_trim = {trim_queries, trim_with5, trim_with3, trim_emptied, busy_trim};
        g_chim = {chim_queries, chim_checked, chim_flagged, busy_chim};
        g_demux = {demux_queries, demux_assigned, {demux_reasons[0], demux_reasons[1], demux_reasons[2], demux_reasons[3], demux_reasons[4]}, busy_demux};
        g_qual = {qual_queries, qual_passed, qual_truncated, {qual_reasons[0], qual_reasons[1], qual_reasons[2], qual_reasons[3], qual_reasons[4], qual_reasons[5], qual_reasons[6]}, busy_qual};
    }
    if (failed != RTX_OK) { rtx::set_error("%s", failed_msg.c_str()); return failed; }
    if (warnings)  // raxtax.rs:93-95
        fprintf(stderr, "\x1b[33m[WARN ]\x1b[0m Exact matches for some queries differ above the species level! Check the log file for more information!\n");
    return RTX_OK;
}

}  // namespace

namespace raxtax {

int raxtax(const std::vector<std::pair<std::string, std::vector<uint8_t>>> &queries, const rtx_tree *tree,
           rtx_index *index, bool skip_exact_matches, bool raw_confidence, size_t chunk_size, const Sender &sender,
           bool tsv) {
    std::vector<const char *> labels(queries.size());
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off(queries.size() + 1, 0);
    for (size_t i = 0; i < queries.size(); i++) {
        labels[i] = queries[i].first.c_str();
        bases.insert(bases.end(), queries[i].second.begin(), queries[i].second.end());
        off[i + 1] = bases.size();
    }
    // (the C++ face hands out owned strings, as the reference's channel does)
    RawSender raw = [&](const char *label, const char *out, const char *t) {
        return sender(std::string(label), std::string(out), t ? std::optional<std::string>(std::string(t)) : std::nullopt);
    };
    return run(&index, 1, tree, queries.size(), labels.data(), bases.data(), off.data(), skip_exact_matches, raw_confidence,
               chunk_size, raw, tsv);
}

}  // namespace raxtax

extern "C" int rtx_raxtax(rtx_index *index, const rtx_tree *tree, uint64_t n_queries, const char *const *labels,
                          const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches, int raw_confidence,
                          uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv) {
    if (!sender) { rtx::set_error("rtx_raxtax: null sender"); return RTX_ERR_INVALID; }
    return rtx_raxtax_multi_ex(&index, 1, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender, sender_ctx,
                               tsv, nullptr, nullptr);
}

// The same over several device handles (one per GPU, or several on one): the reference's parallel driver is one call inside the
// process as well (par_chunks over a rayon pool, raxtax.rs:35-36, main.rs:40-57).  Chunks of `chunk_size` queries are dealt to the
// handles in turn, one driving thread per handle; the messages reach the sender in input order.
extern "C" int rtx_raxtax_multi(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv) {
    return rtx_raxtax_multi_ex(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender,
                               sender_ctx, tsv, nullptr, nullptr);
}

// ... with `info` called directly before the sender for every query that has a message: its label, strand, peak and t
extern "C" int rtx_raxtax_multi_ex(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                   const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                   int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                   rtx_query_info_fn info, void *info_ctx) {
    if (!sender) { rtx::set_error("rtx_raxtax_multi: null sender"); return RTX_ERR_INVALID; }
    RawSender s = [&](const char *label, const char *out, const char *t) { return sender(sender_ctx, label, out, t) == 0; };
    RawInfo fi;
    if (info) fi = [&](const char *label, int strand, uint32_t peak, uint32_t t, uint32_t, uint32_t, uint32_t, uint32_t) { return info(info_ctx, label, strand, peak, t) == 0; };
    return run(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches != 0, raw_confidence != 0, chunk_size, s,
               tsv != 0, fi);
}

// ... with the nearest reference and its ties as well (RTX_OPT_NEAREST)
extern "C" int rtx_raxtax_multi_ex2(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_hit_fn hit, void *hit_ctx) {
    if (!sender) { rtx::set_error("rtx_raxtax_multi: null sender"); return RTX_ERR_INVALID; }
    RawSender s = [&](const char *label, const char *out, const char *t) { return sender(sender_ctx, label, out, t) == 0; };
    RawInfo fi;
    if (hit) fi = [&](const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t, uint32_t) { return hit(hit_ctx, label, strand, peak, t, nearest, ties) == 0; };
    return run(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches != 0, raw_confidence != 0, chunk_size, s,
               tsv != 0, fi);
}

// ... and the alignment identity (RTX_OPT_IDENTITY)
extern "C" int rtx_raxtax_multi_ex3(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx) {
    return rtx_raxtax_multi_ex4(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender,
                                sender_ctx, tsv, align, align_ctx, nullptr, nullptr);
}

// ... and the primer trimming of every query (rtx_index_set_primers)
extern "C" int rtx_raxtax_multi_ex4(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx) {
    return rtx_raxtax_multi_ex5(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender,
                                sender_ctx, tsv, align, align_ctx, trim, trim_ctx, nullptr, nullptr, nullptr);
}

// ... and the quality strings of the reads with the quality filter of every query (rtx_index_set_quality)
extern "C" int rtx_raxtax_multi_ex5(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx) {
    return rtx_raxtax_multi_ex6(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender,
                                sender_ctx, tsv, align, align_ctx, trim, trim_ctx, quals, qual, qual_ctx, nullptr, nullptr);
}

// ... and the chimera record of every query (rtx_index_set_chimera)
extern "C" int rtx_raxtax_multi_ex6(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx) {
    return rtx_raxtax_multi_ex7(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender,
                                sender_ctx, tsv, align, align_ctx, trim, trim_ctx, quals, qual, qual_ctx, chimera, chimera_ctx, nullptr, nullptr);
}

// ... and the sample of every query (rtx_index_set_tags)
extern "C" int rtx_raxtax_multi_ex7(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx, rtx_query_demux_fn demux,
                                    void *demux_ctx) {
    if (!sender) { rtx::set_error("rtx_raxtax_multi: null sender"); return RTX_ERR_INVALID; }
    RawSender s = [&](const char *label, const char *out, const char *t) { return sender(sender_ctx, label, out, t) == 0; };
    RawInfo fi;
    if (align)
        fi = [&](const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t dist, uint32_t qlen) {
            return align(align_ctx, label, strand, peak, t, nearest, ties, dist, qlen) == 0;
        };
    RawTrim ft;
    if (trim) ft = [&](const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint32_t hit) { return trim(trim_ctx, label, raw_len, lo, hi, hit) == 0; };
    RawQual fq;
    if (qual) fq = [&](const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint64_t ee, uint32_t verdict) { return qual(qual_ctx, label, raw_len, lo, hi, ee, verdict) == 0; };
    RawChim fc;
    if (chimera) fc = [&](const char *label, const rtx_chimera_rec *rec) { return chimera(chimera_ctx, label, rec) == 0; };
    RawDemux fx;
    if (demux)
        fx = [&](const char *label, uint32_t raw_len, uint32_t sample, uint32_t lo, uint32_t hi, uint32_t hit, uint32_t info) {
            return demux(demux_ctx, label, raw_len, sample, lo, hi, hit, info) == 0;
        };
    return run(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches != 0, raw_confidence != 0, chunk_size, s,
               tsv != 0, fi, ft, quals, fq, fc, fx);
}

extern "C" int rtx_raxtax_last_demux(uint64_t *queries, uint64_t *assigned, uint64_t reasons[5], double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_demux.queries;
    if (assigned) *assigned = g_demux.assigned;
    if (reasons) for (int v = 0; v < 5; v++) reasons[v] = g_demux.reasons[v];
    if (busy_seconds) *busy_seconds = g_demux.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_timing(double busy[4], uint64_t *n_chunks) {
    if (!busy) { rtx::set_error("rtx_raxtax_last_timing: null argument"); return RTX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(g_timing_mu);
    for (int i = 0; i < 4; i++) busy[i] = g_timing.busy[i];
    if (n_chunks) *n_chunks = g_timing.n_chunks;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_derep(uint64_t *queries, uint64_t *distinct, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_derep.queries;
    if (distinct) *distinct = g_derep.distinct;
    if (busy_seconds) *busy_seconds = g_derep.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_trim(uint64_t *queries, uint64_t *with5, uint64_t *with3, uint64_t *emptied, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_trim.queries;
    if (with5) *with5 = g_trim.with5;
    if (with3) *with3 = g_trim.with3;
    if (emptied) *emptied = g_trim.emptied;
    if (busy_seconds) *busy_seconds = g_trim.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_qual(uint64_t *queries, uint64_t *passed, uint64_t *truncated, uint64_t reasons[7], double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_qual.queries;
    if (passed) *passed = g_qual.passed;
    if (truncated) *truncated = g_qual.truncated;
    if (reasons) for (int b = 0; b < 7; b++) reasons[b] = g_qual.reasons[b];
    if (busy_seconds) *busy_seconds = g_qual.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_chimera(uint64_t *queries, uint64_t *checked, uint64_t *flagged, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_chim.queries;
    if (checked) *checked = g_chim.checked;
    if (flagged) *flagged = g_chim.flagged;
    if (busy_seconds) *busy_seconds = g_chim.busy;
    return RTX_OK;
}

// The host side of a dereplication map (rtx_derep_run): the distinct queries in ascending order, every query's position among them and the
// size of every cluster.  Refuses a map that is none: a representative behind its query, or one that is not its own representative.
extern "C" int rtx_derep_plan(uint64_t n, const uint32_t *rep, uint32_t *uniq, uint32_t *slot, uint32_t *size, uint64_t *n_unique) {
    if (n_unique) *n_unique = 0;
    if (n > 0xFFFFFFFFull || (n && (!rep || !uniq || !slot || !size))) { rtx::set_error("rtx_derep_plan: invalid argument"); return RTX_ERR_INVALID; }
    uint64_t nu = 0;
    for (uint64_t q = 0; q < n; q++) {
        const uint32_t r = rep[q];
        if (r > q || rep[r] != r) { rtx::set_error("rtx_derep_plan: rep[%llu] = %u is no representative (rep[q] <= q and rep[rep[q]] == rep[q])", (unsigned long long)q, r); return RTX_ERR_INVALID; }
        if (r == q) {
            uniq[nu] = (uint32_t)q;
            size[nu] = 1;
            slot[q] = (uint32_t)nu++;
        } else {
            slot[q] = slot[r];
            size[slot[r]]++;
        }
    }
    for (uint64_t u = nu; u < n; u++) uniq[u] = size[u] = 0;
    if (n_unique) *n_unique = nu;
    return RTX_OK;
}

// A sender that keeps nothing: counts the messages and their bytes into ctx (uint64_t[2]) if given.  For callers that time the
// path through rtx_raxtax without a disk behind it (bench.py: value_end_to_end).
extern "C" int rtx_sender_discard(void *ctx, const char *label, const char *out_lines, const char *tsv_lines) {
    (void)label;
    if (ctx) {
        uint64_t *c = static_cast<uint64_t *>(ctx);
        c[0] += 1;
        c[1] += (out_lines ? strlen(out_lines) : 0) + (tsv_lines ? strlen(tsv_lines) : 0);
    }
    return 0;
}

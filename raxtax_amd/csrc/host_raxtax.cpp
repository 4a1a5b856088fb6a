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
#include <tuple>

#include "host_front.hpp"
#include "rtx_internal.hpp"

namespace {

using rtx_front::BufPool;
using rtx_front::Front;
using rtx_front::FrontChunk;
using rtx_front::FrontTotals;
using rtx_front::parallel_ranges;
using rtx_front::Reads;

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

std::mutex g_timing_mu;
FrontTotals g_last{};  // the last call of this process: what the eight rtx_raxtax_last_* report (under g_timing_mu)

// The arguments of a call.  A callback is a function of the C ABI with its context (0: go on, else the sink is closed); null: nobody asked.
//   sender (label, out_lines, tsv_lines or null) of every query that has a message
//   align  (label, strand, peak, t, nearest, ties, dist, qlen) directly before it: RTX_NO_REF and 0 with RTX_OPT_NEAREST off, RTX_NO_DIST and the
//          length with RTX_OPT_IDENTITY off
//   demux, trim, qual, screen, chimera: of EVERY query, in this order, before its align call
struct Call {
    rtx_index *const *indices; uint32_t n_dev;
    const rtx_tree *tree;
    uint64_t n_queries;
    const char *const *labels;
    const uint8_t *bases; const uint64_t *base_off;
    bool skip_exact_matches, raw_confidence;
    uint64_t chunk_size;
    rtx_sender_fn sender; void *sender_ctx;
    bool tsv;
    const uint8_t *quals;
    rtx_query_align_fn align; void *align_ctx;
    rtx_query_trim_fn trim; void *trim_ctx;
    rtx_query_qual_fn qual; void *qual_ctx;
    rtx_query_chimera_fn chimera; void *chimera_ctx;
    rtx_query_demux_fn demux; void *demux_ctx;
    rtx_query_screen_fn screen; void *screen_ctx;
};

// The text of a formatting thread's queries: NUL-terminated messages back to back
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
    ~Arena() { free(p); }
    Arena() = default;
    Arena(const Arena &) = delete;
    Arena(Arena &&o) noexcept : p(o.p), cap(o.cap), len(o.len) { o.p = nullptr; o.cap = o.len = 0; }
    Arena &operator=(Arena &&o) noexcept {
        if (this != &o) { free(p); p = o.p; cap = o.cap; len = o.len; o.p = nullptr; o.cap = o.len = 0; }
        return *this;
    }
};

// One chunk of queries travelling through the stages of run().  The sender releases the three groups when the chunk is sent.
struct Chunk {
    uint64_t q0 = 0, nq = 0;
    FrontChunk front;  // the views of the chunk's reads and what the front said of them (host_front.hpp); front.dev: what the handle is given
    // What the stages copied out of the handle's result sets, which the handle reuses once this chunk is formatted; but for the
    // exact matches ([front.dev.n]) per query of the caller, as everything the sender reads
    struct Copies {
        std::vector<uint32_t> exact_ids;   // tree.sequences.get(query), raxtax.rs:42
        std::vector<uint64_t> exact_off;
        std::vector<uint8_t> differ;       // raxtax.rs:43-53: exact matches with different parents
        std::vector<uint8_t> status;       // res.status / res.t, by the format stage
        std::vector<uint32_t> t;
        std::vector<uint8_t> strand;       // rtx_batch_strands, by the device stage (both strands, or an align callback)
        std::vector<uint32_t> peak;
        std::vector<uint32_t> nearest, ties;  // rtx_batch_nearest (RTX_OPT_NEAREST and an align callback)
        std::vector<uint32_t> dist;           // rtx_batch_identity (RTX_OPT_IDENTITY and an align callback)
    } copies;
    // The messages of the chunk: every formatting thread appends the NUL-terminated `.out` (and `.tsv`) text of its queries to an arena
    // of its own; msg_off[i] locates query i's text in the arena of the thread that took it (a std::string per message was a malloc in
    // the format thread and a free in the sender's, per query: half of the format stage)
    struct Messages {
        std::vector<Arena> out_arena, tsv_arena;   // one per formatting thread
        std::vector<uint64_t> msg_off, tsv_off;    // [nq] offset of the query's text in its thread's arena
        std::vector<uint32_t> msg_arena;           // [nq] which arena
    } msg;
    rtx_text_view text{};              // RTX_OPT_DEVICE_TEXT: the messages as the device formatted them (valid as long as `res`)
    rtx_result_view res{};
    int stage = 0;                     // 1: exact matches looked up (or left to the device), 2: classified, 3: formatted, 4: sent
};

// dst[i] = src[slot[i]] per query of the caller; without a slot (no copies in the chunk, or RTX_OPT_DEREP off) src[i]
template <class T>
void per_query(std::vector<T> &dst, const T *src, const std::vector<uint32_t> &slot, uint64_t nq) {
    if (slot.empty()) { dst.assign(src, src + nq); return; }
    dst.resize(nq);
    for (uint64_t i = 0; i < nq; i++) dst[i] = src[slot[i]];
}

// raxtax() (src/raxtax.rs:14-97) as a pipeline over chunks of `chunk_size` queries on one or several device handles -- the
// reference's `par_chunks(chunk_size)` (raxtax.rs:35-36) with GPUs in the place of rayon workers.  Chunk c belongs to handle
// c mod n_dev; per handle
//   device thread : classification of its chunks, one after the other  (rtx_classify_batch, raxtax.rs:42,55-71)
//   format thread : lineage check of the exact matches (raxtax.rs:43-53), override + formatting (raxtax.rs:73-84), chunk by chunk
// and for all of them
//   lookup thread : the read front (host_front.hpp: tags, primers, quality, contaminants, copies, chimeras, distinct reads -- each on the device, on a stream of its own
//                   beside the handle's, while that handle still classifies an earlier chunk), then the exact-match ids (host hash map,
//                   raxtax.rs:42) -- only for handles without the device lookup (rtx_index_has_exact_lookup): otherwise the ids come back
//                   with the results of the device stage.  The handle classifies front.dev; the format thread and the sender go on
//                   per query of the caller (FrontChunk::slot)
//   calling thread: the sender, one message per query in INPUT order (raxtax.rs:85-87): chunk 0, 1, 2 ... as they become ready.
// A handle keeps two result sets, so the view of its k-th chunk stays valid until its (k + 2)-th is classified.
int run(const Call &call) {
    rtx_index *const *const indices = call.indices;
    const uint32_t n_dev = call.n_dev;
    const rtx_tree *const tree = call.tree;
    const char *const *const labels = call.labels;
    const bool tsv = call.tsv;
    if (!call.sender) { rtx::set_error("rtx_raxtax_multi: null sender"); return RTX_ERR_INVALID; }
    if (!indices || n_dev == 0 || !tree || !call.base_off || !labels) { rtx::set_error("rtx_raxtax: null argument"); return RTX_ERR_INVALID; }
    for (uint32_t d = 0; d < n_dev; d++) {
        if (!indices[d]) { rtx::set_error("rtx_raxtax: null index handle"); return RTX_ERR_INVALID; }
        if (rtx_index_num_refs(indices[d]) != tree->num_tips) { rtx::set_error("index and tree disagree on num_tips"); return RTX_ERR_INVALID; }
        for (uint32_t e = 0; e < d; e++)
            if (indices[e] == indices[d]) { rtx::set_error("rtx_raxtax_multi: the same handle twice (calls on one handle must be serialised)"); return RTX_ERR_INVALID; }
    }
    const uint64_t n_queries = call.n_queries;
    const uint64_t chunk_size = call.chunk_size == 0 || call.chunk_size > n_queries ? std::max<uint64_t>(1, (n_queries + n_dev - 1) / n_dev) : call.chunk_size;
    const uint32_t flags = (call.skip_exact_matches ? RTX_SKIP_EXACT_MATCHES : 0u) | (call.raw_confidence ? RTX_RAW_CONFIDENCE : 0u);
    const uint64_t n_chunks = (n_queries + chunk_size - 1) / chunk_size;
    // thread budget: this process's share of the host's CPUs (rtx::host_threads), split over the handles driven here
    const unsigned nt_lookup = rtx::host_threads(4u), nt_format = rtx::host_threads(16u, n_dev);
    std::vector<uint8_t> dev_lookup(n_dev), dev_text(n_dev);
    bool any_host_lookup = false;
    // RTX_OPT_STRAND: every handle classifies both orientations, or none does; the exact matches then come from the device (those of a
    // reverse complement belong to the same lookup) and the text from the host (the device formats the given orientation only)
    const bool both = rtx::index_strand(indices[0]);
    for (uint32_t d = 0; d < n_dev && rtx::index_strand(indices[d]) == both; d++)  // (handle by handle: up to the first that disagrees)
        if (both && !rtx_index_has_exact_lookup(indices[d])) { rtx::set_error("RTX_OPT_STRAND needs the exact-match lookup of the device (a handle built from the reference sequences)"); return RTX_ERR_STATE; }
    int rc = rtx_front::agree(indices, n_dev, rtx::index_strand, "rtx_raxtax_multi: the handles disagree on RTX_OPT_STRAND");
    const bool want_strands = both || call.align;
    const bool near = rtx::index_nearest(indices[0]);  // RTX_OPT_NEAREST: on every handle, or on none
    if (!rc) rc = rtx_front::agree(indices, n_dev, rtx::index_nearest, "rtx_raxtax_multi: the handles disagree on RTX_OPT_NEAREST");
    const bool ident = rtx::index_identity(indices[0]);  // RTX_OPT_IDENTITY: the same
    if (!rc) rc = rtx_front::agree(indices, n_dev, rtx::index_identity, "rtx_raxtax_multi: the handles disagree on RTX_OPT_IDENTITY");
    // an open taxon profile (rtx_index_profile_begin): on every handle or on none, with one cutoff, and with the flags of this call
    auto profile = [](const rtx_index *ix) {
        uint32_t c = 0, f = 0;
        return rtx::index_profile(ix, &c, &f) ? std::make_tuple(true, c, f) : std::make_tuple(false, 0u, 0u);
    };
    const bool prof = std::get<0>(profile(indices[0]));
    const uint32_t prof_flags = std::get<2>(profile(indices[0]));
    if (!rc) rc = rtx_front::agree(indices, n_dev, profile, "rtx_raxtax_multi: the handles disagree on their taxon profile (open on all or on none, one cutoff, one set of flags)");
    if (rc) return rc;
    if (prof && prof_flags != flags) {
        rtx::set_error("rtx_raxtax: the open taxon profile has flags %#x, the call %#x (skip_exact_matches / raw_confidence must match)", prof_flags, flags);
        return RTX_ERR_INVALID;
    }
    Front front;  // the stage objects live as long as the call
    rc = front.open(indices, n_dev, call.quals != nullptr, prof);
    if (rc) return rc;
    for (uint32_t d = 0; d < n_dev; d++) {
        dev_lookup[d] = rtx_index_has_exact_lookup(indices[d]) != 0;
        any_host_lookup = any_host_lookup || !dev_lookup[d];
        // RTX_OPT_DEVICE_TEXT: the messages come from the device (rtx_text.hip), set up for this tree and these flags
        // (not under RTX_OPT_DEREP: a device line carries one label, a distinct read has as many as it has copies)
        dev_text[d] = rtx::index_device_text(indices[d]) && !both && !front.derep;
        if (dev_text[d]) {
            rc = rtx_index_text_setup(indices[d], tree, flags | (tsv ? RTX_TEXT_TSV : 0u));
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
        Chunk &ch = chunks[c];
        ch.q0 = c * chunk_size;
        ch.nq = std::min<uint64_t>(chunk_size, n_queries - ch.q0);
        FrontChunk &fc = ch.front;
        fc.given = Reads{call.bases, call.quals, call.base_off + ch.q0, ch.nq};
        fc.in = fc.src = fc.dev = fc.given;
    }
    // the front's counters, and the busy seconds of the stages (rtx_raxtax_last_timing: which stage bounds an end-to-end run)
    FrontTotals totals{};   // (filled by the lookup thread)
    double busy_lookup = 0, busy_send = 0;
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
    std::vector<Arena> arena_pool;  // message arenas between the sender (done with a chunk) and the format threads (next chunk)
    BufPool bases_pool;             // ... and the arrays of cut reads between the sender and the lookup thread

    std::thread lookup([&] {
        for (uint64_t c = 0; c < n_chunks; c++) {
            Chunk &ch = chunks[c];
            const uint32_t d = (uint32_t)(c % n_dev);
            // no front stage, and Tree.sequences.get runs on the device, inside rtx_classify_batch: nothing to do, and nothing to wait for
            if (!front.any() && dev_lookup[d]) { set_stage(c, 1); continue; }
            if (c >= ahead && !wait_stage(c - ahead, 2)) return;
            const int rc = front.run(d, ch.front, bases_pool, nt_lookup, totals);
            if (rc) { fail(rc, rtx_last_error()); return; }
            if (dev_lookup[d]) { set_stage(c, 1); continue; }
            const double t_l0 = now();
            const Reads &dev = ch.front.dev;
            std::vector<const uint32_t *> ptr(dev.n);
            std::vector<uint32_t> cnt(dev.n);
            parallel_ranges(dev.n, nt_lookup, [&](uint64_t a, uint64_t b) {
                for (uint64_t i = a; i < b; i++) {
                    const uint32_t *ids = nullptr;
                    cnt[i] = (uint32_t)rtx_tree_exact_matches(tree, dev.bases + dev.off[i], dev.len(i), &ids);
                    ptr[i] = ids;
                }
            });
            Chunk::Copies &cp = ch.copies;
            cp.exact_off.assign(dev.n + 1, 0);
            for (uint64_t i = 0; i < dev.n; i++) cp.exact_off[i + 1] = cp.exact_off[i] + cnt[i];
            cp.exact_ids.resize(cp.exact_off[dev.n]);
            for (uint64_t i = 0; i < dev.n; i++) std::copy(ptr[i], ptr[i] + cnt[i], cp.exact_ids.begin() + cp.exact_off[i]);
            busy_lookup += now() - t_l0;
            set_stage(c, 1);
        }
    });

    // The device stage of a handle: activate -> run -> STAGE THE NEXT CHUNK -> download.  The queries of chunk c + n_dev are packed (two
    // bases per byte, pinned memory) and cross PCIe on the handle's transfer stream while the kernels of chunk c run
    // (rtx_batch_prefetch / rtx_batch_activate): the reference's workers pick up their next chunk without a pause either (raxtax.rs:35-36).
    // upload: the chunk on its own, at once (rtx_batch_upload), for a chunk whose run-ahead was abandoned
    auto stage_chunk = [&](uint32_t d, uint64_t c, bool upload) -> int {
        Chunk &ch = chunks[c];
        const FrontChunk &fc = ch.front;
        if (dev_text[d]) {  // the labels travel with the chunk (the same input set)
            const int rc = rtx_batch_prefetch_labels(indices[d], ch.nq, labels + ch.q0);
            if (rc) return rc;
        }
        if (prof && !fc.size.empty()) {  // a distinct read counts with its copies in the open profile (the same input set as well)
            const int rc = rtx_batch_prefetch_weights(indices[d], fc.dev.n, fc.size.data());
            if (rc) return rc;
        }
        if (front.prof_samples && front.demux) {  // the sample of every read for the per-sample counters (no dereplication beside them: dev.n == nq)
            const int rc = rtx_batch_prefetch_samples(indices[d], ch.nq, fc.dx_sample.data());
            if (rc) return rc;
        }
        const bool host_ids = !dev_lookup[d];
        return (upload ? rtx_batch_upload : rtx_batch_prefetch)(indices[d], fc.dev.n, fc.dev.bases, fc.dev.off, host_ids && !ch.copies.exact_ids.empty() ? ch.copies.exact_ids.data() : nullptr,
                                                                host_ids ? ch.copies.exact_off.data() : nullptr);
    };
    auto device_loop = [&](uint32_t d) {
        bool running = false;  // the kernels of chunk c have been enqueued already (behind the download of the chunk before it)
        for (uint64_t c = d; c < n_chunks; c += n_dev) {
            if (!wait_stage(c, 1)) return;
            // the result set of this handle's second-last chunk is reused now (device text: the sender reads the text of that set itself)
            if (c >= ahead && !wait_stage(c - ahead, dev_text[d] ? 4 : 3)) return;
            Chunk &ch = chunks[c];
            Chunk::Copies &cp = ch.copies;
            const std::vector<uint32_t> &slot = ch.front.slot;
            const double t_d0 = now();
            int rc = RTX_OK;
            if (!running) {  // the handle's first chunk
                rc = stage_chunk(d, c, false);
                if (!rc) rc = rtx_batch_activate(indices[d]);
                if (!rc) rc = rtx_batch_run(indices[d], flags);
            }
            running = false;
            const uint64_t nxt = c + n_dev;
            bool staged = false;
            if (!rc && nxt < n_chunks) {
                if (!wait_stage(nxt, 1)) return;   // its exact-match ids (host lookup), ready long ago as a rule
                rc = stage_chunk(d, nxt, false);
                staged = !rc;
            }
            // the device goes on with the next chunk as soon as the last records of this one have left it: the host's finalisation of
            // the last sub-batch (and this thread's bookkeeping) no longer stand between two chunks (rtx_batch_download_then_run)
            if (!rc) rc = staged ? rtx_batch_download_then_run(indices[d], &ch.res, flags) : rtx_batch_download(indices[d], &ch.res);
            if (rc == RTX_RETRY_CHUNK) {  // the run-ahead was abandoned (this chunk outgrew a buffer with the next one enqueued already): this chunk on its own
                rc = stage_chunk(d, c, true);
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
                    cp.exact_off.assign(xo, xo + ch.front.dev.n + 1);
                    cp.exact_ids.assign(xi, xi + xo[ch.front.dev.n]);
                }
            }
            if (!rc && want_strands) {
                const uint8_t *st = nullptr;
                const uint32_t *pk = nullptr;
                rc = rtx_batch_strands(indices[d], &st, &pk);
                if (!rc) { per_query(cp.strand, st, slot, ch.nq); per_query(cp.peak, pk, slot, ch.nq); }
            }
            if (!rc && near && call.align) {
                const uint32_t *nr = nullptr, *ti = nullptr;
                rc = rtx_batch_nearest(indices[d], &nr, &ti);
                if (!rc) { per_query(cp.nearest, nr, slot, ch.nq); per_query(cp.ties, ti, slot, ch.nq); }
            }
            if (!rc && ident && call.align) {  // (a copy has its representative's bases, and so its distance)
                const uint32_t *di = nullptr;
                rc = rtx_batch_identity(indices[d], &di, nullptr);
                if (!rc) per_query(cp.dist, di, slot, ch.nq);
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
            Chunk::Copies &cp = ch.copies;
            Chunk::Messages &msg = ch.msg;
            const Reads &src = ch.front.src;  // (the read as it was classified: trimmed, with primers set)
            const double t_f0 = now();
            cp.differ.assign(ch.nq, 0);
            per_query(cp.status, ch.res.status, ch.front.slot, ch.nq);
            per_query(cp.t, ch.res.t, ch.front.slot, ch.nq);
            msg.msg_off.assign(ch.nq, 0);
            msg.msg_arena.assign(ch.nq, 0);
            if (tsv) msg.tsv_off.assign(ch.nq, 0);
            const unsigned nt_f = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt_format, (ch.nq + 255) / 256));
            msg.out_arena.clear();
            msg.tsv_arena.clear();
            {   // arenas the sender is done with come back through the pool: a fresh megabyte per thread and chunk was a page fault per 4 KB of text
                std::lock_guard<std::mutex> g(pool_mu);
                for (unsigned r = 0; r < nt_f * (tsv ? 2u : 1u); r++) {
                    std::vector<Arena> &dst = r < nt_f ? msg.out_arena : msg.tsv_arena;
                    if (!arena_pool.empty()) { dst.push_back(std::move(arena_pool.back())); arena_pool.pop_back(); }
                    else dst.emplace_back();
                    dst.back().len = 0;
                }
            }
            std::atomic<int> rc_fmt{0};
            auto format_range = [&](unsigned r) {
                const uint64_t a = ch.nq * r / nt_f, b = ch.nq * (r + 1) / nt_f;
                // (worked on as locals and handed back: the arenas of neighbouring threads share cache lines in the vector, and `len` moves per query)
                Arena oa = std::move(msg.out_arena[r]), tsv_local;
                if (tsv) tsv_local = std::move(msg.tsv_arena[r]);
                Arena *ta = tsv ? &tsv_local : nullptr;
                struct Back {
                    Chunk::Messages &m; unsigned r; Arena &o, *t;
                    ~Back() { m.out_arena[r] = std::move(o); if (t) m.tsv_arena[r] = std::move(*t); }
                } back{msg, r, oa, ta};
                std::vector<uint8_t> rc_seq;  // a minus-strand query prints the orientation that was classified (the `.tsv` sequence column)
                // The rows of a view lie in the PROCESSING order of the batch and the queries are formatted in input order: every row array
                // (confidences: 256 bytes per row, lineage, depth, local signal) and the lineage string are cache misses per query -- what
                // the stage waited for (0.6 us per query on sixteen threads where the arithmetic needs 0.2).  Three prefetch stages ahead of
                // the formatting: the row arrays of query i + 24, the string object of i + 16 (its index has arrived), the characters of i + 8.
                // (j, i: queries of the caller; the view is read at their representative's position at(.), RTX_OPT_DEREP)
                const uint32_t *const slot = ch.front.slot.empty() ? nullptr : ch.front.slot.data();
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
                    const uint64_t ne = cp.exact_off[s + 1] - cp.exact_off[s];
                    if (!call.skip_exact_matches && ne > 1) {  // raxtax.rs:43-53 (the info! lines go to the log in the CLI)
                        const uint32_t *ids = cp.exact_ids.data() + cp.exact_off[s];
                        auto parent = [&](uint32_t id) {
                            const std::string &l = tree->lineages[id];
                            const size_t k = l.rfind(',');
                            return k == std::string::npos ? std::string_view() : std::string_view(l).substr(0, k);
                        };
                        for (uint64_t j = 1; j < ne; j++)
                            if (parent(ids[j]) != parent(ids[0])) { cp.differ[i] = 1; break; }
                    }
                    if (dev_text[d] || ch.res.status[s] != RTX_Q_OK) continue;  // (device text: the lines are formatted already)
                    const uint64_t len = src.len(i);
                    const uint64_t rows = ch.res.row_count[s];
                    const size_t need = (rows + 1) * (strlen(labels[q]) + 4096 + 8 * RTX_MAX_DEPTH) + len + 64;
                    char *ob = oa.room(need);
                    char *tb = ta ? ta->room(need + rows * len) : nullptr;
                    if (!ob || (ta && !tb)) { rc_fmt = RTX_ERR_OOM; return; }
                    int64_t tsv_len = 0;
                    const uint8_t *seq = src.bases + src.off[i];
                    if (tb && both && cp.strand[i]) {
                        rc_seq.resize(len + 1);
                        (void)rtx_revcomp(seq, len, rc_seq.data());
                        seq = rc_seq.data();
                    }
                    const int64_t n = rtx_format_query(tree, &ch.res, s, labels[q], seq, len,
                                                       cp.exact_ids.data() + cp.exact_off[s], ne, flags, ob, need,
                                                       tb, tb ? need + rows * len : 0, &tsv_len);
                    if (n < 0) { rc_fmt = (int)n; return; }
                    msg.msg_arena[i] = r;
                    msg.msg_off[i] = oa.len;
                    oa.len += (size_t)n + 1;  // (rtx_format_query terminates its text)
                    if (ta) { msg.tsv_off[i] = ta->len; ta->len += (size_t)tsv_len + 1; }
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
        const FrontChunk &fc = ch.front;
        const Chunk::Copies &cp = ch.copies;
        const double t_s0 = now();
        bool closed = false;
        for (uint64_t i = 0; i < ch.nq && !closed; i++) {
            const uint64_t q = ch.q0 + i;
            if (cp.differ[i]) {
                fprintf(stderr, "[WARN ] Exact matches for %s differ above the leafs of the lineage tree!\n", labels[q]);
                warnings = true;
            }
            if (call.demux) {  // every query, also one without a message (a read that is not assigned)
                const uint32_t raw = fc.given.len32(i);
                const bool on = !fc.dx_info.empty();
                if (call.demux(call.demux_ctx, labels[q], raw, on ? fc.dx_sample[i] : RTX_DEMUX_NONE, on ? fc.dx_lo[i] : 0u, on ? fc.dx_hi[i] : raw,
                            on ? fc.dx_hit[i] : (RTX_DEMUX_NO_TAG | RTX_DEMUX_NO_TAG << 16), on ? fc.dx_info[i] : 0u)) { closed = true; break; }
            }
            if (call.trim) {  // every query, also one without a message (an emptied read)
                const uint32_t raw = fc.in.len32(i);
                const bool on = !fc.lo.empty();
                if (call.trim(call.trim_ctx, labels[q], raw, on ? fc.lo[i] : 0u, on ? fc.hi[i] : raw, on ? fc.hit[i] : (RTX_TRIM_NO_PATTERN | RTX_TRIM_NO_PATTERN << 16))) { closed = true; break; }
            }
            if (call.qual) {  // likewise
                const uint32_t raw = fc.in.len32(i);
                const bool ranged = !fc.lo.empty(), on = !fc.q_hi.empty();
                if (call.qual(call.qual_ctx, labels[q], raw, ranged ? fc.lo[i] : 0u, on ? fc.q_hi[i] : (ranged ? fc.hi[i] : raw), on ? fc.q_ee[i] : 0ull, on ? fc.q_verdict[i] : 0u)) { closed = true; break; }
            }
            if (call.screen) {  // likewise
                const bool on = !fc.s_verdict.empty();
                if (call.screen(call.screen_ctx, labels[q], on ? fc.s_windows[i] : 0u, on ? fc.s_hits[i] : 0u, on ? fc.s_first[i] : RTX_SCREEN_NONE, on ? fc.s_source[i] : RTX_SCREEN_NONE,
                                on ? fc.s_verdict[i] : 0u)) { closed = true; break; }
            }
            if (call.chimera) {  // likewise; a copy takes its representative's record
                static const rtx_chimera_rec none{RTX_CHIM_OK, 0u, 0u, RTX_NO_REF, 0u, 0u, 0u, RTX_NO_REF, 0u, RTX_NO_REF, 0u, 0u};
                if (call.chimera(call.chimera_ctx, labels[q], fc.chim.empty() ? &none : &fc.chim[fc.at(i)])) { closed = true; break; }
            }
            if (cp.status[i] != RTX_Q_OK) {
                // the reference aborts here (prob.rs:21/162); report and skip the query instead
                if (cp.status[i] == RTX_Q_ALL_KMERS) fprintf(stderr, "[ERROR] query %s holds every 8-mer (t = 65536): the reference asserts t < 65536 (raxtax.rs:56)\n", labels[q]);
                else fprintf(stderr, "[ERROR] query %s has too few valid 8-mers (%u) to be classified\n", labels[q], cp.t[i]);
                continue;
            }
            if (call.align && call.align(call.align_ctx, labels[q], cp.strand[i], cp.peak[i], cp.t[i], near ? cp.nearest[i] : RTX_NO_REF, near ? cp.ties[i] : 0u,
                                   ident ? cp.dist[i] : RTX_NO_DIST, fc.src.len32(i))) { closed = true; break; }
            int sent;
            if (dev_text[c % n_dev]) {
                sent = call.sender(call.sender_ctx, labels[q], ch.text.out + ch.text.out_off[i], tsv ? ch.text.tsv + ch.text.tsv_off[i] : nullptr);
            } else {
                const uint32_t r = ch.msg.msg_arena[i];
                sent = call.sender(call.sender_ctx, labels[q], ch.msg.out_arena[r].p + ch.msg.msg_off[i], tsv ? ch.msg.tsv_arena[r].p + ch.msg.tsv_off[i] : nullptr);
            }
            if (sent != 0) closed = true;
        }
        if (closed) { fail(RTX_ERR_SENDER, "result sink closed"); break; }  // sender.send(..)?, raxtax.rs:87
        // the chunk is sent: its buffers and arenas go back to their pools, everything else is freed
        ch.front.release(bases_pool);
        ch.copies = {};
        {
            std::lock_guard<std::mutex> g(pool_mu);
            for (auto &ar : ch.msg.out_arena) arena_pool.push_back(std::move(ar));
            for (auto &ar : ch.msg.tsv_arena) arena_pool.push_back(std::move(ar));
        }
        ch.msg = {};
        busy_send += now() - t_s0;
        set_stage(c, 4);
    }
    lookup.join();
    for (auto &t : workers) t.join();
    {
        double bd = 0, bf = 0;
        for (uint32_t d = 0; d < n_dev; d++) { bd = std::max(bd, busy_device[d]); bf = std::max(bf, busy_format[d]); }
        const double busy[4] = {any_host_lookup ? busy_lookup : 0.0, bd, bf, busy_send};
        std::copy(busy, busy + 4, totals.busy);
        totals.n_chunks = n_chunks;
        std::lock_guard<std::mutex> g(g_timing_mu);
        g_last = totals;
    }
    if (failed != RTX_OK) { rtx::set_error("%s", failed_msg.c_str()); return failed; }
    if (warnings)  // raxtax.rs:93-95
        fprintf(stderr, "\x1b[33m[WARN ]\x1b[0m Exact matches for some queries differ above the species level! Check the log file for more information!\n");
    return RTX_OK;
}

// A narrower callback of an earlier entry point (rtx_query_info_fn, rtx_query_hit_fn) with its context, called in the align shape
template <class Fn>
struct Narrow { Fn fn; void *ctx; };
int info_as_align(void *p, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t, uint32_t, uint32_t, uint32_t) {
    const auto *n = static_cast<const Narrow<rtx_query_info_fn> *>(p);
    return n->fn(n->ctx, label, strand, peak, t);
}
int hit_as_align(void *p, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t, uint32_t) {
    const auto *n = static_cast<const Narrow<rtx_query_hit_fn> *>(p);
    return n->fn(n->ctx, label, strand, peak, t, nearest, ties);
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
    const rtx_sender_fn owned = [](void *ctx, const char *label, const char *out, const char *t) -> int {
        return (*static_cast<const Sender *>(ctx))(std::string(label), std::string(out), t ? std::optional<std::string>(std::string(t)) : std::nullopt) ? 0 : 1;
    };
    Call c{};
    c.indices = &index; c.n_dev = 1; c.tree = tree; c.n_queries = queries.size(); c.labels = labels.data(); c.bases = bases.data(); c.base_off = off.data();
    c.skip_exact_matches = skip_exact_matches; c.raw_confidence = raw_confidence; c.chunk_size = chunk_size;
    c.sender = owned; c.sender_ctx = const_cast<Sender *>(&sender); c.tsv = tsv;
    return run(c);
}

}  // namespace raxtax

// The same over several device handles (one per GPU, or several on one): the reference's parallel driver is one call inside the
// process as well (par_chunks over a rayon pool, raxtax.rs:35-36, main.rs:40-57).  Chunks of `chunk_size` queries are dealt to the
// handles in turn, one driving thread per handle; the messages reach the sender in input order.
// rtx_raxtax_multi_ex8 takes everything a call can bring; every entry point before it is the next one with nulls appended.
extern "C" int rtx_raxtax_multi_ex8(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx, rtx_query_demux_fn demux,
                                    void *demux_ctx, rtx_query_screen_fn screen, void *screen_ctx) {
    return run(Call{indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches != 0, raw_confidence != 0, chunk_size, sender, sender_ctx, tsv != 0,
                    quals, align, align_ctx, trim, trim_ctx, qual, qual_ctx, chimera, chimera_ctx, demux, demux_ctx, screen, screen_ctx});
}

// ... without the contaminant screen's callback (rtx_index_set_screen)
extern "C" int rtx_raxtax_multi_ex7(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx, rtx_query_demux_fn demux,
                                    void *demux_ctx) {
    return rtx_raxtax_multi_ex8(indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender, sender_ctx, tsv,
                                align, align_ctx, trim, trim_ctx, quals, qual, qual_ctx, chimera, chimera_ctx, demux, demux_ctx, nullptr, nullptr);
}

#define RTX_COMMON_ARGS indices, n_indices, tree, n_queries, labels, bases, base_off, skip_exact_matches, raw_confidence, chunk_size, sender, sender_ctx, tsv

extern "C" int rtx_raxtax(rtx_index *index, const rtx_tree *tree, uint64_t n_queries, const char *const *labels,
                          const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches, int raw_confidence,
                          uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv) {
    if (!sender) { rtx::set_error("rtx_raxtax: null sender"); return RTX_ERR_INVALID; }
    rtx_index *const *indices = &index;
    const uint32_t n_indices = 1;
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int rtx_raxtax_multi(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv) {
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ... with `info` called directly before the sender for every query that has a message: its label, strand, peak and t
extern "C" int rtx_raxtax_multi_ex(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                   const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                   int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                   rtx_query_info_fn info, void *info_ctx) {
    Narrow<rtx_query_info_fn> n{info, info_ctx};
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, info ? info_as_align : nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ... with the nearest reference and its ties as well (RTX_OPT_NEAREST)
extern "C" int rtx_raxtax_multi_ex2(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_hit_fn hit, void *hit_ctx) {
    Narrow<rtx_query_hit_fn> n{hit, hit_ctx};
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, hit ? hit_as_align : nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ... and the alignment identity (RTX_OPT_IDENTITY)
extern "C" int rtx_raxtax_multi_ex3(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx) {
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, align, align_ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ... and the primer trimming of every query (rtx_index_set_primers)
extern "C" int rtx_raxtax_multi_ex4(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx) {
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, align, align_ctx, trim, trim_ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// ... and the quality strings of the reads with the quality filter of every query (rtx_index_set_quality)
extern "C" int rtx_raxtax_multi_ex5(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx) {
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, align, align_ctx, trim, trim_ctx, quals, qual, qual_ctx, nullptr, nullptr, nullptr, nullptr);
}

// ... and the chimera record of every query (rtx_index_set_chimera); rtx_raxtax_multi_ex7 adds the sample of every query (rtx_index_set_tags)
extern "C" int rtx_raxtax_multi_ex6(rtx_index *const *indices, uint32_t n_indices, const rtx_tree *tree, uint64_t n_queries,
                                    const char *const *labels, const uint8_t *bases, const uint64_t *base_off, int skip_exact_matches,
                                    int raw_confidence, uint64_t chunk_size, rtx_sender_fn sender, void *sender_ctx, int tsv,
                                    rtx_query_align_fn align, void *align_ctx, rtx_query_trim_fn trim, void *trim_ctx, const uint8_t *quals,
                                    rtx_query_qual_fn qual, void *qual_ctx, rtx_query_chimera_fn chimera, void *chimera_ctx) {
    return rtx_raxtax_multi_ex7(RTX_COMMON_ARGS, align, align_ctx, trim, trim_ctx, quals, qual, qual_ctx, chimera, chimera_ctx, nullptr, nullptr);
}

#undef RTX_COMMON_ARGS

extern "C" int rtx_raxtax_last_demux(uint64_t *queries, uint64_t *assigned, uint64_t reasons[5], double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.demux.queries;
    if (assigned) *assigned = g_last.demux.assigned;
    if (reasons) for (int v = 0; v < 5; v++) reasons[v] = g_last.demux.reasons[v];
    if (busy_seconds) *busy_seconds = g_last.demux.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_timing(double busy[4], uint64_t *n_chunks) {
    if (!busy) { rtx::set_error("rtx_raxtax_last_timing: null argument"); return RTX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(g_timing_mu);
    for (int i = 0; i < 4; i++) busy[i] = g_last.busy[i];
    if (n_chunks) *n_chunks = g_last.n_chunks;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_derep(uint64_t *queries, uint64_t *distinct, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.derep.queries;
    if (distinct) *distinct = g_last.derep.distinct;
    if (busy_seconds) *busy_seconds = g_last.derep.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_trim(uint64_t *queries, uint64_t *with5, uint64_t *with3, uint64_t *emptied, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.trim.queries;
    if (with5) *with5 = g_last.trim.with5;
    if (with3) *with3 = g_last.trim.with3;
    if (emptied) *emptied = g_last.trim.emptied;
    if (busy_seconds) *busy_seconds = g_last.trim.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_qual(uint64_t *queries, uint64_t *passed, uint64_t *truncated, uint64_t reasons[7], double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.qual.queries;
    if (passed) *passed = g_last.qual.passed;
    if (truncated) *truncated = g_last.qual.truncated;
    if (reasons) for (int b = 0; b < 7; b++) reasons[b] = g_last.qual.reasons[b];
    if (busy_seconds) *busy_seconds = g_last.qual.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_screen(uint64_t *queries, uint64_t *screened, uint64_t *contaminants, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.screen.queries;
    if (screened) *screened = g_last.screen.screened;
    if (contaminants) *contaminants = g_last.screen.contaminants;
    if (busy_seconds) *busy_seconds = g_last.screen.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_chimera(uint64_t *queries, uint64_t *checked, uint64_t *flagged, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.chim.queries;
    if (checked) *checked = g_last.chim.checked;
    if (flagged) *flagged = g_last.chim.flagged;
    if (busy_seconds) *busy_seconds = g_last.chim.busy;
    return RTX_OK;
}

extern "C" int rtx_raxtax_last_tally(uint64_t *queries, uint64_t *counted, uint64_t *entries_added, double *busy_seconds) {
    std::lock_guard<std::mutex> g(g_timing_mu);
    if (queries) *queries = g_last.tally.queries;
    if (counted) *counted = g_last.tally.counted;
    if (entries_added) *entries_added = g_last.tally.added;
    if (busy_seconds) *busy_seconds = g_last.tally.busy;
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

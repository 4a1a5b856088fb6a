// raxtax-hip: command line around the host mirror of raxtax() -- FASTA/.bin database + FASTA queries in,
// the reference's output files out, on one GPU or, with --gpus N / --devices a,b,..., on several at once (one process, one
// index handle and one driving thread per device: rtx_raxtax_multi; the reference's `-t` of rayon threads, main.rs:40-57).  Flag names and file semantics follow the reference
// (src/io.rs:112-154 Args, :202-263 get_output, :47-90 Checkpoint, :156-187 check_incomplete_output;
// src/main.rs:72-99 database caching, :126-136 writer):
//   PREFIX/raxtax.out   one line per result row            PREFIX/raxtax.tsv  (--tsv)
//   PREFIX/raxtax.ckp   one finished query label per line  PREFIX/raxtax.json checkpoint (flags + DB fingerprint)
//   PREFIX/<db>.bin     bincode database cache (unless --skip-db)
//   PREFIX/raxtax.strand  (--strand both) label, + or -, peak, t per query, in the order of raxtax.out
//   PREFIX/raxtax.profile (--profile CUTOFF) the taxon profile of the whole run: reads under and at every taxon whose confidence reaches CUTOFF (rtx_profile_format)
//   PREFIX/raxtax.hits    (--hits) label, + or -, peak, t, ties, id and lineage of the nearest reference per query, in the order of raxtax.out
//   (--identity, implies --hits: two more columns at the end of every line of raxtax.hits -- the semi-global edit distance of the query to that
//    reference and the identity in percent, two decimals; '-' twice where there is no distance: RTX_OPT_IDENTITY)
//   PREFIX/raxtax.uniques (--uniques [--uniques-minsize N] [--uniques-max-entries N] [--uniques-max-bytes N]) the distinct reads of the whole run with their
//    abundances, `>uniq{rank};size={N}` and the sequence, largest first (rtx_tally.hip: one object per handle, accumulated on the device over the blocks of
//    the file; read, summed and written once at the end; rtx_tally_format_fasta).  The reads counted are those that go on to be classified, as given (also
//    under --strand both).  With --tags also PREFIX/raxtax.uniques.tsv, the sequence x sample table of read counts (rtx_tally_format_table).  Entries
//    below N (default 1) are left out of both files, the ranks stay.  Sequences beyond the caps are not stored; their reads are named in the log.
//   PREFIX/raxtax.otus    (--uniques --otus [--otus-minsize N]) the distinct reads of the run collapsed into OTUs by Swarm's d = 1 rule on the first device
//    (rtx_otu.hip: after the tables of the handles are summed; the whole table is clustered, --uniques-minsize only filters what is printed of the
//    uniques): `>otu{k};size={N};seed=uniq{rank}` and the seed's sequence (rtx_otu_format_fasta); PREFIX/raxtax.otus.map, `uniq{rank}\totu{k}` per
//    distinct read; with --tags also PREFIX/raxtax.otus.tsv, the OTU x sample table of read counts.  OTUs below N (default 1) are left out of
//    raxtax.otus and raxtax.otus.tsv, the numbers stay.
//   PREFIX/raxtax.otus.grafts (--uniques --otus --fastidious [--fastidious-boundary N]) Swarm's fastidious pass on the first device (rtx_graft.hip), right after the
//    clustering: an OTU below N reads (default 3) is grafted onto an OTU of at least N that holds a distinct read at most two differences away.  One line per
//    graft (rtx_otu_format_grafts); raxtax.otus, .map and .tsv are then those of the grafted OTUs, and --denovo checks those.
//   PREFIX/raxtax.otus.unoise (--uniques --otus --unoise [--unoise-minsize N] [--unoise-alpha A] [--unoise-maxdiffs D]) the distinct reads denoised into ZOTUs
//    by the UNOISE rule on the first device (rtx_unoise.hip) INSTEAD of the clustering: a read is an error of a more abundant read d differences away when
//    it is at most 1 / 2^(A d + 1) as abundant (A default 2, d at most D, default 16); what is left and holds at least N reads (default 8) is a ZOTU.  A header
//    line and one line per distinct read (rtx_otu_format_unoise); raxtax.otus, .map, .tsv, --denovo and --otus-tax are then those of the ZOTUs, written
//    under the larger of --otus-minsize and --unoise-minsize.  Not with --fastidious.
//   PREFIX/raxtax.otus.denovo (--uniques --otus --denovo [--denovo-abskew N] [--denovo-mindelta N] [--denovo-segments S]) the de novo chimera check of the
//    OTUs on the first device (rtx_denovo.hip), right after the clustering: is an OTU's seed the head of one more abundant OTU of the run joined to the tail
//    of another?  A header line and one line per OTU (rtx_denovo_format_records); PREFIX/raxtax.otus.clean, the lines of raxtax.otus of the OTUs that
//    are not flagged (under --otus-minsize); with --tags also PREFIX/raxtax.otus.clean.tsv.  raxtax.otus, .map and .tsv are what they are without it.
//   PREFIX/raxtax.otus.tax (--uniques --otus --otus-tax CUTOFF [--otus-tax-agree P]) the consensus taxonomy of the OTUs (rtx_otutax.hip): after the clustering, and after
//    the grafting under --fastidious, every distinct read of the table is classified once more through the first handle -- in chunks, in table order, with
//    the run's --skip-exact-matches / --raw-confidence / --strand and no front stage: the rows went through the front already -- its best lineage cut where the
//    confidence falls below CUTOFF (rtx_result_best_lineages, as --profile cuts it), and an OTU takes the deepest taxon that P percent (51 .. 100, default 51)
//    of its reads reach.  A header line and one line per OTU under --otus-minsize (rtx_otu_taxonomy_format), the numbers those of raxtax.otus.  The second
//    pass costs one classification per distinct read.
//   (--derep: each distinct read of a chunk is classified once, RTX_OPT_DEREP; the files are byte for byte the same, "N queries, U distinct" goes to the log)
//   PREFIX/raxtax.demux (--tags SHEET) and PREFIX/raxtax.samples (with --profile as well): below
//   (--tags SHEET [--tag-mismatches N] [--tag-offset N] [--tags-both-orientations]: every read is assigned to a sample by the inline tags at
//    its ends and loses them, on the device, before anything else sees it (rtx_index_set_tags, rtx_demux.hip).  SHEET: tab-separated lines
//    sample, fwd_tag, rev_tag in IUPAC letters, '#' starts a comment; rev_tag as on the oligo (the read ends with its reverse complement),
//    empty or '-': single-ended; a sample may own several lines.  N substitutions per tag (default 0), up to N bases in front of a tag
//    (default 0); --tags-both-orientations also registers every line flipped (rev_tag at 5', the reverse complement of fwd_tag at 3').
//    PREFIX/raxtax.demux: a header, then label, sample or '*', verdict, tag5, mm5, off5, tag3, mm3, off3, lo, hi per query in input order
//    -- the tags by their place in the list the run logs, '-' where an end has none.  A read without a sample has no result lines.  With
//    --profile the taxon x sample table of read counts goes to PREFIX/raxtax.samples (rtx_sample_table_format); not together with --derep.)
//   (--primers FWD:REV [--primer-errors PCT] [--primer-window N]: the PCR primers are trimmed off every read on the device before anything else
//    sees it (rtx_index_set_primers, rtx_trim.hip).  The oligos as ordered, 5'->3', IUPAC codes allowed, either side may be empty, the option
//    may be given twice: FWD is looked for at the 5' end and the reverse complement of REV at the 3' end -- under --strand both REV at the
//    5' end and the reverse complement of FWD at the 3' end as well -- with at most len * PCT / 100 errors (default 10) in the first / last
//    N bases (default: len + errors + 32).  PREFIX/raxtax.trim: a header, then label, length, start, end, primer5, errors5, primer3, errors3
//    per query in input order -- the read kept [start, end) of its length bases, the primers by their place in the list above, '-' where
//    none was found; "N queries, A with a 5' primer, B with a 3' primer, C left empty" goes to the log)
//   (-i takes FASTQ as well -- the first non-blank byte of the file decides: '@' FASTQ, '>' FASTA; four-line records, --fastq-ascii 33|64 --
//    and then the quality filter on the device, rtx_index_set_quality / rtx_qual.hip: --trunclen N, --truncq Q, --truncee E, --minlen N,
//    --maxlen N, --maxns N, --maxee E, --maxee-rate R as `vsearch --fastq_filter` names them.  With a filter option PREFIX/raxtax.qc: a header,
//    then label, length, start, end, expected errors, verdict per query in input order -- the read kept [start, end) of its length bases with
//    that many expected errors (six decimals, truncated), verdict `pass` or the reasons it was discarded for joined by '+'; a discarded read has
//    no result lines; the totals go to the log.  A filter option on FASTA input is refused.)
//   (--reverse R2.fastq, short -r: -i holds the forward mates and this file the reverse mates of the same pairs, record for record; the two
//    mates of every pair are merged on the first device of the run before anything else sees them (rtx_merge_queries, rtx_merge.hip), block
//    by block on the reader's thread, so that merging overlaps with the classification of the block before.  --merge-minovlen N (16),
//    --merge-maxdiffs N (10), --merge-maxdiffpct N (100), --merge-qcap N (41) are the fields of rtx_merge_params.  Primers, quality filter,
//    dereplication and classification see merged reads; a pair that is not merged is the empty read: no result lines.  PREFIX/raxtax.merge: a
//    header, then label, forward length, reverse length, overlap, diffs, merged length and verdict (`merged`, or the reason it was not) per
//    pair in input order; the totals go to the log.  --reverse with FASTA input, or a merge option without --reverse, is refused.)
//   (--contaminants FILE[.gz] [--contam-minhits N] [--contam-minpct P]: every read is screened against the 16-mers of the FASTA records of FILE on
//    the device before it is classified (rtx_index_set_screen, rtx_screen.hip; behind primers and quality filter, in front of --derep): a read
//    with at least N (2) of its 16-base windows in the set, and at least P (50) percent of them, is a contaminant and has no result lines, like a
//    read the quality filter discards.  PREFIX/raxtax.screen: a header, then label, the length of the screened range, its valid windows, the
//    hits, the position of the first hit or -, the record of FILE that holds it (its label up to the first blank) or -, pass or contaminant,
//    one line per read in input order.  FASTA and FASTQ input alike.)
//   (--chimera [--chimera-mindelta N] [--chimera-segments S]: every read is checked against the references on the device before it is classified
//    (rtx_index_set_chimera, rtx_chimera.hip; behind --derep, so a distinct read is checked once): the best pair of references over a left and
//    a right part of the read against the best single reference, at S - 1 breakpoints (S = 2 .. 32, default 16); a read whose pair explains N
//    windows more (default 24) is flagged and has no result lines, like a read the quality filter discards.  PREFIX/raxtax.chimera: a header,
//    then label, status (ok, no_kmer, too_long), windows, single, parent_id, seg, pos, left, a_id, right, b_id, delta, Y|N|? (? where the read
//    was not checked) and the lineages of the three references per query in input order, '-' where there is none; the totals go to the log.
//    --chimera with --strand both is refused: a read is checked in the orientation given.)
// A rerun with the same flags and database resumes: labels listed in raxtax.ckp are skipped
// (parser.rs:150-153) and half-written result lines of unlisted queries are purged first.
// Inputs ending in .gz / .gzip are decompressed on the fly (utils.rs:42-60 get_reader: the extension decides).
// Out of scope: raxtax.log, progress bars, thread options.
//
// The file in the order of a run, main() at the end: options (Options, parse_args), what they come to before any device is touched (Plan,
// Identity, validate), the per-read reports (Report, Sink and the callbacks), the reader's thread (BlockQueue, read_single, read_paired),
// the handles, the loop over blocks with the totals of the stages (Stage), the files written at the end of a run.
#include <sys/stat.h>
#include <zlib.h>

#include <cctype>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <mutex>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "host_raxtax.hpp"
#include "raxtax_hip.h"

namespace {

using ull = unsigned long long;

// utils::get_reader (utils.rs:42-60): the file's last extension, lower-cased, "gz" or "gzip" = a GzDecoder in front of the reader
bool is_gz(const std::string &path) {
    const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return false;
    std::string ext = path.substr(dot + 1);
    for (char &c : ext) c = (char)tolower((unsigned char)c);
    return ext == "gz" || ext == "gzip";
}

// A file read in pieces, plain or gzip-compressed.
struct Input {
    FILE *f = nullptr;
    gzFile g = nullptr;
    bool open(const std::string &path) {
        if (is_gz(path)) {
            g = gzopen(path.c_str(), "rb");
            if (g) gzbuffer(g, 1 << 20);
            return g != nullptr;
        }
        f = fopen(path.c_str(), "rb");
        return f != nullptr;
    }
    // up to n bytes; fewer only at the end of the data; (size_t)-1 on a read / decompression error
    size_t read(char *buf, size_t n) {
        if (f) return fread(buf, 1, n, f);
        size_t got = 0;
        while (got < n) {
            const int k = gzread(g, buf + got, (unsigned)std::min<size_t>(n - got, 1u << 30));
            if (k < 0) return (size_t)-1;
            if (k == 0) break;
            got += (size_t)k;
        }
        if (got < n) {  // the end of the data -- or of a truncated / corrupt stream: zlib hands out what it decoded and keeps the error
            int err = Z_OK;
            (void)gzerror(g, &err);
            if (err != Z_OK && err != Z_STREAM_END) return (size_t)-1;
        }
        return got;
    }
    void close() {
        if (f) fclose(f);
        if (g) gzclose(g);
        f = nullptr;
        g = nullptr;
    }
};

// The next piece of the file behind what the buffer holds (eof: it was the last); false on a read error
bool read_on(Input &in, std::string &buf, size_t piece, bool &eof) {
    const size_t have = buf.size();
    buf.resize(have + piece);
    const size_t got = in.read(&buf[have], piece);
    if (got == (size_t)-1) return false;
    buf.resize(have + got);
    eof = got < piece;
    return true;
}

bool slurp(const std::string &path, std::string &out) {
    Input in;
    if (!in.open(path)) return false;
    out.clear();
    bool eof = false, ok = true;
    while (ok && !eof) ok = read_on(in, out, (size_t)16 << 20, eof);
    in.close();
    return ok;
}

bool is_file(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
bool is_dir(const std::string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

// FileFingerprint (io.rs:24-45): path, size, mtime in seconds
std::string fingerprint(const std::string &path) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return "";
    char *abs = realpath(path.c_str(), nullptr);
    std::ostringstream ss;
    ss << (abs ? abs : path.c_str()) << "|" << (long long)st.st_size << "|" << (long long)st.st_mtime;
    free(abs);
    return ss.str();
}

// A file written once, at the end of a run; false behind the message
bool write_whole(const std::string &path, const std::string &text) {
    std::ofstream f(path, std::ios::trunc);
    f << text;
    f.close();
    if (!f.good()) fprintf(stderr, "[ERROR] cannot write %s\n", path.c_str());
    return f.good();
}

// The two-pass protocol of the library's formatters: fn(nullptr, 0) says how long the text is, fn(buf, cap) writes it
template <class F>
int format_two_pass(std::string &text, F fn) {
    const int64_t need = fn(nullptr, 0);
    if (need < 0) return (int)need;
    text.resize((size_t)need);
    const int64_t got = fn(&text[0], text.size());
    return got == need ? RTX_OK : (got < 0 ? (int)got : RTX_ERR_STATE);
}

// --timing: seconds per stage of the run, one JSON object on stderr at the end
struct Laps {
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    std::ostringstream log;
    void lap(const char *what) {
        const auto now = std::chrono::steady_clock::now();
        log << (log.tellp() > 0 ? ", " : "") << '"' << what << "\": " << std::chrono::duration<double>(now - prev).count();
        prev = now;
    }
};

// ---- options: everything the argument loop sets

struct Options {
    std::string db, qf, prefix = "raxtax";
    bool skip_exact = false, raw = false, tsv = false, only_db = false, skip_db = false, clean = false, redo = false, timing = false;
    std::vector<int> devices{0};
    bool device_format = false;  // --device-format: RTX_OPT_DEVICE_TEXT on every handle: the lines are formatted on the GPU
    bool both_strands = false;   // --strand both: RTX_OPT_STRAND on every handle
    bool want_hits = false;      // --hits: RTX_OPT_NEAREST on every handle, PREFIX/raxtax.hits
    bool want_identity = false;  // --identity: RTX_OPT_IDENTITY on every handle, dist and identity at the end of every line of raxtax.hits (implies --hits)
    bool derep = false;          // --derep: RTX_OPT_DEREP on every handle (each distinct read of a chunk is classified once; the files are the same)
    std::vector<std::pair<std::string, std::string>> primer_pairs;  // --primers FWD:REV (once or twice): rtx_index_set_primers on every handle, PREFIX/raxtax.trim
    uint32_t primer_pct = 10, primer_window = 0;                   // --primer-errors PCT, --primer-window N
    rtx_qual_params qual{33u, 0u, -1, -1.0, 0u, 0u, -1, -1.0, -1.0};  // --fastq-ascii and the filter options: rtx_index_set_quality on every handle, PREFIX/raxtax.qc
    std::string qual_spec;                                             // the filter options as given, name=value (empty: none) -- part of the checkpoint
    std::string rev_file;                                              // --reverse FILE: the reverse mates of the pairs of -i, merged on the device (rtx_merge_queries), PREFIX/raxtax.merge
    rtx_merge_params merge{33u, 16u, 10u, 100u, 41u};                  // --merge-minovlen, --merge-maxdiffs, --merge-maxdiffpct, --merge-qcap (ascii_base: --fastq-ascii)
    std::string merge_opts;                                            // the names of the merge options given (empty: none)
    bool chim_on = false;                                              // --chimera: rtx_index_set_chimera on every handle, PREFIX/raxtax.chimera
    rtx_chimera_params chim{RTX_CHIMERA_DEFAULT_SEGMENTS, RTX_CHIMERA_DEFAULT_MINDELTA};  // --chimera-segments, --chimera-mindelta
    std::string chim_opts;                                             // those two, likewise
    std::string contam_file;                                           // --contaminants FILE: rtx_index_set_screen on every handle, PREFIX/raxtax.screen
    rtx_screen_params contam{2u, 50u};                                 // --contam-minhits N, --contam-minpct P
    std::string contam_opts;                                           // those two, likewise
    std::string tags_file;                                             // --tags SHEET: rtx_index_set_tags on every handle, PREFIX/raxtax.demux (and raxtax.samples with --profile)
    rtx_demux_params tag_params{0u, 0u};                               // --tag-mismatches N, --tag-offset N
    bool tags_both = false;                                            // --tags-both-orientations
    std::string tag_opts;                                              // those three, likewise
    bool uniques = false;         // --uniques: a tally (rtx_tally.hip) on every handle, PREFIX/raxtax.uniques (and raxtax.uniques.tsv with --tags)
    uint64_t uniques_minsize = 1, uniques_max_entries = 0, uniques_max_bytes = 0;  // --uniques-minsize N, --uniques-max-entries N, --uniques-max-bytes N (0: the library's defaults)
    std::string uniques_opts;     // those three, likewise
    bool otus = false;            // --otus: the table of --uniques clustered into OTUs (rtx_otu.hip), PREFIX/raxtax.otus, raxtax.otus.map (and raxtax.otus.tsv with --tags)
    uint64_t otus_minsize = 1;    // --otus-minsize N
    std::string otus_opts;        // that one, likewise
    bool fastidious = false;      // --fastidious: the small OTUs grafted onto large ones two differences away (rtx_graft.hip), PREFIX/raxtax.otus.grafts; the OTU files are the grafted ones
    uint64_t fastidious_boundary = 0;  // --fastidious-boundary N (0: the library's default, 3)
    std::string fastidious_opts;  // that one, likewise
    bool unoise = false;          // --unoise: the OTU object is made by the denoiser (rtx_unoise.hip) instead of the clustering, PREFIX/raxtax.otus.unoise; the OTU files are the ZOTUs
    rtx_unoise_params unoise_params{8, 2, 0, 0};  // --unoise-minsize N, --unoise-alpha A, --unoise-maxdiffs D
    std::string unoise_opts;      // those three, likewise
    bool denovo = false;          // --denovo: the OTUs checked for chimeras of more abundant OTUs (rtx_denovo.hip), PREFIX/raxtax.otus.denovo, raxtax.otus.clean (and .clean.tsv with --tags)
    rtx_denovo_params denovo_params{RTX_CHIMERA_DEFAULT_SEGMENTS, RTX_CHIMERA_DEFAULT_MINDELTA, RTX_DENOVO_DEFAULT_ABSKEW, 0, 0};  // --denovo-segments S, --denovo-mindelta N, --denovo-abskew N
    std::string denovo_opts;      // those three, likewise
    uint32_t otus_tax_cutoff = 0; // --otus-tax CUTOFF, in hundredths (0: off): the consensus taxonomy of the OTUs (rtx_otutax.hip), PREFIX/raxtax.otus.tax
    uint32_t otus_tax_agree = 51; // --otus-tax-agree P
    std::string otus_tax_opts;    // that one, likewise
    uint32_t profile_cutoff = 0;  // --profile CUTOFF, in hundredths (0: no profile): a taxon profile open on every handle, PREFIX/raxtax.profile
    size_t chunk = 0;             // --batch: queries per chunk of rtx_raxtax; 0 = chosen per block of the query file (classify_blocks)
    size_t block_bytes = (size_t)256 << 20;  // query file read and parsed in blocks of this size
};

// An option that takes one number.  kind: 'u' / 'i' a whole number, least .. most, into a uint32_t / an int32_t; 'r' a number that is not negative
// into a double; 'p' a positive integer, at most `most`, into a uint64_t.  given: the string of its group that records it
struct Numeric { const char *flag; char kind; long long least, most; void *to; std::string *given; };

// 0, or the exit code behind the message
int parse_args(int argc, char **argv, Options &o) {
    const Numeric numeric[] = {
        {"--trunclen", 'u', 1, RTX_QUAL_MAX_READ, &o.qual.trunc_len, &o.qual_spec},
        {"--minlen", 'u', 1, RTX_QUAL_MAX_READ, &o.qual.min_len, &o.qual_spec},
        {"--maxlen", 'u', 1, RTX_QUAL_MAX_READ, &o.qual.max_len, &o.qual_spec},
        {"--maxns", 'i', 0, RTX_QUAL_MAX_READ, &o.qual.max_ns, &o.qual_spec},
        {"--truncq", 'i', 0, 93, &o.qual.trunc_qual, &o.qual_spec},
        {"--truncee", 'r', 0, 0, &o.qual.trunc_ee, &o.qual_spec},
        {"--maxee", 'r', 0, 0, &o.qual.max_ee, &o.qual_spec},
        {"--maxee-rate", 'r', 0, 0, &o.qual.max_ee_rate, &o.qual_spec},
        {"--merge-minovlen", 'u', 1, RTX_MERGE_MAX_READ, &o.merge.min_overlap, &o.merge_opts},
        {"--merge-maxdiffs", 'u', 0, RTX_MERGE_MAX_READ, &o.merge.max_diffs, &o.merge_opts},
        {"--merge-maxdiffpct", 'u', 0, 100, &o.merge.max_diff_pct, &o.merge_opts},
        {"--merge-qcap", 'u', 0, 93, &o.merge.q_cap, &o.merge_opts},
        {"--chimera-mindelta", 'u', 0, RTX_CHIMERA_MAX_QUERY, &o.chim.mindelta, &o.chim_opts},
        {"--chimera-segments", 'u', 2, RTX_CHIMERA_MAX_SEGMENTS, &o.chim.segments, &o.chim_opts},
        {"--contam-minhits", 'u', 1, 0x7FFFFFFF, &o.contam.min_hits, &o.contam_opts},
        {"--contam-minpct", 'u', 0, 100, &o.contam.min_pct, &o.contam_opts},
        {"--tag-mismatches", 'u', 0, RTX_DEMUX_MAX_MISMATCHES, &o.tag_params.max_mismatches, &o.tag_opts},
        {"--tag-offset", 'u', 0, RTX_DEMUX_MAX_OFFSET, &o.tag_params.max_offset, &o.tag_opts},
        {"--uniques-minsize", 'p', 1, LLONG_MAX, &o.uniques_minsize, &o.uniques_opts},
        {"--uniques-max-entries", 'p', 1, 0x7FFFFFFE, &o.uniques_max_entries, &o.uniques_opts},
        {"--uniques-max-bytes", 'p', 1, LLONG_MAX, &o.uniques_max_bytes, &o.uniques_opts},
        {"--otus-minsize", 'p', 1, LLONG_MAX, &o.otus_minsize, &o.otus_opts},
        {"--fastidious-boundary", 'p', 1, LLONG_MAX, &o.fastidious_boundary, &o.fastidious_opts},
        {"--unoise-minsize", 'p', 1, LLONG_MAX, &o.unoise_params.minsize, &o.unoise_opts},
        {"--unoise-alpha", 'u', 1, 8, &o.unoise_params.alpha, &o.unoise_opts},
        {"--unoise-maxdiffs", 'u', 1, RTX_UNOISE_MAX_DIFFS, &o.unoise_params.max_diffs, &o.unoise_opts},
        {"--otus-tax-agree", 'u', 51, 100, &o.otus_tax_agree, &o.otus_tax_opts},
        {"--denovo-abskew", 'u', 1, 0x7FFFFFFF, &o.denovo_params.abskew, &o.denovo_opts},
        {"--denovo-mindelta", 'u', 0, RTX_CHIMERA_MAX_QUERY, &o.denovo_params.mindelta, &o.denovo_opts},
        {"--denovo-segments", 'u', 2, RTX_CHIMERA_MAX_SEGMENTS, &o.denovo_params.segments, &o.denovo_opts},
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        const Numeric *num = nullptr;
        for (const Numeric &n : numeric)
            if (a == n.flag) num = &n;
        if (num) {
            const char *v = val();
            char *end = nullptr;
            if (num->kind == 'r') {
                const double x = strtod(v, &end);
                if (end == v || *end != 0 || !(x >= 0.0)) { fprintf(stderr, "raxtax-hip: %s takes a number that is not negative, not '%s'\n", num->flag, v); return 64; }
                *static_cast<double *>(num->to) = x;
            } else {
                const long long x = strtoll(v, &end, 10);
                if (end == v || *end != 0 || x < num->least || x > num->most) {
                    if (num->kind == 'p') fprintf(stderr, "raxtax-hip: %s takes a positive integer\n", num->flag);
                    else fprintf(stderr, "raxtax-hip: %s takes a whole number, %lld .. %lld, not '%s'\n", num->flag, num->least, num->most, v);
                    return 64;
                }
                if (num->kind == 'p') *static_cast<uint64_t *>(num->to) = (uint64_t)x;
                else if (num->kind == 'i') *static_cast<int32_t *>(num->to) = (int32_t)x;
                else *static_cast<uint32_t *>(num->to) = (uint32_t)x;
            }
            std::string &given = *num->given;
            if (&given == &o.qual_spec) given += (given.empty() ? "" : ";") + a.substr(2) + "=" + v;  // (the filter's settings go into the checkpoint as given)
            else given += (given.empty() ? "" : " ") + a;
        }
        else if (a == "-d" || a == "--database-path") o.db = val();
        else if (a == "-i" || a == "--query-file") o.qf = val();
        else if (a == "-o" || a == "--prefix") o.prefix = val();
        else if (a == "--skip-exact-matches") o.skip_exact = true;
        else if (a == "--raw-confidence") o.raw = true;
        else if (a == "--tsv") o.tsv = true;
        else if (a == "--only-db") o.only_db = true;
        else if (a == "--skip-db") o.skip_db = true;
        else if (a == "-c" || a == "--clean") o.clean = true;
        else if (a == "--redo") o.redo = true;
        else if (a == "--timing") o.timing = true;
        else if (a == "--device-format") o.device_format = true;
        // CPU tuning flags of the reference (io.rs:139-153): accepted so that existing command lines keep working,
        // without effect on the device path.  -t takes a value; clap also accepts -tN, --threads=N, -vv, -qq.
        else if (a == "-t" || a == "--threads") (void)val();
        else if (a.rfind("--threads=", 0) == 0 || (a.size() > 2 && a[0] == '-' && a[1] == 't' && isdigit((unsigned char)a[2]))) {}
        else if (a == "--pin") {}
        else if (a == "--verbose" || a == "--quiet" || (a.size() >= 2 && a[0] == '-' && a[1] != '-' &&
                                                        a.find_first_not_of(a[1] == 'v' ? "v" : "q", 1) == std::string::npos &&
                                                        (a[1] == 'v' || a[1] == 'q'))) {}
        else if (a == "--device") o.devices.assign(1, atoi(val()));
        else if (a == "--gpus") {  // devices 0 .. N-1
            const int n = atoi(val());
            o.devices.clear();
            for (int d = 0; d < n; d++) o.devices.push_back(d);
        } else if (a == "--devices") {  // an explicit list; a device may be named twice (two handles on one GPU)
            o.devices.clear();
            std::stringstream ss(val());
            std::string tok;
            while (std::getline(ss, tok, ',')) if (!tok.empty()) o.devices.push_back(atoi(tok.c_str()));
        }
        else if (a == "--strand") {
            const std::string v = val();
            if (v != "plus" && v != "both") { fprintf(stderr, "raxtax-hip: --strand takes plus or both\n"); return 64; }
            o.both_strands = v == "both";
        }
        else if (a == "--hits") o.want_hits = true;
        else if (a == "--identity") o.want_identity = o.want_hits = true;
        else if (a == "--derep") o.derep = true;
        else if (a == "--primers") {
            const std::string v = val();
            const size_t colon = v.find(':');
            if (colon == std::string::npos || v.find(':', colon + 1) != std::string::npos || v.size() < 2) {
                fprintf(stderr, "raxtax-hip: --primers takes FWD:REV (either side may be empty), not '%s'\n", v.c_str());
                return 64;
            }
            o.primer_pairs.emplace_back(v.substr(0, colon), v.substr(colon + 1));
        }
        else if (a == "--primer-errors") {
            const int x = atoi(val());
            if (x < 0 || x > 99) { fprintf(stderr, "raxtax-hip: --primer-errors takes a percentage, 0 .. 99\n"); return 64; }
            o.primer_pct = (uint32_t)x;
        }
        else if (a == "--primer-window") {
            const int x = atoi(val());
            if (x < 1 || x > RTX_TRIM_MAX_WINDOW) { fprintf(stderr, "raxtax-hip: --primer-window takes 1 .. %d bases\n", RTX_TRIM_MAX_WINDOW); return 64; }
            o.primer_window = (uint32_t)x;
        }
        else if (a == "--fastq-ascii") {
            const std::string v = val();
            if (v != "33" && v != "64") { fprintf(stderr, "raxtax-hip: --fastq-ascii takes 33 or 64, not '%s'\n", v.c_str()); return 64; }
            o.qual.ascii_base = (uint32_t)atoi(v.c_str());
        }
        else if (a == "-r" || a == "--reverse") o.rev_file = val();
        else if (a == "--chimera") o.chim_on = true;
        else if (a == "--contaminants") o.contam_file = val();
        else if (a == "--tags") o.tags_file = val();
        else if (a == "--tags-both-orientations") { o.tags_both = true; o.tag_opts += (o.tag_opts.empty() ? "" : " ") + a; }
        else if (a == "--profile" || a == "--otus-tax") {
            char *end = nullptr;
            const char *v = val();
            const double x = strtod(v, &end);
            const long c = end != v && *end == '\0' && x > 0.0 && x <= 1.0 ? lround(x * 100.0) : 0;
            if (c < 1 || c > 100) { fprintf(stderr, "raxtax-hip: %s takes a confidence cutoff in (0, 1], such as 0.8\n", a.c_str()); return 64; }
            (a == "--profile" ? o.profile_cutoff : o.otus_tax_cutoff) = (uint32_t)c;
        }
        else if (a == "--uniques") o.uniques = true;
        else if (a == "--otus") o.otus = true;
        else if (a == "--fastidious") o.fastidious = true;
        else if (a == "--unoise") o.unoise = true;
        else if (a == "--denovo") o.denovo = true;
        else if (a == "--batch") o.chunk = (size_t)atoll(val());
        else if (a == "--block-bytes") o.block_bytes = std::max<size_t>(1, (size_t)atoll(val()));
        else {
            fprintf(stderr, "usage: raxtax-hip -d DB.(fasta|bin) [-i QUERIES.(fasta|fastq)] [-o PREFIX] [--skip-exact-matches] [--raw-confidence] "
                            "[--tsv] [--only-db] [--skip-db] [-c] [--redo] [--device N | --gpus N | --devices a,b,..] [--batch N] [--block-bytes N] [--device-format] [--strand plus|both] [--hits] [--identity] [--profile CUTOFF] [--derep] [--primers FWD:REV [--primer-errors PCT] [--primer-window N]] [--fastq-ascii 33|64] [--trunclen N] [--truncq Q] [--truncee E] [--minlen N] [--maxlen N] [--maxns N] [--maxee E] [--maxee-rate R] [--reverse R2.fastq [--merge-minovlen N] [--merge-maxdiffs N] [--merge-maxdiffpct N] [--merge-qcap N]] [--chimera [--chimera-mindelta N] [--chimera-segments S]] [--tags SHEET [--tag-mismatches N] [--tag-offset N] [--tags-both-orientations]] [--contaminants FILE [--contam-minhits N] [--contam-minpct P]] [--uniques [--uniques-minsize N] [--uniques-max-entries N] [--uniques-max-bytes N] [--otus [--otus-minsize N] [--fastidious [--fastidious-boundary N]] [--unoise [--unoise-minsize N] [--unoise-alpha A] [--unoise-maxdiffs D]] [--otus-tax CUTOFF [--otus-tax-agree P]] [--denovo [--denovo-abskew N] [--denovo-mindelta N] [--denovo-segments S]]]]\n"
                            "       (-t/--threads N, --pin, -v, -q of the reference are accepted and ignored)\n"
                            "       (--otus-tax classifies every distinct read of the run once more, after the clustering: one classification per distinct read on top of the run)\n");
            return 64;
        }
    }
    if (o.devices.empty()) { fprintf(stderr, "raxtax-hip: --gpus / --devices need at least one device\n"); return 64; }
    if (o.db.empty() || (o.qf.empty() && !o.only_db) || (o.only_db && o.skip_db)) {
        fprintf(stderr, "raxtax-hip: -d is required, -i unless --only-db; --only-db conflicts with --skip-db\n");
        return 64;
    }
    return 0;
}

// ---- what the options come to, before the database is read and any device is touched

// What makes up a run's identity: the text of PREFIX/raxtax.json, its entries in this order.  A rerun resumes only where the text is the same.  The
// first four are always there; an entry of an option group is filled where validate() checks the group, and is left out while it is empty.
struct Identity {
    struct Entry { const char *key; bool quoted; std::string value; };
    std::vector<Entry> entries{
        {"db_fingerprint", true, ""}, {"raw_confidence", false, ""}, {"skip_exact_matches", false, ""}, {"tsv", false, ""},
        {"strand", true, ""},         // "both": a rerun with the other setting starts over; a default run writes the file it always wrote
        {"hits", false, ""},          // ... and so is --hits,
        {"identity", false, ""},      //     --identity,
        {"profile", false, ""},       //     and the cutoff of --profile in hundredths
        {"primers", true, ""},        // --primers with its two settings, as given: trimmed reads are other reads
        {"quality", true, ""},        // the quality filter's settings, as given
        {"merge", true, ""},          // --reverse with the merge settings: merged reads are other reads
        {"chimera", true, ""},        // --chimera with its two settings: flagged reads have no lines
        {"tags", true, ""},           // --tags with its settings: demultiplexed reads are other reads
        {"contaminants", true, ""},   // --contaminants with its settings and the set's fingerprint: contaminants have no lines
        {"uniques", true, ""},        // --uniques with its settings: the table is the run's, a resumed run would miss reads
        {"otus", true, ""},           // --otus with its setting: its files are the run's
        {"fastidious", true, ""},     // --fastidious with its boundary: the OTU files are the grafted ones
        {"unoise", true, ""},         // --unoise with its three settings: the OTU files are the ZOTUs
        {"denovo", true, ""},         // --denovo with its three settings, likewise
        {"otus_tax", true, ""},       // --otus-tax with its cutoff and agreement, likewise
    };
    std::string &operator[](const std::string &key) {
        for (Entry &e : entries)
            if (key == e.key) return e.value;
        abort();
    }
    std::string json() const {
        std::string s = "{";
        for (size_t k = 0; k < entries.size(); k++) {
            const Entry &e = entries[k];
            if (k >= 4 && e.value.empty()) continue;
            s += std::string(k ? ",\n  \"" : "\n  \"") + e.key + "\": " + (e.quoted ? "\"" + e.value + "\"" : e.value);
        }
        return s + "\n}\n";
    }
};

struct Oligo { std::string name; std::vector<uint8_t> codes; uint32_t end; };  // a primer or a tag: at RTX_TRIM_5P or RTX_TRIM_3P

struct Plan {
    bool fastq = false;                                    // -i is FASTQ
    bool qual_on = false, merge_on = false, tags_on = false, screen_on = false;  // (primers: !primers.empty(); the other groups are flags of Options)
    std::vector<Oligo> primers, tags;                      // the patterns of --primers, the distinct tags of the sheet, in the order the run logs them
    std::vector<rtx_demux_pair> tag_pairs;                 // the lines of the sheet: two tags and a sample
    std::vector<std::string> sample_names, contam_names;   // the samples of the sheet; the records of --contaminants
    rtx_screen_set *contam_set = nullptr;                  // freed once the handles hold what they need
    Identity identity;
};

// parser.rs:11-34 for an oligo on the command line; 0 where the character is no IUPAC code
uint8_t iupac_code(char ch) {
    switch (toupper((unsigned char)ch)) {
        case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
        case 'W': return 9; case 'S': return 6; case 'M': return 3; case 'K': return 12; case 'R': return 5; case 'Y': return 10;
        case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
        default: return 0;
    }
}

// The codes of an oligo in IUPAC letters; false, and the letter, where one is no code
bool parse_oligo(const std::string &oligo, std::vector<uint8_t> &codes, char &bad) {
    for (char ch : oligo) {
        const uint8_t c = iupac_code(ch);
        if (!c) { bad = ch; return false; }
        codes.push_back(c);
    }
    return true;
}

std::vector<uint8_t> revcomp(const std::vector<uint8_t> &x) {
    std::vector<uint8_t> y(x.size() + 1);
    (void)rtx_revcomp(x.data(), x.size(), y.data());
    y.resize(x.size());
    return y;
}

// An option of a group (given: their names) without the option that turns the group on
bool orphan(const std::string &given, bool parent_on, const char *sentence) {
    if (given.empty() || parent_on) return false;
    fprintf(stderr, "raxtax-hip: %s %s\n", given.c_str(), sentence);
    return true;
}

// --primers: the pattern list
int primer_patterns(const Options &o, Plan &p) {
    std::string spec;
    for (const auto &pr : o.primer_pairs) {
        std::vector<uint8_t> codes[2];
        for (int side = 0; side < 2; side++) {
            const std::string &oligo = side ? pr.second : pr.first;
            char bad = 0;
            if (!parse_oligo(oligo, codes[side], bad)) { fprintf(stderr, "raxtax-hip: --primers: '%c' in primer %s is no IUPAC code\n", bad, oligo.c_str()); return 64; }
            if (oligo.size() > RTX_TRIM_MAX_PATTERN) { fprintf(stderr, "raxtax-hip: --primers: primer %s has %zu bases (at most %d)\n", oligo.c_str(), oligo.size(), RTX_TRIM_MAX_PATTERN); return 64; }
        }
        auto add = [&](const std::string &name, const std::vector<uint8_t> &c, uint32_t end) {
            if (!c.empty()) p.primers.push_back({name, c, end});
        };
        add(pr.first, codes[0], RTX_TRIM_5P);
        add("revcomp(" + pr.second + ")", revcomp(codes[1]), RTX_TRIM_3P);
        if (o.both_strands) {
            add(pr.second, codes[1], RTX_TRIM_5P);
            add("revcomp(" + pr.first + ")", revcomp(codes[0]), RTX_TRIM_3P);
        }
        if (p.primers.size() > RTX_TRIM_MAX_PATTERNS) {
            fprintf(stderr, "raxtax-hip: --primers: %s:%s makes %zu patterns (at most %d%s)\n", pr.first.c_str(), pr.second.c_str(), p.primers.size(), RTX_TRIM_MAX_PATTERNS,
                    o.both_strands ? "; --strand both registers every oligo at both ends" : "");
            return 64;
        }
        spec += (spec.empty() ? "" : ",") + pr.first + ":" + pr.second;
    }
    if (!spec.empty()) p.identity["primers"] = spec + ";errors=" + std::to_string(o.primer_pct) + ";window=" + std::to_string(o.primer_window);
    return 0;
}

// --tags: the sample sheet
int read_sample_sheet(const Options &o, Plan &p) {
    std::string sheet;
    if (!slurp(o.tags_file, sheet)) { fprintf(stderr, "raxtax-hip: --tags: cannot read %s\n", o.tags_file.c_str()); return 66; }
    auto strip = [](std::string s) {
        while (!s.empty() && isspace((unsigned char)s.back())) s.pop_back();
        size_t a = 0;
        while (a < s.size() && isspace((unsigned char)s[a])) a++;
        return s.substr(a);
    };
    auto tag_of = [&](const std::string &name, const std::vector<uint8_t> &codes, uint32_t end) -> uint32_t {  // a tag that several lines share is listed once
        for (size_t k = 0; k < p.tags.size(); k++)
            if (p.tags[k].end == end && p.tags[k].codes == codes) return (uint32_t)k;
        p.tags.push_back({name, codes, end});
        return (uint32_t)p.tags.size() - 1u;
    };
    std::istringstream lines(sheet);
    std::string line;
    for (unsigned line_no = 1; std::getline(lines, line); line_no++) {
        line = line.substr(0, line.find('#'));
        if (strip(line).empty()) continue;
        std::vector<std::string> f;
        for (size_t a = 0;;) {
            const size_t t = line.find('\t', a);
            f.push_back(strip(line.substr(a, t == std::string::npos ? std::string::npos : t - a)));
            if (t == std::string::npos) break;
            a = t + 1;
        }
        if (f.size() < 2 || f.size() > 3 || f[0].empty() || f[1].empty()) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: expected sample<TAB>fwd_tag<TAB>rev_tag\n", o.tags_file.c_str(), line_no); return 64; }
        std::vector<uint8_t> codes[2];
        const bool single = f.size() == 2 || f[2].empty() || f[2] == "-";
        char bad = 0;
        for (int side = 0; side < (single ? 1 : 2); side++)
            if (!parse_oligo(f[1 + side], codes[side], bad)) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: '%c' is no IUPAC code\n", o.tags_file.c_str(), line_no, bad); return 64; }
        size_t s = 0;
        while (s < p.sample_names.size() && p.sample_names[s] != f[0]) s++;
        if (s == p.sample_names.size()) p.sample_names.push_back(f[0]);
        p.tag_pairs.push_back({tag_of(f[1], codes[0], RTX_TRIM_5P), single ? RTX_DEMUX_NO_TAG : tag_of("revcomp(" + f[2] + ")", revcomp(codes[1]), RTX_TRIM_3P), (uint32_t)s});
        if (o.tags_both) {
            if (single) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: --tags-both-orientations needs a rev_tag\n", o.tags_file.c_str(), line_no); return 64; }
            p.tag_pairs.push_back({tag_of(f[2], codes[1], RTX_TRIM_5P), tag_of("revcomp(" + f[1] + ")", revcomp(codes[0]), RTX_TRIM_3P), (uint32_t)s});
        }
    }
    std::vector<rtx_demux_tag> ct;
    for (const Oligo &t : p.tags) ct.push_back({t.codes.data(), (uint32_t)t.codes.size(), t.end});
    uint32_t x[5];  // the checks of the library on the list (rtx_demux_create makes them again): one read through the host function
    if (rtx_demux_read(&o.tag_params, ct.data(), (uint32_t)ct.size(), p.tag_pairs.data(), (uint32_t)p.tag_pairs.size(), nullptr, 0, &x[0], &x[1], &x[2], &x[3], &x[4]) != RTX_OK) {
        fprintf(stderr, "raxtax-hip: --tags: %s: %s\n", o.tags_file.c_str(), rtx_last_error());
        return 64;
    }
    p.identity["tags"] = fingerprint(o.tags_file) + ";mismatches=" + std::to_string(o.tag_params.max_mismatches) + ";offset=" + std::to_string(o.tag_params.max_offset) +
                         ";both=" + (o.tags_both ? "1" : "0");
    return 0;
}

// --contaminants: the set of 16-mers and the names of the records
int build_contaminant_set(const Options &o, Plan &p) {
    std::string text;
    if (!slurp(o.contam_file, text)) { fprintf(stderr, "raxtax-hip: --contaminants: cannot read %s\n", o.contam_file.c_str()); return 66; }
    rtx_queries *cq = nullptr;  // (the query parser: the labels need no lineage)
    if (rtx_queries_parse_fasta(text.data(), text.size(), nullptr, 0, &cq) != RTX_OK) { fprintf(stderr, "raxtax-hip: --contaminants: %s: %s\n", o.contam_file.c_str(), rtx_last_error()); return 66; }
    const uint8_t *cb = nullptr;
    const uint64_t *co = nullptr;
    rtx_queries_data(cq, &cb, &co);
    const uint64_t nc = rtx_queries_len(cq);
    for (uint64_t i = 0; i < nc; i++) {
        const std::string label = rtx_queries_label(cq, i);
        p.contam_names.push_back(label.substr(0, label.find_first_of(" \t")));
    }
    uint64_t keys = 0, slots = 0, fp = 0;
    const int brc = rtx_screen_set_build(nc, cb, co, &p.contam_set);
    rtx_queries_destroy(cq);
    if (brc != RTX_OK || rtx_screen_set_info(p.contam_set, &keys, &slots, nullptr, nullptr, &fp) != RTX_OK) {
        fprintf(stderr, "raxtax-hip: --contaminants: %s: %s\n", o.contam_file.c_str(), rtx_last_error());
        return 64;
    }
    char hex[24];
    snprintf(hex, sizeof hex, "%016llx", (ull)fp);
    p.identity["contaminants"] = "file=" + o.contam_file + ";minhits=" + std::to_string(o.contam.min_hits) + ";minpct=" + std::to_string(o.contam.min_pct) + ";keys=" + hex;
    fprintf(stderr, "[INFO ] --contaminants: %llu record(s) of %s, %llu distinct 16-mers in %llu slots; a read is a contaminant from %u hit(s) and %u %% of its windows on\n",
            (ull)nc, o.contam_file.c_str(), (ull)keys, (ull)slots, o.contam.min_hits, o.contam.min_pct);
    return 0;
}

// Everything between the argument loop and the checkpoint: what cannot work is refused here, in this order, and what the run needs of the options is
// left in the plan.  0, or the exit code behind the message
int validate(Options &o, Plan &p) {
    Identity &id = p.identity;
    id["db_fingerprint"] = fingerprint(o.db);
    id["raw_confidence"] = o.raw ? "true" : "false";
    id["skip_exact_matches"] = o.skip_exact ? "true" : "false";
    id["tsv"] = o.tsv ? "true" : "false";
    if (o.both_strands) id["strand"] = "both";
    if (o.want_hits) id["hits"] = "true";
    if (o.want_identity) id["identity"] = "true";
    if (o.profile_cutoff) id["profile"] = std::to_string(o.profile_cutoff);
    // FASTQ or FASTA: the first non-blank byte of the query file.  A filter option needs quality strings
    if (!o.qf.empty()) {
        Input f;
        if (f.open(o.qf)) {
            char c = 0;
            while (f.read(&c, 1) == 1 && isspace((unsigned char)c)) c = 0;
            p.fastq = c == '@';
            f.close();
        }
    }
    const char *const input = o.qf.empty() ? "-i" : o.qf.c_str();
    p.qual_on = !o.qual_spec.empty();
    if (p.qual_on && !p.fastq) {
        fprintf(stderr, "raxtax-hip: the quality filter (%s) needs FASTQ input: %s does not start with '@'\n", o.qual_spec.c_str(), input);
        return 64;
    }
    if (p.qual_on) id["quality"] = o.qual_spec + ";ascii=" + std::to_string(o.qual.ascii_base);
    // --reverse: paired input, merged before anything else
    p.merge_on = !o.rev_file.empty();
    if (orphan(o.merge_opts, p.merge_on, "sets how pairs are merged and needs --reverse FILE (the reverse mates)")) return 64;
    if (p.merge_on && !p.fastq) {
        fprintf(stderr, "raxtax-hip: --reverse needs FASTQ input: %s does not start with '@'\n", input);
        return 64;
    }
    if (p.merge_on) {
        o.merge.ascii_base = o.qual.ascii_base;
        id["merge"] = "reverse=" + o.rev_file + ";minovlen=" + std::to_string(o.merge.min_overlap) + ";maxdiffs=" + std::to_string(o.merge.max_diffs) + ";maxdiffpct=" +
                      std::to_string(o.merge.max_diff_pct) + ";qcap=" + std::to_string(o.merge.q_cap) + ";ascii=" + std::to_string(o.merge.ascii_base);
    }
    if (orphan(o.chim_opts, o.chim_on, "sets how reads are checked for chimeras and needs --chimera")) return 64;
    if (o.chim_on && o.both_strands) {
        fprintf(stderr, "raxtax-hip: --chimera checks a read in the orientation given and cannot go with --strand both\n");
        return 64;
    }
    if (o.chim_on) id["chimera"] = "segments=" + std::to_string(o.chim.segments) + ";mindelta=" + std::to_string(o.chim.mindelta);
    if (const int rc = primer_patterns(o, p)) return rc;
    p.tags_on = !o.tags_file.empty();
    if (orphan(o.tag_opts, p.tags_on, "sets how reads are assigned to samples and needs --tags SHEET")) return 64;
    if (p.tags_on && o.derep && o.profile_cutoff) {
        fprintf(stderr, "raxtax-hip: --tags cannot go with --derep and --profile together: copies from different samples would be counted as one read\n");
        return 64;
    }
    if (p.tags_on)
        if (const int rc = read_sample_sheet(o, p)) return rc;
    p.screen_on = !o.contam_file.empty();
    if (orphan(o.contam_opts, p.screen_on, "sets how reads are screened and needs --contaminants FILE")) return 64;
    if (p.screen_on)
        if (const int rc = build_contaminant_set(o, p)) return rc;
    if (orphan(o.uniques_opts, o.uniques, "sets how the distinct reads are kept and written and needs --uniques")) return 64;
    if (orphan(o.otus_opts.empty() ? "" : "--otus-minsize", o.otus, "sets what is written of the OTUs and needs --otus")) return 64;  // (named once, however often it was given)
    if (orphan(o.otus ? "--otus" : "", o.uniques, "clusters the distinct reads of the run and needs --uniques")) return 64;
    if (o.uniques) id["uniques"] = "minsize=" + std::to_string(o.uniques_minsize) + " max_entries=" + std::to_string(o.uniques_max_entries) + " max_bytes=" + std::to_string(o.uniques_max_bytes);
    if (o.otus) id["otus"] = "minsize=" + std::to_string(o.otus_minsize);
    if (orphan(o.fastidious_opts, o.fastidious, "sets which OTUs are grafted and needs --fastidious")) return 64;
    if (orphan(o.fastidious ? "--fastidious" : "", o.otus, "grafts the small OTUs of the run onto the large ones and needs --otus")) return 64;
    if (o.fastidious) id["fastidious"] = "boundary=" + std::to_string(o.fastidious_boundary ? o.fastidious_boundary : 3);
    if (orphan(o.unoise_opts, o.unoise, "sets how the distinct reads are denoised and needs --unoise")) return 64;
    if (orphan(o.unoise ? "--unoise" : "", o.otus, "denoises the distinct reads of the run into the OTUs and needs --otus")) return 64;
    if (o.unoise && o.fastidious) { fprintf(stderr, "raxtax-hip: --unoise and --fastidious exclude each other (grafting is a pass over a d = 1 clustering)\n"); return 64; }
    if (o.unoise)
        id["unoise"] = "minsize=" + std::to_string(o.unoise_params.minsize) + ";alpha=" + std::to_string(o.unoise_params.alpha) +
                       ";maxdiffs=" + std::to_string(o.unoise_params.max_diffs ? o.unoise_params.max_diffs : RTX_UNOISE_MAX_DIFFS);
    if (orphan(o.denovo_opts, o.denovo, "sets how the OTUs are checked for chimeras and needs --denovo")) return 64;
    if (orphan(o.denovo ? "--denovo" : "", o.otus, "checks the OTUs of the run for chimeras and needs --otus")) return 64;
    if (o.denovo)
        id["denovo"] = "abskew=" + std::to_string(o.denovo_params.abskew) + ";mindelta=" + std::to_string(o.denovo_params.mindelta) + ";segments=" + std::to_string(o.denovo_params.segments);
    if (orphan(o.otus_tax_opts.empty() ? "" : "--otus-tax-agree", o.otus_tax_cutoff != 0, "sets the share of an OTU's reads that must agree and needs --otus-tax CUTOFF")) return 64;
    if (orphan(o.otus_tax_cutoff ? "--otus-tax" : "", o.otus, "names the taxon of every OTU of the run and needs --otus")) return 64;
    if (o.otus_tax_cutoff) id["otus_tax"] = "cutoff=" + std::to_string(o.otus_tax_cutoff) + ";agree=" + std::to_string(o.otus_tax_agree);
    const char *const on_host = o.derep ? "--derep" : (o.both_strands ? "--strand both" : nullptr);
    if (o.device_format && on_host) {
        fprintf(stderr, "[INFO ] %s: the result lines are formatted on the host (--device-format has no effect)\n", on_host);
        o.device_format = false;
    }
    return 0;
}

// ---- the per-read reports

// What the callbacks of a run write to, and what they need to know
struct Sink {
    std::ofstream out, tsv, ckp, strand, hits, trim, qc, merge, chimera, demux, screen;
    bool want_tsv = false, want_strand = false, want_hits = false, want_qc = false;
    uint32_t screen_len = 0;                                 // the length of the range the screen was given, of the query whose callbacks are running
    const std::vector<std::string> *contam_names = nullptr;  // --contaminants: the records of the file (raxtax.screen)
    const std::vector<std::string> *sample_names = nullptr;  // --tags: the samples of the sheet (raxtax.demux)
    const rtx_tree *tree = nullptr;                          // the lineages of references (raxtax.hits, raxtax.chimera)
};

// A report of an option group: one line per read, in input order, written while the run classifies.  A rerun that resumes purges the lines of
// unfinished queries and goes on behind the rest; a run that starts over removes the file of a group that is off -- it would describe other lines
// (raxtax.out, raxtax.tsv and raxtax.ckp stand beside the table: they have no group, and a raxtax.tsv that is off is left alone)
struct Report { const char *name; bool on; const char *header; std::ofstream *stream; };

std::vector<Report> report_table(const Options &o, const Plan &p, Sink &s) {
    s.want_tsv = o.tsv;
    s.want_strand = o.both_strands;
    s.want_hits = o.want_hits;
    s.want_qc = p.qual_on;
    s.sample_names = &p.sample_names;
    s.contam_names = &p.contam_names;
    return {{"raxtax.strand", o.both_strands, nullptr, &s.strand},
            {"raxtax.hits", o.want_hits, nullptr, &s.hits},
            {"raxtax.trim", !p.primers.empty(), "label\tlength\tstart\tend\tprimer5\terrors5\tprimer3\terrors3\n", &s.trim},
            {"raxtax.demux", p.tags_on, "label\tsample\tverdict\ttag5\tmm5\toff5\ttag3\tmm3\toff3\tlo\thi\n", &s.demux},
            {"raxtax.qc", p.qual_on, "label\tlength\tstart\tend\texpected_errors\tverdict\n", &s.qc},
            {"raxtax.merge", p.merge_on, "label\tforward_length\treverse_length\toverlap\tdiffs\tmerged_length\tverdict\n", &s.merge},
            {"raxtax.chimera", o.chim_on, "label\tstatus\twindows\tsingle\tparent_id\tseg\tpos\tleft\ta_id\tright\tb_id\tdelta\tchimera\tparent\ta\tb\n", &s.chimera},
            {"raxtax.screen", p.screen_on, "label\tlength\twindows\thits\tfirst\tsource\tverdict\n", &s.screen}};
}

// The files written once, at the end of a run (--profile, --tags with --profile, --uniques, --otus, --fastidious, --unoise, --denovo, --otus-tax): a run that starts over removes them
const char *const kEndOfRunFiles[] = {"raxtax.profile", "raxtax.samples", "raxtax.uniques", "raxtax.uniques.tsv", "raxtax.otus", "raxtax.otus.map", "raxtax.otus.tsv",
                                      "raxtax.otus.grafts", "raxtax.otus.unoise", "raxtax.otus.denovo", "raxtax.otus.clean", "raxtax.otus.clean.tsv", "raxtax.otus.tax"};

// check_incomplete_output (io.rs:156-187): keep only the lines whose first field is a finished query
void purge_incomplete(const std::string &path, const std::set<std::string> &done, bool keep_header = false) {
    std::ifstream in(path);
    if (!in) return;
    std::vector<std::string> keep;
    bool rewrite = false;
    std::string line;
    while (std::getline(in, line)) {
        const size_t tab = line.find('\t');
        if (keep_header) { keep.push_back(line); keep_header = false; continue; }
        if (tab != std::string::npos && done.count(line.substr(0, tab))) keep.push_back(line);
        else rewrite = true;
    }
    in.close();
    if (!rewrite) return;
    const std::string tmp = path + ".tmp";
    {
        std::ofstream out(tmp, std::ios::trunc);
        for (const std::string &l : keep) out << l << '\n';
    }
    rename(tmp.c_str(), path.c_str());
}

// The writer of main.rs:127-135: result lines, then the label into the progress file
int sender(void *c, const char *label, const char *lines, const char *tsv_lines) {
    Sink *s = static_cast<Sink *>(c);
    if (s->want_tsv && tsv_lines) s->tsv << tsv_lines << '\n';
    s->out << lines << '\n';
    s->ckp << label << '\n';
    return s->out.good() && s->ckp.good() ? 0 : 1;
}

// ... and in front of them, under --strand both, which orientation the lines are of (raxtax.strand), and, under --hits, which reference they look
// like: peak, t, ties, id and lineage of the nearest reference ('-' twice where no reference shares a k-mer) -- the line of raxtax.hits without its end
void strand_and_nearest(Sink *s, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties) {
    if (s->want_strand) s->strand << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\n';
    if (!s->want_hits) return;
    s->hits << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\t' << ties << '\t';
    if (nearest == RTX_NO_REF) s->hits << "-\t-";
    else s->hits << nearest << '\t' << rtx_tree_lineage(s->tree, nearest);
}

int info(void *c, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t, uint32_t) {  // (in the shape of --identity's callback)
    Sink *s = static_cast<Sink *>(c);
    strand_and_nearest(s, label, strand, peak, t, nearest, ties);
    if (s->want_hits) s->hits << '\n';
    return (!s->want_strand || s->strand.good()) && (!s->want_hits || s->hits.good()) ? 0 : 1;
}

// ... and, under --identity (which implies --hits), how far the query is from it: the edit distance and the identity in percent behind the line of --hits
int align(void *c, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t dist, uint32_t qlen) {
    Sink *s = static_cast<Sink *>(c);
    strand_and_nearest(s, label, strand, peak, t, nearest, ties);
    if (dist == RTX_NO_DIST || qlen == 0u) {
        s->hits << "\t-\t-\n";
    } else {
        const uint64_t h = ((uint64_t)(qlen - dist) * 10000u + qlen / 2u) / qlen;  // hundredths of a percent
        char pct[32];
        snprintf(pct, sizeof pct, "%llu.%02llu", (ull)(h / 100u), (ull)(h % 100u));
        s->hits << '\t' << dist << '\t' << pct << '\n';
    }
    return (!s->want_strand || s->strand.good()) && s->hits.good() ? 0 : 1;
}

// ... and, under --primers, what was cut off every query (also one that has no result lines: an emptied read)
int trimmed(void *c, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint32_t hit) {
    Sink *s = static_cast<Sink *>(c);
    const uint32_t p5 = hit & 0xFFu, e5 = (hit >> 8) & 0xFFu, p3 = (hit >> 16) & 0xFFu, e3 = hit >> 24;
    s->trim << label << '\t' << raw_len << '\t' << lo << '\t' << hi << '\t';
    if (p5 == RTX_TRIM_NO_PATTERN) s->trim << "-\t-\t";
    else s->trim << p5 << '\t' << e5 << '\t';
    if (p3 == RTX_TRIM_NO_PATTERN) s->trim << "-\t-\n";
    else s->trim << p3 << '\t' << e3 << '\n';
    return s->trim.good() ? 0 : 1;
}

// The range of every query that is left behind primers and quality filter, and what the filter made of the query.  It serves two groups: the
// contaminant screen is given that range, and `screened` below prints its length; with a quality filter the line of raxtax.qc is written (also
// for a query without result lines: a discarded read).  So it is registered when either is on.
bool wants_range_and_quality(const Plan &p) { return p.qual_on || p.screen_on; }
int range_and_quality(void *c, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint64_t ee, uint32_t verdict) {
    static const char *const names[7] = {"bad_quality", "short_for_trunc_len", "too_short", "too_long", "too_many_n", "max_ee", "max_ee_rate"};
    Sink *s = static_cast<Sink *>(c);
    s->screen_len = verdict ? 0u : hi - lo;
    if (!s->want_qc) return 0;
    char frac[8];  // six decimals of ee / 2^40, truncated: from the integer, no floating point
    snprintf(frac, sizeof frac, "%06llu", (ull)(((ee & ((1ull << 40) - 1)) * 1000000ull) >> 40));
    s->qc << label << '\t' << raw_len << '\t' << lo << '\t' << hi << '\t' << (ee >> 40) << '.' << frac << '\t';
    if (!verdict) s->qc << "pass";
    for (uint32_t b = 0, first = 1; b < 7u; b++)
        if ((verdict >> b) & 1u) { s->qc << (first ? "" : "+") << names[b]; first = 0; }
    s->qc << '\n';
    return s->qc.good() ? 0 : 1;
}

// ... and, under --chimera, what the check made of every query (also one without result lines: a flagged read)
int checked(void *c, const char *label, const rtx_chimera_rec *r) {
    static const char *const status[3] = {"ok", "no_kmer", "too_long"};
    Sink *s = static_cast<Sink *>(c);
    auto id = [s](uint32_t ref) { if (ref == RTX_NO_REF) s->chimera << '-'; else s->chimera << ref; };
    auto lin = [s](uint32_t ref) { if (ref == RTX_NO_REF) s->chimera << '-'; else s->chimera << rtx_tree_lineage(s->tree, ref); };
    s->chimera << label << '\t' << status[r->status < 3u ? r->status : 0u] << '\t' << r->n_valid << '\t' << r->single << '\t';
    id(r->parent);
    s->chimera << '\t' << r->seg << '\t' << r->pos << '\t' << r->left << '\t';
    id(r->parent_a);
    s->chimera << '\t' << r->right << '\t';
    id(r->parent_b);
    s->chimera << '\t' << r->delta << '\t' << (r->status != RTX_CHIM_OK ? '?' : (r->flag ? 'Y' : 'N')) << '\t';
    lin(r->parent);
    s->chimera << '\t';
    lin(r->parent_a);
    s->chimera << '\t';
    lin(r->parent_b);
    s->chimera << '\n';
    return s->chimera.good() ? 0 : 1;
}

// ... and, under --contaminants, what the screen made of every query (also one without result lines: a contaminant)
int screened(void *c, const char *label, uint32_t windows, uint32_t hits, uint32_t first, uint32_t source, uint32_t verdict) {
    Sink *s = static_cast<Sink *>(c);
    s->screen << label << '\t' << s->screen_len << '\t' << windows << '\t' << hits << '\t';
    if (first == RTX_SCREEN_NONE) s->screen << '-';
    else s->screen << first;
    s->screen << '\t';
    if (source == RTX_SCREEN_NONE || source >= s->contam_names->size()) s->screen << '-';
    else s->screen << (*s->contam_names)[source];
    s->screen << '\t' << (verdict ? "contaminant" : "pass") << '\n';
    return s->screen.good() ? 0 : 1;
}

// ... and, under --tags, which sample every query belongs to (also one without result lines: a read that is not assigned)
int assigned(void *c, const char *label, uint32_t, uint32_t sample, uint32_t lo, uint32_t hi, uint32_t hit, uint32_t info) {
    static const char *const verdicts[5] = {"ok", "no_tag5", "no_tag3", "ambiguous", "unknown_pair"};
    Sink *s = static_cast<Sink *>(c);
    const uint32_t t5 = hit & 0xFFFFu, t3 = hit >> 16, v = info & 0xFFu;
    s->demux << label << '\t';
    if (sample == RTX_DEMUX_NONE || sample >= s->sample_names->size()) s->demux << '*';
    else s->demux << (*s->sample_names)[sample];
    s->demux << '\t' << verdicts[v < 5u ? v : 0u] << '\t';
    if (t5 == RTX_DEMUX_NO_TAG) s->demux << "-\t-\t-\t";
    else s->demux << t5 << '\t' << ((info >> 8) & 0xFFu) << '\t' << ((info >> 24) & 0xFu) << '\t';
    if (t3 == RTX_DEMUX_NO_TAG) s->demux << "-\t-\t-\t";
    else s->demux << t3 << '\t' << ((info >> 16) & 0xFFu) << '\t' << (info >> 28) << '\t';
    s->demux << lo << '\t' << hi << '\n';
    return s->demux.good() ? 0 : 1;
}

// ---- checkpoint and resume (io.rs:202-263): the labels a matching checkpoint lists as finished, the reports purged of everything else
int resume_or_start(const Options &o, const Plan &p, const std::vector<Report> &reports, std::set<std::string> &done, bool &resume) {
    const std::string ckp_json = o.prefix + "/raxtax.json", ckp_path = o.prefix + "/raxtax.ckp";
    if (!o.redo && is_file(ckp_json)) {
        std::string have;
        slurp(ckp_json, have);
        if (have == p.identity.json()) {  // checkpoint_valid (io.rs:288-302)
            std::ifstream f(ckp_path);
            std::string l;
            while (std::getline(f, l)) done.insert(l);
            // the queries of the earlier run are not classified again: their share of the sample is gone
            const char *const whole_run[2][2] = {{o.profile_cutoff ? "--profile" : nullptr, "the profile"}, {o.uniques ? "--uniques" : nullptr, "the table"}};
            for (const auto &w : whole_run)
                if (w[0] && !done.empty()) {
                    fprintf(stderr, "raxtax-hip: %s cannot resume a checkpoint with processed queries (%zu in %s): %s would miss them; "
                                    "run with --redo to classify the whole sample again\n", w[0], done.size(), ckp_path.c_str(), w[1]);
                    return 64;
                }
            purge_incomplete(o.prefix + "/raxtax.out", done);
            if (o.tsv) purge_incomplete(o.prefix + "/raxtax.tsv", done);
            for (const Report &r : reports)
                if (r.on) purge_incomplete(o.prefix + "/" + r.name, done, r.header != nullptr);
            resume = true;
            fprintf(stderr, "[INFO ] Restarting from checkpoint %s\n", ckp_json.c_str());
        }
    }
    if (is_dir(o.prefix) && !is_file(ckp_json) && !o.redo) {
        fprintf(stderr, "[ERROR] Output folder %s already exists! Please specify another folder with -o <PATH> or run with --redo "
                        "to force overriding existing files!\n", o.prefix.c_str());
        return 73;  // exitcode::CANTCREAT
    }
    mkdir(o.prefix.c_str(), 0777);
    return 0;
}

// ---- database: try the binary format first, then FASTA (parser.rs:37-44); db_bin: where its cache goes, empty for none
int load_database(const Options &o, bool resume, Laps &laps, rtx_tree *&tree, std::string &db_bin) {
    bool store_db = false;
    if (rtx_tree_load_bin(o.db.c_str(), &tree) != RTX_OK) {
        std::string db_text;
        // Tree.k_mer_map is only needed for the .bin cache: the device index is built from the sequences
        if (!slurp(o.db, db_text) || rtx_tree_parse_reference_fasta_ex(db_text.data(), db_text.size(), RTX_TREE_SKIP_KMER_MAP, &tree) != RTX_OK) {
            fprintf(stderr, "[ERROR] Failed to parse %s: %s\n", o.db.c_str(), rtx_last_error());
            return 66;  // exitcode::NOINPUT
        }
        store_db = true;
    }
    laps.lap("database");
    if (store_db && !o.skip_db) {  // main.rs:72-86, io.rs:269-286
        std::string base = o.db.substr(o.db.find_last_of('/') == std::string::npos ? 0 : o.db.find_last_of('/') + 1);
        const size_t dot = base.find_last_of('.');
        db_bin = o.prefix + "/" + (dot == std::string::npos ? base : base.substr(0, dot)) + ".bin";
        if (is_file(db_bin) && !o.redo && !resume) {
            fprintf(stderr, "[ERROR] Output database file %s already exists! Delete it or run with --redo\n", db_bin.c_str());
            return 73;
        }
    }
    return 0;
}

// The database cache is written on a thread of its own while the queries are parsed and classified
struct BinWriter {
    std::thread th;
    int rc = RTX_OK;
    std::string err;
    void start(rtx_tree *tree, const std::string &path) {
        if (path.empty()) return;
        th = std::thread([this, tree, path]() {
            rc = rtx_tree_save_bin(tree, path.c_str());
            if (rc != RTX_OK) err = rtx_last_error();
        });
    }
    bool join() {
        if (th.joinable()) th.join();
        if (rc != RTX_OK) fprintf(stderr, "[ERROR] Failed to write database: %s\n", err.c_str());
        return rc == RTX_OK;
    }
};

// ---- queries: the file is read and parsed block by block on a thread of its own (cut in front of header lines,
// rtx_fasta_block_end; FASTQ: behind whole records, rtx_fastq_block_end), so that ingest overlaps with classification and memory stays bounded for very large
// files (the reference reads the whole file, parser.rs:112-115).  Already finished labels are dropped
// (parser.rs:150-153).

struct Parsed { rtx_queries *qs = nullptr; int rc = RTX_OK; std::string err; bool end = false; double merge_s[3] = {0, 0, 0}; float merge_ms = 0; };

// The parsed blocks between the reader's thread and the loop over blocks
class BlockQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Parsed> ready;  // at most two blocks ahead
    bool stop = false;

public:
    void push(Parsed &&pz) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return ready.size() < 2 || stop; });
        ready.push_back(std::move(pz));
        cv.notify_all();
    }
    void fail(int rc, const std::string &msg) { push(Parsed{nullptr, rc, msg, true}); }  // the last block of a file that cannot be read on
    Parsed pop() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return !ready.empty(); });
        Parsed pz = std::move(ready.front());
        ready.pop_front();
        cv.notify_all();
        return pz;
    }
    bool stopped() {
        std::lock_guard<std::mutex> g(mu);
        return stop;
    }
    void stop_and_join(std::thread &reader) {  // the reader leaves behind its next block; what it had queued is released
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
            cv.notify_all();
        }
        reader.join();
        for (Parsed &pz : ready) rtx_queries_destroy(pz.qs);
    }
};

void read_single(const Options &o, bool fastq, const std::vector<const char *> &skip, BlockQueue &q) {
    Input f;
    if (!f.open(o.qf)) { q.fail(RTX_ERR_PARSE, "cannot open file"); return; }
    std::string buf;
    bool first = true, eof = false;
    while (!eof) {
        if (!read_on(f, buf, o.block_bytes, eof)) { q.fail(RTX_ERR_PARSE, "read error (corrupt gzip stream?)"); break; }
        uint64_t end = buf.size();
        uint32_t flags = first ? 0u : RTX_FASTA_NOT_FIRST;
        if (!eof) {
            end = fastq ? rtx_fastq_block_end(buf.data(), buf.size()) : rtx_fasta_block_end(buf.data(), buf.size());
            if (end == 0) continue;  // no header (FASTQ: no whole record) inside the block yet: read on
            flags |= RTX_FASTA_MORE_FOLLOWS;
        }
        Parsed pz;
        pz.rc = fastq ? rtx_queries_parse_fastq_block(buf.data(), end, skip.empty() ? nullptr : skip.data(), skip.size(), o.qual.ascii_base, flags, &pz.qs)
                      : rtx_queries_parse_fasta_block(buf.data(), end, skip.empty() ? nullptr : skip.data(), skip.size(), flags, &pz.qs);
        if (pz.rc != RTX_OK) pz.err = rtx_last_error();
        pz.end = eof || pz.rc != RTX_OK;
        const bool failed = pz.rc != RTX_OK;
        q.push(std::move(pz));
        if (failed || q.stopped()) break;
        buf.erase(0, end);
        first = false;
    }
    f.close();
}

// Paired input: both files block by block, cut at the same record (rtx_fastq_block_end_n), parsed, and merged on the first device
// of the run; what is queued is the handle of merged reads.  Nothing behind the queue knows.
void read_paired(const Options &o, const std::vector<const char *> &skip, BlockQueue &q) {
    Input in[2];
    const std::string *name[2] = {&o.qf, &o.rev_file};
    if (!in[0].open(o.qf)) { q.fail(RTX_ERR_PARSE, "cannot open file"); return; }
    if (!in[1].open(o.rev_file)) { in[0].close(); q.fail(RTX_ERR_PARSE, "cannot open " + o.rev_file); return; }
    rtx_merge *stage = nullptr;
    if (const int mrc = rtx_merge_create(o.devices[0], &o.merge, &stage)) {
        q.fail(mrc, std::string("paired-end merging on device ") + std::to_string(o.devices[0]) + ": " + rtx_last_error());
        in[0].close();
        in[1].close();
        return;
    }
    std::string buf[2];
    bool eof[2] = {false, false};
    uint64_t records = 0;  // pairs handed on so far
    bool force = false;
    for (;;) {
        bool failed = false;
        for (int k = 0; k < 2 && !failed; k++) {
            if (eof[k] || (buf[k].size() >= o.block_bytes && !force)) continue;
            if (!read_on(in[k], buf[k], o.block_bytes, eof[k])) { q.fail(RTX_ERR_PARSE, "read error in " + *name[k] + " (corrupt gzip stream?)"); failed = true; break; }
            if (eof[k] && !buf[k].empty() && buf[k].back() != '\n') buf[k].push_back('\n');  // (the last record may lack its newline: counted as whole from here on)
        }
        if (failed) break;
        force = false;
        uint64_t n_rec[2] = {0, 0}, end[2] = {0, 0};
        for (int k = 0; k < 2; k++) (void)rtx_fastq_block_end_n(buf[k].data(), buf[k].size(), ~0ull, &n_rec[k]);
        const bool last = eof[0] && eof[1];
        const uint64_t take = std::min(n_rec[0], n_rec[1]);
        if (!last && take == 0) {
            const int out = eof[0] ? 0 : (eof[1] ? 1 : -1);
            if (out >= 0 && n_rec[out] == 0 && n_rec[1 - out] > 0) {
                q.fail(RTX_ERR_PARSE, "paired FASTQ: " + *name[out] + " ends after record " + std::to_string(records) + ", " + *name[1 - out] + " goes on");
                break;
            }
            force = true;  // no whole record of one file yet: read on
            continue;
        }
        for (int k = 0; k < 2; k++) end[k] = last ? buf[k].size() : rtx_fastq_block_end_n(buf[k].data(), buf[k].size(), take, nullptr);
        auto blank = [](const std::string &t) { return t.find_first_not_of(" \t\r\n\v\f") == std::string::npos; };
        Parsed pz;
        pz.end = last;
        if (last && blank(buf[0]) && blank(buf[1])) { q.push(std::move(pz)); break; }  // both files ended with the block before
        if (last && n_rec[0] != n_rec[1]) {  // the files run out at different records
            const int out = n_rec[0] < n_rec[1] ? 0 : 1;
            q.fail(RTX_ERR_PARSE, "paired FASTQ: " + *name[out] + " ends after record " + std::to_string(records + n_rec[out]) + ", " + *name[1 - out] + " goes on");
            break;
        }
        rtx_queries *mates[2] = {nullptr, nullptr};
        for (int k = 0; k < 2 && pz.rc == RTX_OK; k++) {
            pz.rc = rtx_queries_parse_fastq_block(buf[k].data(), end[k], nullptr, 0, o.qual.ascii_base, 0u, &mates[k]);
            if (pz.rc != RTX_OK) pz.err = *name[k] + ", records from " + std::to_string(records + 1) + " on: " + rtx_last_error();
        }
        if (pz.rc == RTX_OK) {
            pz.rc = rtx_merge_queries(stage, mates[0], mates[1], skip.empty() ? nullptr : skip.data(), skip.size(), &pz.qs);
            if (pz.rc != RTX_OK) pz.err = "pairs from record " + std::to_string(records + 1) + " on: " + rtx_last_error();
            else { (void)rtx_merge_stage_times(stage, pz.merge_s); (void)rtx_merge_kernel_time(stage, &pz.merge_ms); }
        }
        rtx_queries_destroy(mates[0]);
        rtx_queries_destroy(mates[1]);
        records += take;
        failed = pz.rc != RTX_OK;
        pz.end = last || failed;
        q.push(std::move(pz));
        if (failed || last || q.stopped()) break;
        for (int k = 0; k < 2; k++) buf[k].erase(0, end[k]);
    }
    rtx_merge_destroy(stage);
    in[0].close();
    in[1].close();
}

// ---- handles: one index handle per device, created side by side (each on a thread of its own: the builds run on their GPUs), with everything the
// options turn on; --uniques: a tally per handle as well, alive over the blocks of the file
bool create_handles(const Options &o, const Plan &p, const rtx_tree *tree, std::vector<rtx_index *> &indices, std::vector<rtx_tally *> &tallies) {
    const size_t nd = o.devices.size();
    const uint32_t n_samples = p.tags_on ? (uint32_t)p.sample_names.size() : 0u, mode = (o.skip_exact ? RTX_SKIP_EXACT_MATCHES : 0u) | (o.raw ? RTX_RAW_CONFIDENCE : 0u);
    std::vector<int> rcs(nd, RTX_OK);
    std::vector<std::string> errs(nd);
    std::vector<std::thread> th;
    for (size_t k = 0; k < nd; k++)
        th.emplace_back([&, k] {
            rtx_index *&ix = indices[k];
            int &rc = rcs[k];
            rc = rtx_index_create_from_tree(o.devices[k], tree, &ix);
            const std::pair<bool, int> flags[] = {{o.device_format, RTX_OPT_DEVICE_TEXT}, {o.both_strands, RTX_OPT_STRAND}, {o.want_hits, RTX_OPT_NEAREST},
                                                       {o.want_identity, RTX_OPT_IDENTITY}, {o.derep, RTX_OPT_DEREP}};
            for (const auto &f : flags)
                if (rc == RTX_OK && f.first) rc = rtx_index_set_option(ix, f.second, 1);
            if (rc == RTX_OK && !p.primers.empty()) {
                std::vector<rtx_trim_pattern> pats;
                for (const Oligo &pr : p.primers) pats.push_back({pr.codes.data(), (uint32_t)pr.codes.size(), pr.end, (uint32_t)(pr.codes.size() * o.primer_pct / 100u), o.primer_window});
                rc = rtx_index_set_primers(ix, pats.data(), (uint32_t)pats.size());
            }
            if (rc == RTX_OK && p.tags_on) {
                std::vector<rtx_demux_tag> ct;
                for (const Oligo &t : p.tags) ct.push_back({t.codes.data(), (uint32_t)t.codes.size(), t.end});
                rc = rtx_index_set_tags(ix, ct.data(), (uint32_t)ct.size(), p.tag_pairs.data(), (uint32_t)p.tag_pairs.size(), &o.tag_params);
            }
            if (rc == RTX_OK && p.qual_on) rc = rtx_index_set_quality(ix, &o.qual);
            if (rc == RTX_OK && p.screen_on) rc = rtx_index_set_screen(ix, p.contam_set, &o.contam);
            if (rc == RTX_OK && o.chim_on) rc = rtx_index_set_chimera(ix, &o.chim);
            if (rc == RTX_OK && o.uniques) {
                const rtx_tally_params tp{n_samples, o.uniques_max_entries, o.uniques_max_bytes, 0, 0};
                rc = rtx_tally_create(o.devices[k], &tp, &tallies[k]);
                if (rc == RTX_OK) rc = rtx_index_set_tally(ix, tallies[k]);
            }
            if (rc == RTX_OK && o.profile_cutoff && p.tags_on)  // ... with a column of counters per sample (PREFIX/raxtax.samples)
                rc = rtx_index_profile_begin_samples(ix, o.profile_cutoff, mode, n_samples);
            else if (rc == RTX_OK && o.profile_cutoff)
                rc = rtx_index_profile_begin(ix, o.profile_cutoff, mode);
            if (rc != RTX_OK) errs[k] = rtx_last_error();
        });
    for (auto &t : th) t.join();
    for (size_t k = 0; k < nd; k++)
        if (rcs[k] != RTX_OK) {
            fprintf(stderr, "[ERROR] device %d: %s\n", o.devices[k], errs[k].c_str());
            return false;
        }
    return true;
}

// The streams of a run: behind what a resumed run kept, over what an earlier run left otherwise; and what the log says of the groups that are on
void open_reports(const Options &o, const Plan &p, const std::vector<Report> &reports, Sink &s, bool fresh) {
    const auto mode = fresh ? std::ios::trunc : std::ios::app;
    s.out.open(o.prefix + "/raxtax.out", mode);
    s.ckp.open(o.prefix + "/raxtax.ckp", mode);
    if (o.tsv) s.tsv.open(o.prefix + "/raxtax.tsv", mode);
    for (const Report &r : reports) {
        const std::string path = o.prefix + "/" + r.name;
        if (r.on) {
            const bool header = r.header && (fresh || !is_file(path));
            r.stream->open(path, mode);
            if (header) *r.stream << r.header;
        } else if (fresh) remove(path.c_str());
    }
    if (fresh)
        for (const char *name : kEndOfRunFiles) remove((o.prefix + "/" + name).c_str());
    for (size_t k = 0; k < p.primers.size(); k++)
        fprintf(stderr, "[INFO ] --primers: pattern %zu at the %s end: %s, at most %zu error(s)\n", k, p.primers[k].end == RTX_TRIM_3P ? "3'" : "5'", p.primers[k].name.c_str(),
                p.primers[k].codes.size() * o.primer_pct / 100u);
    for (size_t k = 0; k < p.tags.size(); k++)
        fprintf(stderr, "[INFO ] --tags: tag %zu at the %s end: %s\n", k, p.tags[k].end == RTX_TRIM_3P ? "3'" : "5'", p.tags[k].name.c_str());
    if (p.tags_on)
        fprintf(stderr, "[INFO ] --tags: %zu samples, %zu pairs, at most %u mismatch(es), at most %u base(s) in front of a tag\n", p.sample_names.size(), p.tag_pairs.size(),
                o.tag_params.max_mismatches, o.tag_params.max_offset);
    if (p.merge_on)
        fprintf(stderr, "[INFO ] --reverse: pairs of %s and %s are merged on device %d: overlap at least %u, at most %u diffs and %u %% of the overlap, Q capped at %u\n", o.qf.c_str(),
                o.rev_file.c_str(), o.devices[0], o.merge.min_overlap, o.merge.max_diffs, o.merge.max_diff_pct, o.merge.q_cap);
    if (o.chim_on) fprintf(stderr, "[INFO ] --chimera: %u segments, a read is flagged from delta %u on\n", o.chim.segments, o.chim.mindelta);
}

// ---- the stages in front of the classification and what they count over the blocks of the file.  The rows in the order of the [TIMING] lines of a
// block; key: "<key>_busy" in the JSON of --timing; n counters, the first the queries; second: what the second counter is, where the line of a block
// names it; last: the counters and the busy seconds of the last call of rtx_raxtax_multi_ex*
struct Stage { const char *name, *key, *second; int n; int (*last)(uint64_t *c, double *busy); };
enum { SCREEN, DEMUX, TRIM, QUAL, CHIMERA, DEREP, MERGE, N_STAGES };
const Stage kStages[N_STAGES] = {
    {"contaminant screen", "screen", nullptr, 3, [](uint64_t *c, double *b) { return rtx_raxtax_last_screen(c, c + 1, c + 2, b); }},       // queries, screened, contaminants
    {"demultiplexing", "demux", nullptr, 7, [](uint64_t *c, double *b) { return rtx_raxtax_last_demux(c, c + 1, c + 2, b); }},               // queries, assigned, and the queries of every verdict
    {"primer trimming", "trim", nullptr, 4, [](uint64_t *c, double *b) { return rtx_raxtax_last_trim(c, c + 1, c + 2, c + 3, b); }},         // queries, with a 5' primer, with a 3' primer, emptied
    {"quality filter", "qual", nullptr, 10, [](uint64_t *c, double *b) { return rtx_raxtax_last_qual(c, c + 1, c + 2, c + 3, b); }},         // queries, passed, cut short, the seven reasons
    {"chimera check", "chimera", "reads checked", 3, [](uint64_t *c, double *b) { return rtx_raxtax_last_chimera(c, c + 1, c + 2, b); }},  // queries, reads checked, queries flagged
    {"dereplication", "derep", "distinct", 2, [](uint64_t *c, double *b) { return rtx_raxtax_last_derep(c, c + 1, b); }},                   // queries, distinct (per chunk)
    {nullptr, "merge", nullptr, 6, nullptr},  // --reverse, on the reader's thread (merge_report): pairs, merged, and not merged for each of the four reasons (RTX_MG_*)
};
struct Totals { bool on = false; ull c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; double busy = 0; };

// What the merge made of every pair of a block (raxtax.merge), before the block is classified
void merge_report(const Options &o, const Parsed &pz, uint64_t nb, const char *const *labels, const uint64_t *off, Sink &sink, Totals &tot) {
    static const char *const names[4] = {"bad_quality", "too_long", "too_short", "no_overlap"};
    const uint32_t *mnf, *mnr, *mov, *md, *mv;
    if (rtx_queries_merge_report(pz.qs, &mnf, &mnr, &mov, &md, &mv) == RTX_OK)
        for (uint64_t i = 0; i < nb; i++) {
            const char *verdict = "merged";
            tot.c[0]++;
            if (!mv[i]) tot.c[1]++;
            for (uint32_t b = 0; b < 4u; b++)
                if ((mv[i] >> b) & 1u) { verdict = names[b]; tot.c[2 + b]++; break; }
            sink.merge << labels[i] << '\t' << mnf[i] << '\t' << mnr[i] << '\t' << mov[i] << '\t' << md[i] << '\t' << (off[i + 1] - off[i]) << '\t' << verdict << '\n';
        }
    tot.busy += pz.merge_s[2];
    if (o.timing) fprintf(stderr, "[TIMING] merging of this block: %llu pairs, kernel %.3f ms, staging %.3f s, copies and wait %.3f s, all %.3f s (on the reader's thread, beside the classification of the block before)\n",
                          (ull)nb, pz.merge_ms, pz.merge_s[0], pz.merge_s[1], pz.merge_s[2]);
}

// ---- the loop over blocks: every block of the reader through rtx_raxtax_multi_ex8.  The library's code of the run; parse_failed: the reader gave up
int classify_blocks(const Options &o, const Plan &p, BlockQueue &queue, std::vector<rtx_index *> &indices, const rtx_tree *tree, Sink &sink, Totals *tot, uint64_t &n, bool &parse_failed) {
    int rc = RTX_OK;
    for (;;) {
        Parsed pz = queue.pop();
        if (pz.rc != RTX_OK) {
            fprintf(stderr, "[ERROR] Failed to parse %s: %s\n", o.qf.c_str(), pz.err.c_str());
            parse_failed = true;
            break;
        }
        const uint64_t nb = rtx_queries_len(pz.qs);
        if (nb) {
            std::vector<const char *> labels(nb);
            for (uint64_t i = 0; i < nb; i++) labels[i] = rtx_queries_label(pz.qs, i);
            const uint8_t *bases;
            const uint64_t *off;
            rtx_queries_data(pz.qs, &bases, &off);
            if (p.merge_on) merge_report(o, pz, nb, labels.data(), off, sink, tot[MERGE]);
            // Chunks of 131 072 queries are what a device handles best (two sub-batches of 65 536 on its two streams, the next chunk enqueued ahead:
            // 43 ms per 524 288 queries against 101-113 with chunks of 32 768, the default until round 6); smaller ones when the block would
            // otherwise leave a device without two chunks of its own, never below 32 768.
            const size_t per_dev = (size_t)((nb + 2 * indices.size() - 1) / (2 * indices.size()));
            const size_t chunk_now = o.chunk ? o.chunk : std::min<size_t>(131072, std::max<size_t>(32768, per_dev));
            // one entry point takes everything a run can bring: an option that is off passes no callback
            const uint8_t *quals = nullptr;
            if (p.qual_on) rtx_queries_quals(pz.qs, &quals);
            rc = rtx_raxtax_multi_ex8(indices.data(), (uint32_t)indices.size(), tree, nb, labels.data(), bases, off, o.skip_exact, o.raw, chunk_now, sender, &sink, o.tsv,
                                      o.want_identity ? align : (o.both_strands || o.want_hits ? info : nullptr), &sink, p.primers.empty() ? nullptr : trimmed, &sink,
                                      quals, wants_range_and_quality(p) ? range_and_quality : nullptr, &sink, o.chim_on ? checked : nullptr, &sink, p.tags_on ? assigned : nullptr, &sink,
                                      p.screen_on ? screened : nullptr, &sink);
            n += nb;
            for (int s = 0; s < MERGE; s++) {
                if (!tot[s].on) continue;
                const Stage &st = kStages[s];
                uint64_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                double busy = 0;
                if (st.last(c, &busy) == RTX_OK) {
                    for (int k = 0; k < st.n; k++) tot[s].c[k] += c[k];
                    tot[s].busy += busy;
                }
                if (o.timing && st.second) fprintf(stderr, "[TIMING] %s of this block: %llu queries, %llu %s, busy %.3f s (ahead of the device stage)\n", st.name, (ull)c[0], (ull)c[1], st.second, busy);
                else if (o.timing) fprintf(stderr, "[TIMING] %s of this block: %llu queries, busy %.3f s (ahead of the device stage)\n", st.name, (ull)c[0], busy);
            }
            if (o.timing) {  // busy seconds of the pipeline stages of this block (which stage bounds the run)
                double busy[4];
                uint64_t nch = 0;
                if (rtx_raxtax_last_timing(busy, &nch) == RTX_OK)
                    fprintf(stderr, "[TIMING] pipeline busy seconds over %llu chunk(s) on %zu handle(s): lookup %.3f, device %.3f (busiest handle), format %.3f, sender %.3f\n",
                            (ull)nch, indices.size(), busy[0], busy[1], busy[2], busy[3]);
                uint64_t ahead = 0, abandoned = 0;  // RTX_OPT_RUN_AHEAD (the first handle, since its creation)
                if (rtx_index_run_ahead_stats(indices[0], &ahead, &abandoned) == RTX_OK)
                    fprintf(stderr, "[TIMING] chunks enqueued ahead of the end of the chunk before them: %llu, abandoned: %llu (queries of this block: %llu)\n", (ull)ahead,
                            (ull)abandoned, (ull)nb);
            }
        }
        rtx_queries_destroy(pz.qs);
        if (rc != RTX_OK || pz.end) break;
    }
    return rc;
}

// What the stages that were on counted over the run, to the log, and their busy seconds to the JSON of --timing: merge, tags, primers, quality,
// contaminants, chimera, derep
void print_totals(const Options &o, const Totals *tot, Laps &laps) {
    const ull *c = tot[MERGE].c;
    if (tot[MERGE].on)
        fprintf(stderr, "[INFO ] --reverse: %llu pairs, %llu merged; not merged for bad_quality %llu, too_long %llu, too_short %llu, no_overlap %llu\n", c[0], c[1], c[2], c[3], c[4], c[5]);
    c = tot[DEMUX].c;
    if (tot[DEMUX].on)
        fprintf(stderr, "[INFO ] --tags: %llu queries, %llu assigned to a sample; not assigned for no_tag5 %llu, no_tag3 %llu, ambiguous %llu, unknown_pair %llu\n",
                c[0], c[1], c[3], c[4], c[5], c[6]);
    c = tot[TRIM].c;
    if (tot[TRIM].on) fprintf(stderr, "[INFO ] --primers: %llu queries, %llu with a 5' primer, %llu with a 3' primer, %llu left empty\n", c[0], c[1], c[2], c[3]);
    c = tot[QUAL].c;
    if (tot[QUAL].on)
        fprintf(stderr, "[INFO ] quality filter: %llu queries, %llu passed (%llu of them cut short); discarded for bad_quality %llu, short_for_trunc_len %llu, too_short %llu, "
                        "too_long %llu, too_many_n %llu, max_ee %llu, max_ee_rate %llu\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]);
    c = tot[SCREEN].c;
    if (tot[SCREEN].on) fprintf(stderr, "[INFO ] --contaminants: %llu queries, %llu screened, %llu contaminants\n", c[0], c[1], c[2]);
    c = tot[CHIMERA].c;
    if (tot[CHIMERA].on) fprintf(stderr, "[INFO ] --chimera: %llu queries, %llu reads checked, %llu queries flagged\n", c[0], c[1], c[2]);
    c = tot[DEREP].c;
    if (tot[DEREP].on) fprintf(stderr, "[INFO ] --derep: %llu queries, %llu distinct\n", c[0], c[1]);  // (per chunk: a copy in another chunk counts as a distinct read of its own)
    for (int s : {MERGE, DEMUX, TRIM, QUAL, SCREEN, CHIMERA, DEREP})
        if (tot[s].on && o.timing) laps.log << ", \"" << kStages[s].key << "_busy\": " << tot[s].busy;
}

// ---- the files written at the end of a run.  Each: 0, or the exit code behind the message

// --profile: the taxon profile of the whole run: the sum over the handles, written once
int write_profile(const Options &o, const std::vector<rtx_index *> &indices, const rtx_tree *tree) {
    std::vector<rtx_profile_view> views(indices.size());
    std::vector<rtx_profile_view *> ptrs(indices.size());
    int prc = RTX_OK;
    for (size_t k = 0; k < indices.size() && prc == RTX_OK; k++) {
        prc = rtx_index_profile_read(indices[k], &views[k]);
        ptrs[k] = &views[k];
    }
    const size_t nn = prc == RTX_OK ? views[0].n_nodes : 0;
    std::vector<uint64_t> acc(3 * nn);
    uint64_t totals[4] = {0, 0, 0, 0};
    if (prc == RTX_OK) prc = rtx_profile_merge(ptrs.data(), (uint32_t)ptrs.size(), acc.data(), acc.data() + nn, acc.data() + 2 * nn, totals);
    std::string text;
    if (prc == RTX_OK)
        prc = format_two_pass(text, [&](char *buf, uint64_t cap) { return rtx_profile_format(tree, acc.data(), acc.data() + nn, acc.data() + 2 * nn, totals, o.profile_cutoff, buf, cap); });
    if (prc != RTX_OK) { fprintf(stderr, "[ERROR] taxon profile: %s\n", rtx_last_error()); return 70; }
    return write_whole(o.prefix + "/raxtax.profile", text) ? 0 : 74;
}

// --profile with --tags: the taxon x sample table beside it: the per-sample counters summed over the handles
int write_sample_table(const Options &o, const Plan &p, const std::vector<rtx_index *> &indices, const rtx_tree *tree) {
    std::vector<rtx_sample_profile_view> views(indices.size());
    std::vector<rtx_sample_profile_view *> ptrs(indices.size());
    int prc = RTX_OK;
    for (size_t k = 0; k < indices.size() && prc == RTX_OK; k++) {
        prc = rtx_index_profile_read_samples(indices[k], &views[k]);
        ptrs[k] = &views[k];
    }
    const size_t nn = prc == RTX_OK ? views[0].n_nodes : 0, ns = p.sample_names.size();
    std::vector<uint64_t> direct(ns * nn + 1), totals(ns * 4);
    if (prc == RTX_OK) prc = rtx_sample_profile_merge(ptrs.data(), (uint32_t)ptrs.size(), direct.data(), totals.data());
    std::vector<const char *> names;
    for (const std::string &s : p.sample_names) names.push_back(s.c_str());
    std::string text;
    if (prc == RTX_OK)
        prc = format_two_pass(text, [&](char *buf, uint64_t cap) { return rtx_sample_table_format(tree, (uint32_t)ns, names.data(), direct.data(), totals.data(), o.profile_cutoff, buf, cap); });
    if (prc != RTX_OK) { fprintf(stderr, "[ERROR] sample table: %s\n", rtx_last_error()); return 70; }
    return write_whole(o.prefix + "/raxtax.samples", text) ? 0 : 74;
}

// --otus-tax: the rows of the table classified once more through the first handle, in chunks, in table order (no front stage: the rows went through
// the front already); every chunk turned into records; then the consensus of every OTU on the first device
int write_otu_taxonomy(const Options &o, rtx_index *ix, const rtx_tree *tree, const rtx_tally_view &view, const rtx_otu_view_t &ov, uint64_t minsize) {
    const auto t0 = std::chrono::steady_clock::now();
    rtx_nodes_view nodes{};
    int trc = rtx_tree_nodes(tree, &nodes);
    uint32_t stride = 0;  // the deepest lineage of the tree: the nodes come breadth first, so the last one is among the deepest
    for (uint32_t u = trc == RTX_OK && nodes.n_nodes ? nodes.n_nodes - 1u : 0u; u != 0 && stride < RTX_MAX_DEPTH; u = nodes.node_parent[u]) stride++;
    stride = std::max(stride, 1u);
    const uint64_t n = view.n_entries, step = o.chunk ? o.chunk : 65536;
    const uint32_t flags = (o.skip_exact ? RTX_SKIP_EXACT_MATCHES : 0u) | (o.raw ? RTX_RAW_CONFIDENCE : 0u);
    std::vector<uint8_t> kind(n), depth(n), hund(n * stride);
    std::vector<uint32_t> node(n);
    const bool lookup = rtx_index_has_exact_lookup(ix) != 0;
    std::vector<uint64_t> x_off;
    std::vector<uint32_t> x_ids;
    if (trc == RTX_OK && o.profile_cutoff) trc = rtx_index_profile_end(ix);  // (the profile of the run is written: the second pass is not part of it)
    for (uint64_t a = 0; a < n && trc == RTX_OK; a += step) {
        const uint64_t m = std::min(step, n - a);
        const uint64_t *xo = nullptr;
        const uint32_t *xi = nullptr;
        if (!lookup) {  // Tree.sequences.get on the host, as the run itself does for such a handle
            x_off.assign(m + 1, 0);
            x_ids.assign(16, 0);
            const uint64_t tot = rtx_tree_exact_matches_batch(tree, m, view.bases, view.base_off + a, x_off.data(), x_ids.data(), x_ids.size());
            if (tot > x_ids.size()) {
                x_ids.assign(tot, 0);
                rtx_tree_exact_matches_batch(tree, m, view.bases, view.base_off + a, x_off.data(), x_ids.data(), x_ids.size());
            }
            xo = x_off.data();
            xi = x_ids.data();
        }
        rtx_result_view res{};
        trc = rtx_classify_batch(ix, m, view.bases, view.base_off + a, xi, xo, flags, &res);
        if (trc == RTX_OK && lookup) trc = rtx_batch_exact_matches(ix, &xo, &xi);
        if (trc == RTX_OK)
            trc = rtx_result_best_lineages(tree, &res, xi, xo, o.otus_tax_cutoff, flags, kind.data() + a, depth.data() + a, node.data() + a, hund.data() + a * stride, stride);
    }
    const rtx_lineage_records rec{kind.data(), depth.data(), node.data(), hund.data(), stride};
    const rtx_otu_taxonomy_params prm{o.otus_tax_agree, 0};
    rtx_otutax *tax = nullptr;
    if (trc == RTX_OK) trc = rtx_otu_taxonomy(o.devices[0], n, ov.otu, view.sizes, ov.n_otus, ov.seed, &rec, &nodes, &prm, &tax);
    rtx_otu_taxonomy_view_t tv{};
    std::string text;
    if (trc == RTX_OK) trc = rtx_otu_taxonomy_view(tax, &tv);
    if (trc == RTX_OK) trc = format_two_pass(text, [&](char *buf, uint64_t cap) { return rtx_otu_taxonomy_format(tax, tree, minsize, buf, cap); });
    uint64_t named = 0;
    for (uint64_t k = 0; trc == RTX_OK && k < tv.n_otus; k++) named += tv.depth[k] != 0;
    rtx_otu_taxonomy_destroy(tax);
    if (trc != RTX_OK) { fprintf(stderr, "[ERROR] OTU taxonomy: %s\n", rtx_last_error()); return 70; }
    fprintf(stderr, "[INFO ] --otus-tax: %llu OTUs, %llu with a taxon, %.3f s for the second pass over %llu distinct reads\n", (ull)tv.n_otus, (ull)named,
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), (ull)n);
    return write_whole(o.prefix + "/raxtax.otus.tax", text) ? 0 : 74;
}

// --uniques: the distinct reads of the whole run: the tables of the handles' objects read, summed and written once;
// --otus: the summed table, whole, clustered on the first device
int write_uniques_and_otus(const Options &o, const Plan &p, const std::vector<rtx_tally *> &tallies, rtx_index *first, const rtx_tree *tree) {
    struct Owned {  // what the function makes, released on every way out
        std::vector<rtx_tally_table *> tables;
        rtx_tally_table *sum = nullptr;
        rtx_otu *otu = nullptr;
        rtx_denovo *dn = nullptr;
        ~Owned() {
            rtx_denovo_destroy(dn);
            rtx_otu_destroy(otu);
            rtx_tally_table_destroy(sum);
            for (rtx_tally_table *t : tables) rtx_tally_table_destroy(t);
        }
    } own;
    own.tables.assign(tallies.size(), nullptr);
    std::vector<rtx_tally_table *> &tables = own.tables;
    rtx_tally_table *&sum = own.sum;
    int trc = RTX_OK;
    for (size_t k = 0; k < tallies.size() && trc == RTX_OK; k++) trc = rtx_tally_read(tallies[k], &tables[k]);
    if (trc == RTX_OK) trc = rtx_tally_table_merge(tables.data(), (uint32_t)tables.size(), &sum);
    rtx_tally_view view{};
    if (trc == RTX_OK) trc = rtx_tally_table_view(sum, &view);
    std::vector<const char *> names;
    for (const std::string &s : p.sample_names) names.push_back(s.c_str());
    std::string fasta, table;
    if (trc == RTX_OK) trc = format_two_pass(fasta, [&](char *buf, uint64_t cap) { return rtx_tally_format_fasta(sum, o.uniques_minsize, buf, cap); });
    if (trc == RTX_OK && p.tags_on) trc = format_two_pass(table, [&](char *buf, uint64_t cap) { return rtx_tally_format_table(sum, names.data(), o.uniques_minsize, buf, cap); });
    if (trc != RTX_OK) { fprintf(stderr, "[ERROR] distinct reads: %s\n", rtx_last_error()); return 70; }
    fprintf(stderr, "[INFO ] --uniques: %llu reads, %llu distinct\n", (ull)view.totals[0], (ull)view.totals[1]);
    if (view.totals[2])
        fprintf(stderr, "[INFO ] --uniques: %llu of %llu reads belong to sequences beyond the caps (--uniques-max-entries, --uniques-max-bytes) and are in no entry\n",
                (ull)view.totals[2], (ull)view.totals[0]);
    if (!write_whole(o.prefix + "/raxtax.uniques", fasta)) return 74;
    if (p.tags_on && !write_whole(o.prefix + "/raxtax.uniques.tsv", table)) return 74;
    if (o.otus) {
        rtx_otu *&otu = own.otu;
        rtx_otu_view_t ov{};
        std::string otu_fasta, otu_map, otu_table;
        // under --unoise the object is the denoiser's: everything below runs on it as on any other, under the larger of the two minsizes
        const uint64_t otus_minsize = o.unoise ? std::max(o.otus_minsize, o.unoise_params.minsize) : o.otus_minsize;
        rtx_unoise_view_t uv{};
        std::string unoise_text;
        trc = o.unoise ? rtx_otu_unoise(o.devices[0], sum, &o.unoise_params, &otu) : rtx_otu_cluster(o.devices[0], sum, nullptr, &otu);
        if (trc == RTX_OK) trc = rtx_otu_view(otu, &ov);
        if (trc == RTX_OK && o.unoise) trc = rtx_otu_unoise_view(otu, &uv);
        if (trc == RTX_OK && o.unoise) trc = format_two_pass(unoise_text, [&](char *buf, uint64_t cap) { return rtx_otu_format_unoise(otu, buf, cap); });
        rtx_graft_view_t gv{};
        std::string grafts;
        if (trc == RTX_OK && o.fastidious) {  // the small OTUs onto the large ones: everything below is written of the grafted object (ov keeps the numbers of the clustering)
            rtx_otu *grafted = nullptr;
            const rtx_graft_params gp{o.fastidious_boundary, 0, 0, 0, 0};
            trc = rtx_otu_graft(o.devices[0], sum, otu, &gp, &grafted);
            if (trc == RTX_OK) {
                rtx_otu_destroy(otu);
                otu = grafted;
                trc = rtx_otu_graft_view(otu, &gv);
            }
            if (trc == RTX_OK) trc = format_two_pass(grafts, [&](char *buf, uint64_t cap) { return rtx_otu_format_grafts(otu, buf, cap); });
        }
        if (trc == RTX_OK) trc = format_two_pass(otu_fasta, [&](char *buf, uint64_t cap) { return rtx_otu_format_fasta(otu, sum, otus_minsize, buf, cap); });
        if (trc == RTX_OK) trc = format_two_pass(otu_map, [&](char *buf, uint64_t cap) { return rtx_otu_format_map(otu, buf, cap); });
        if (trc == RTX_OK && p.tags_on) trc = format_two_pass(otu_table, [&](char *buf, uint64_t cap) { return rtx_otu_format_table(otu, names.data(), otus_minsize, buf, cap); });
        if (trc != RTX_OK) { fprintf(stderr, "[ERROR] OTUs: %s\n", rtx_last_error()); return 70; }
        if (o.unoise)
            fprintf(stderr, "[INFO ] --unoise: %llu distinct reads, %llu ZOTUs, %llu absorbed, %llu left, %llu long, %u tiers\n", (ull)ov.n_rows, (ull)uv.n_zotu, (ull)uv.n_absorbed,
                    (ull)uv.n_left, (ull)uv.n_long, uv.tiers);
        else
            fprintf(stderr, "[INFO ] --otus: %llu distinct reads, %llu links, %llu OTUs, %u rounds\n", (ull)ov.n_rows, (ull)ov.n_links, (ull)ov.n_otus, ov.rounds);
        if (ov.long_rows) fprintf(stderr, "[INFO ] --otus: %llu distinct reads are longer than %d bases and stand alone\n", (ull)ov.long_rows, RTX_OTU_MAX_LEN);
        if (!write_whole(o.prefix + "/raxtax.otus", otu_fasta) || !write_whole(o.prefix + "/raxtax.otus.map", otu_map)) return 74;
        if (p.tags_on && !write_whole(o.prefix + "/raxtax.otus.tsv", otu_table)) return 74;
        if (o.unoise && !write_whole(o.prefix + "/raxtax.otus.unoise", unoise_text)) return 74;
        if (o.fastidious) {
            fprintf(stderr, "[INFO ] --fastidious: boundary %llu, %llu heavy and %llu light OTUs, %llu grafts, %llu OTUs left\n", (ull)gv.boundary, (ull)gv.heavy_otus, (ull)gv.light_otus,
                    (ull)gv.n_grafts, (ull)gv.n_otus);
            if (!write_whole(o.prefix + "/raxtax.otus.grafts", grafts)) return 74;
        }
        if (o.otus_tax_cutoff) {  // which taxon every OTU is (of the grafted OTUs under --fastidious)
            rtx_otu_view_t cur{};
            if (rtx_otu_view(otu, &cur) != RTX_OK) { fprintf(stderr, "[ERROR] OTU taxonomy: %s\n", rtx_last_error()); return 70; }
            if (const int wrc = write_otu_taxonomy(o, first, tree, view, cur, otus_minsize)) return wrc;
        }
        if (o.denovo) {  // the OTUs against the more abundant OTUs of the run
            rtx_denovo *&dn = own.dn;
            rtx_denovo_view_t dv{};
            std::string records, clean, clean_table;
            trc = rtx_denovo_check(o.devices[0], sum, otu, &o.denovo_params, &dn);
            if (trc == RTX_OK) trc = rtx_denovo_view(dn, &dv);
            if (trc == RTX_OK) trc = format_two_pass(records, [&](char *buf, uint64_t cap) { return rtx_denovo_format_records(dn, buf, cap); });
            if (trc == RTX_OK) trc = format_two_pass(clean, [&](char *buf, uint64_t cap) { return rtx_denovo_format_fasta(dn, sum, otu, otus_minsize, buf, cap); });
            if (trc == RTX_OK && p.tags_on)
                trc = format_two_pass(clean_table, [&](char *buf, uint64_t cap) { return rtx_denovo_format_table(dn, sum, otu, names.data(), otus_minsize, buf, cap); });
            if (trc != RTX_OK) { fprintf(stderr, "[ERROR] de novo chimera check: %s\n", rtx_last_error()); return 70; }
            fprintf(stderr, "[INFO ] --denovo: %llu OTUs, %llu checked, %llu flagged, %u rounds\n", (ull)dv.n_entries, (ull)dv.n_checked, (ull)dv.n_flagged, dv.rounds);
            if (!write_whole(o.prefix + "/raxtax.otus.denovo", records) || !write_whole(o.prefix + "/raxtax.otus.clean", clean)) return 74;
            if (p.tags_on && !write_whole(o.prefix + "/raxtax.otus.clean.tsv", clean_table)) return 74;
        }
    }
    return 0;
}

}  // namespace

// The stages of a run, in order
int main(int argc, char **argv) {
    Laps laps;
    Options o;
    Plan plan;
    if (const int rc = parse_args(argc, argv, o)) return rc;
    if (const int rc = validate(o, plan)) return rc;
    Sink sink;
    const std::vector<Report> reports = report_table(o, plan, sink);

    std::set<std::string> done;
    bool resume = false;
    if (const int rc = resume_or_start(o, plan, reports, done, resume)) return rc;

    rtx_tree *tree = nullptr;
    std::string db_bin;
    if (const int rc = load_database(o, resume, laps, tree, db_bin)) return rc;
    sink.tree = tree;
    {
        const std::string ckp_json = o.prefix + "/raxtax.json", tmp = ckp_json + ".tmp";  // Checkpoint::save: tmp + rename (io.rs:72-78)
        std::ofstream f(tmp, std::ios::trunc);
        f << plan.identity.json();
        f.close();
        rename(tmp.c_str(), ckp_json.c_str());
    }
    BinWriter bin;
    if (o.only_db) {
        bin.start(tree, db_bin);
        const bool ok = bin.join();
        laps.lap("database_cache");
        if (o.timing) fprintf(stderr, "{%s}\n", laps.log.str().c_str());
        return ok ? 0 : 74;
    }

    std::vector<const char *> skip;
    for (const std::string &l : done) skip.push_back(l.c_str());
    BlockQueue queue;
    std::thread reader([&]() {
        if (plan.merge_on) read_paired(o, skip, queue);
        else read_single(o, plan.fastq, skip, queue);
    });

    std::vector<rtx_index *> indices(o.devices.size(), nullptr);
    std::vector<rtx_tally *> tallies(o.uniques ? o.devices.size() : 0, nullptr);
    if (!create_handles(o, plan, tree, indices, tallies)) {
        queue.stop_and_join(reader);
        return 71;  // exitcode::OSERR
    }
    rtx_screen_set_free(plan.contam_set);  // (the handles keep what they need)
    plan.contam_set = nullptr;
    laps.lap("index");
    if (o.timing) {  // the handle's own verdict on tile pruning (rtx_index_self_sample: a property of the database)
        int on = 1;
        double share = -1.0;
        if (rtx_index_prune_verdict(indices[0], &on, &share) == RTX_OK && share >= 0.0)
            fprintf(stderr, "[TIMING] tile pruning %s: a sample of the database's own references keeps %.1f %% of its tiles live\n", on ? "on" : "off", 100.0 * share);
    }
    bin.start(tree, db_bin);  // after the index: rtx_index_create_from_tree looks at the tree's k-mer map

    open_reports(o, plan, reports, sink, o.redo || !resume);

    Totals tot[N_STAGES];
    const bool stage_on[N_STAGES] = {plan.screen_on, plan.tags_on, !plan.primers.empty(), plan.qual_on, o.chim_on, o.derep, plan.merge_on};
    for (int s = 0; s < N_STAGES; s++) tot[s].on = stage_on[s];
    uint64_t n = 0;
    bool parse_failed = false;
    const int rc = classify_blocks(o, plan, queue, indices, tree, sink, tot, n, parse_failed);
    queue.stop_and_join(reader);
    sink.out.flush();
    sink.ckp.flush();
    if (o.tsv) sink.tsv.flush();
    for (const Report &r : reports)
        if (r.on) r.stream->flush();
    if (parse_failed) { bin.join(); return 66; }
    laps.lap("classify_and_write");

    print_totals(o, tot, laps);
    if (!bin.join()) return 74;
    laps.lap("database_cache_wait");
    if (o.timing) fprintf(stderr, "{\"n_queries\": %llu, %s}\n", (ull)n, laps.log.str().c_str());
    if (rc != RTX_OK) {
        fprintf(stderr, "[ERROR] %s\nRerun raxtax-hip to continue from the last checkpoint.\n", rtx_last_error());
        return rc == RTX_ERR_SENDER ? 75 : 70;  // exitcode::TEMPFAIL / SOFTWARE
    }

    if (o.profile_cutoff)
        if (const int wrc = write_profile(o, indices, tree)) return wrc;
    if (o.profile_cutoff && plan.tags_on)
        if (const int wrc = write_sample_table(o, plan, indices, tree)) return wrc;
    // (behind the two profile files, and it must stay there: under --otus-tax the second pass ends the first handle's profile, so that the rows it
    //  classifies once more are not counted as reads of the run)
    if (o.uniques)
        if (const int wrc = write_uniques_and_otus(o, plan, tallies, indices[0], tree)) return wrc;

    if (o.clean) {  // Checkpoint::cleanup (io.rs:80-89)
        remove((o.prefix + "/raxtax.json").c_str());
        remove((o.prefix + "/raxtax.ckp").c_str());
        if (!db_bin.empty()) remove(db_bin.c_str());
    }
    for (rtx_index *ix : indices) rtx_index_destroy(ix);
    for (rtx_tally *t : tallies) rtx_tally_destroy(t);
    rtx_tree_destroy(tree);
    return 0;
}

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
#include <sys/stat.h>
#include <zlib.h>

#include <cctype>
#include <chrono>
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

bool slurp(const std::string &path, std::string &out) {
    Input in;
    if (!in.open(path)) return false;
    out.clear();
    const size_t piece = (size_t)16 << 20;
    for (;;) {
        const size_t have = out.size();
        out.resize(have + piece);
        const size_t got = in.read(&out[have], piece);
        if (got == (size_t)-1) { in.close(); return false; }
        out.resize(have + got);
        if (got < piece) break;
    }
    in.close();
    return true;
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

// (--strand both is part of the checkpoint like the three flags: a rerun with the other setting starts over; a default run writes the file it always wrote)
// (... and so is --hits, and the cutoff of --profile in hundredths: 0 without the option)
// (... and --primers with its two settings, as given: trimmed reads are other reads)
std::string checkpoint_json(const std::string &fp, bool raw, bool skip, bool tsv, bool both, bool hits, uint32_t profile = 0, bool identity = false,
                            const std::string &primers = std::string(), const std::string &quality = std::string(), const std::string &merge = std::string(),
                            const std::string &chimera = std::string(), const std::string &tags = std::string(), const std::string &contaminants = std::string(),
                            const std::string &uniques = std::string(), const std::string &otus = std::string()) {
    std::ostringstream ss;
    ss << "{\n  \"db_fingerprint\": \"" << fp << "\",\n  \"raw_confidence\": " << (raw ? "true" : "false")
       << ",\n  \"skip_exact_matches\": " << (skip ? "true" : "false") << ",\n  \"tsv\": " << (tsv ? "true" : "false")
       << (both ? ",\n  \"strand\": \"both\"" : "") << (hits ? ",\n  \"hits\": true" : "") << (identity ? ",\n  \"identity\": true" : "");
    if (profile) ss << ",\n  \"profile\": " << profile;
    if (!primers.empty()) ss << ",\n  \"primers\": \"" << primers << "\"";
    if (!quality.empty()) ss << ",\n  \"quality\": \"" << quality << "\"";  // (... and the quality filter's settings, as given)
    if (!merge.empty()) ss << ",\n  \"merge\": \"" << merge << "\"";  // (... and --reverse with the merge settings: merged reads are other reads)
    if (!chimera.empty()) ss << ",\n  \"chimera\": \"" << chimera << "\"";  // (... and --chimera with its two settings: flagged reads have no lines)
    if (!tags.empty()) ss << ",\n  \"tags\": \"" << tags << "\"";  // (... and --tags with its settings: demultiplexed reads are other reads)
    if (!contaminants.empty()) ss << ",\n  \"contaminants\": \"" << contaminants << "\"";  // (... and --contaminants with its settings and the set's fingerprint: contaminants have no lines)
    if (!uniques.empty()) ss << ",\n  \"uniques\": \"" << uniques << "\"";  // (... and --uniques with its settings: the table is the run's, a resumed run would miss reads)
    if (!otus.empty()) ss << ",\n  \"otus\": \"" << otus << "\"";  // (... and --otus with its setting: its files are the run's)
    ss << "\n}\n";
    return ss.str();
}

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

// parser.rs:11-34 for an oligo on the command line; 0 where the character is no IUPAC code
uint8_t iupac_code(char ch) {
    switch (toupper((unsigned char)ch)) {
        case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
        case 'W': return 9; case 'S': return 6; case 'M': return 3; case 'K': return 12; case 'R': return 5; case 'Y': return 10;
        case 'B': return 14; case 'D': return 13; case 'H': return 11; case 'V': return 7; case 'N': return 15;
        default: return 0;
    }
}

struct Sink {
    std::ofstream out, tsv, ckp, strand, hits, trim, qc, merge, chimera, demux, screen;
    bool want_qc = false;                                    // the quality filter is on (raxtax.qc); its callback also serves --contaminants:
    uint32_t screen_len = 0;                                 // the length of the range the screen was given, of the query whose callbacks are running
    const std::vector<std::string> *contam_names = nullptr;  // --contaminants: the records of the file (raxtax.screen)
    const std::vector<std::string> *sample_names = nullptr;  // --tags: the samples of the sheet (raxtax.demux)
    bool want_tsv = false, want_strand = false, want_hits = false;
    const rtx_tree *tree = nullptr;  // the lineage of the nearest reference (raxtax.hits)
};

}  // namespace

int main(int argc, char **argv) {
    std::string db, qf, prefix = "raxtax";
    bool skip_exact = false, raw = false, tsv = false, only_db = false, skip_db = false, clean = false, redo = false;
    bool timing = false;
    using clk = std::chrono::steady_clock;
    auto t_prev = clk::now();
    std::ostringstream t_log;
    auto lap = [&](const char *what) {  // --timing: seconds per stage on stderr
        const auto now = clk::now();
        t_log << (t_log.tellp() > 0 ? ", " : "") << '"' << what << "\": " << std::chrono::duration<double>(now - t_prev).count();
        t_prev = now;
    };
    std::vector<int> devices{0};
    bool device_format = false;
    bool both_strands = false;  // --strand both: RTX_OPT_STRAND on every handle
    bool want_hits = false;     // --hits: RTX_OPT_NEAREST on every handle, PREFIX/raxtax.hits
    bool want_identity = false; // --identity: RTX_OPT_IDENTITY on every handle, dist and identity at the end of every line of raxtax.hits (implies --hits)
    bool derep = false;         // --derep: RTX_OPT_DEREP on every handle (each distinct read of a chunk is classified once; the files are the same)
    std::vector<std::pair<std::string, std::string>> primer_pairs;  // --primers FWD:REV (once or twice): rtx_index_set_primers on every handle, PREFIX/raxtax.trim
    uint32_t primer_pct = 10, primer_window = 0;                   // --primer-errors PCT, --primer-window N
    rtx_qual_params qual{33u, 0u, -1, -1.0, 0u, 0u, -1, -1.0, -1.0};  // --fastq-ascii and the filter options: rtx_index_set_quality on every handle, PREFIX/raxtax.qc
    std::string qual_spec;                                             // the filter options as given (empty: none) -- part of the checkpoint
    std::string rev_file;                                              // --reverse FILE: the reverse mates of the pairs of -i, merged on the device (rtx_merge_queries), PREFIX/raxtax.merge
    rtx_merge_params merge{33u, 16u, 10u, 100u, 41u};                  // --merge-minovlen, --merge-maxdiffs, --merge-maxdiffpct, --merge-qcap (ascii_base: --fastq-ascii)
    std::string merge_opts;                                            // the merge options as given (empty: none)
    bool chim_on = false;                                              // --chimera: rtx_index_set_chimera on every handle, PREFIX/raxtax.chimera
    rtx_chimera_params chim{RTX_CHIMERA_DEFAULT_SEGMENTS, RTX_CHIMERA_DEFAULT_MINDELTA};  // --chimera-segments, --chimera-mindelta
    std::string chim_opts;                                             // those two as given (empty: none)
    std::string contam_file;                                           // --contaminants FILE: rtx_index_set_screen on every handle, PREFIX/raxtax.screen
    rtx_screen_params contam{2u, 50u};                                 // --contam-minhits N, --contam-minpct P
    std::string contam_opts;                                           // those two as given (empty: none)
    std::string tags_file;                                             // --tags SHEET: rtx_index_set_tags on every handle, PREFIX/raxtax.demux (and raxtax.samples with --profile)
    rtx_demux_params tag_params{0u, 0u};                               // --tag-mismatches N, --tag-offset N
    bool tags_both = false;                                            // --tags-both-orientations
    std::string tag_opts;                                              // those three as given (empty: none)
    bool uniques = false;         // --uniques: a tally (rtx_tally.hip) on every handle, PREFIX/raxtax.uniques (and raxtax.uniques.tsv with --tags)
    uint64_t uniques_minsize = 1, uniques_max_entries = 0, uniques_max_bytes = 0;  // --uniques-minsize N, --uniques-max-entries N, --uniques-max-bytes N (0: the library's defaults)
    std::string uniques_opts;     // those three as given (empty: none)
    bool otus = false;            // --otus: the table of --uniques clustered into OTUs (rtx_otu.hip), PREFIX/raxtax.otus, raxtax.otus.map (and raxtax.otus.tsv with --tags)
    uint64_t otus_minsize = 1;    // --otus-minsize N
    bool otus_minsize_given = false;
    uint32_t profile_cutoff = 0;  // --profile CUTOFF, in hundredths (0: no profile): a taxon profile open on every handle, PREFIX/raxtax.profile
    size_t chunk = 0;  // --batch: queries per chunk of rtx_raxtax; 0 = chosen per block of the query file (below)
    size_t block_bytes = (size_t)256 << 20;  // query file read and parsed in blocks of this size
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "-d" || a == "--database-path") db = val();
        else if (a == "-i" || a == "--query-file") qf = val();
        else if (a == "-o" || a == "--prefix") prefix = val();
        else if (a == "--skip-exact-matches") skip_exact = true;
        else if (a == "--raw-confidence") raw = true;
        else if (a == "--tsv") tsv = true;
        else if (a == "--only-db") only_db = true;
        else if (a == "--skip-db") skip_db = true;
        else if (a == "-c" || a == "--clean") clean = true;
        else if (a == "--redo") redo = true;
        else if (a == "--timing") timing = true;
        else if (a == "--device-format") device_format = true;  // RTX_OPT_DEVICE_TEXT on every handle: the lines are formatted on the GPU
        // CPU tuning flags of the reference (io.rs:139-153): accepted so that existing command lines keep working,
        // without effect on the device path.  -t takes a value; clap also accepts -tN, --threads=N, -vv, -qq.
        else if (a == "-t" || a == "--threads") (void)val();
        else if (a.rfind("--threads=", 0) == 0 || (a.size() > 2 && a[0] == '-' && a[1] == 't' && isdigit((unsigned char)a[2]))) {}
        else if (a == "--pin") {}
        else if (a == "--verbose" || a == "--quiet" || (a.size() >= 2 && a[0] == '-' && a[1] != '-' &&
                                                        a.find_first_not_of(a[1] == 'v' ? "v" : "q", 1) == std::string::npos &&
                                                        (a[1] == 'v' || a[1] == 'q'))) {}
        else if (a == "--device") devices.assign(1, atoi(val()));
        else if (a == "--gpus") {  // devices 0 .. N-1
            const int n = atoi(val());
            devices.clear();
            for (int d = 0; d < n; d++) devices.push_back(d);
        } else if (a == "--devices") {  // an explicit list; a device may be named twice (two handles on one GPU)
            devices.clear();
            std::stringstream ss(val());
            std::string tok;
            while (std::getline(ss, tok, ',')) if (!tok.empty()) devices.push_back(atoi(tok.c_str()));
        }
        else if (a == "--strand") {
            const std::string v = val();
            if (v != "plus" && v != "both") { fprintf(stderr, "raxtax-hip: --strand takes plus or both\n"); return 64; }
            both_strands = v == "both";
        }
        else if (a == "--hits") want_hits = true;
        else if (a == "--identity") want_identity = want_hits = true;
        else if (a == "--derep") derep = true;
        else if (a == "--primers") {
            const std::string v = val();
            const size_t colon = v.find(':');
            if (colon == std::string::npos || v.find(':', colon + 1) != std::string::npos || v.size() < 2) {
                fprintf(stderr, "raxtax-hip: --primers takes FWD:REV (either side may be empty), not '%s'\n", v.c_str());
                return 64;
            }
            primer_pairs.emplace_back(v.substr(0, colon), v.substr(colon + 1));
        }
        else if (a == "--primer-errors") {
            const int x = atoi(val());
            if (x < 0 || x > 99) { fprintf(stderr, "raxtax-hip: --primer-errors takes a percentage, 0 .. 99\n"); return 64; }
            primer_pct = (uint32_t)x;
        }
        else if (a == "--primer-window") {
            const int x = atoi(val());
            if (x < 1 || x > RTX_TRIM_MAX_WINDOW) { fprintf(stderr, "raxtax-hip: --primer-window takes 1 .. %d bases\n", RTX_TRIM_MAX_WINDOW); return 64; }
            primer_window = (uint32_t)x;
        }
        else if (a == "--fastq-ascii") {
            const std::string v = val();
            if (v != "33" && v != "64") { fprintf(stderr, "raxtax-hip: --fastq-ascii takes 33 or 64, not '%s'\n", v.c_str()); return 64; }
            qual.ascii_base = (uint32_t)atoi(v.c_str());
        }
        else if (a == "--trunclen" || a == "--minlen" || a == "--maxlen" || a == "--maxns" || a == "--truncq") {
            char *end = nullptr;
            const char *v = val();
            const long x = strtol(v, &end, 10);
            const long least = a == "--maxns" || a == "--truncq" ? 0 : 1, most = a == "--truncq" ? 93 : (long)RTX_QUAL_MAX_READ;
            if (end == v || *end != 0 || x < least || x > most) { fprintf(stderr, "raxtax-hip: %s takes a whole number, %ld .. %ld, not '%s'\n", a.c_str(), least, most, v); return 64; }
            if (a == "--trunclen") qual.trunc_len = (uint32_t)x;
            else if (a == "--minlen") qual.min_len = (uint32_t)x;
            else if (a == "--maxlen") qual.max_len = (uint32_t)x;
            else if (a == "--maxns") qual.max_ns = (int32_t)x;
            else qual.trunc_qual = (int32_t)x;
            qual_spec += (qual_spec.empty() ? "" : ";") + a.substr(2) + "=" + v;
        }
        else if (a == "--truncee" || a == "--maxee" || a == "--maxee-rate") {
            char *end = nullptr;
            const char *v = val();
            const double x = strtod(v, &end);
            if (end == v || *end != 0 || !(x >= 0.0)) { fprintf(stderr, "raxtax-hip: %s takes a number that is not negative, not '%s'\n", a.c_str(), v); return 64; }
            (a == "--truncee" ? qual.trunc_ee : a == "--maxee" ? qual.max_ee : qual.max_ee_rate) = x;
            qual_spec += (qual_spec.empty() ? "" : ";") + a.substr(2) + "=" + v;
        }
        else if (a == "-r" || a == "--reverse") rev_file = val();
        else if (a == "--merge-minovlen" || a == "--merge-maxdiffs" || a == "--merge-maxdiffpct" || a == "--merge-qcap") {
            const char *v = val();
            char *end = nullptr;
            const long x = strtol(v, &end, 10);
            const long least = a == "--merge-minovlen" ? 1 : 0, most = a == "--merge-maxdiffpct" ? 100 : (a == "--merge-qcap" ? 93 : (long)RTX_MERGE_MAX_READ);
            if (end == v || *end != 0 || x < least || x > most) { fprintf(stderr, "raxtax-hip: %s takes a whole number, %ld .. %ld, not '%s'\n", a.c_str(), least, most, v); return 64; }
            (a == "--merge-minovlen" ? merge.min_overlap : a == "--merge-maxdiffs" ? merge.max_diffs : a == "--merge-maxdiffpct" ? merge.max_diff_pct : merge.q_cap) = (uint32_t)x;
            merge_opts += (merge_opts.empty() ? "" : " ") + a;
        }
        else if (a == "--chimera") chim_on = true;
        else if (a == "--chimera-mindelta" || a == "--chimera-segments") {
            const char *v = val();
            char *end = nullptr;
            const long x = strtol(v, &end, 10);
            const long least = a == "--chimera-segments" ? 2 : 0, most = a == "--chimera-segments" ? (long)RTX_CHIMERA_MAX_SEGMENTS : (long)RTX_CHIMERA_MAX_QUERY;
            if (end == v || *end != 0 || x < least || x > most) { fprintf(stderr, "raxtax-hip: %s takes a whole number, %ld .. %ld, not '%s'\n", a.c_str(), least, most, v); return 64; }
            (a == "--chimera-segments" ? chim.segments : chim.mindelta) = (uint32_t)x;
            chim_opts += (chim_opts.empty() ? "" : " ") + a;
        }
        else if (a == "--contaminants") contam_file = val();
        else if (a == "--contam-minhits" || a == "--contam-minpct") {
            const char *v = val();
            char *end = nullptr;
            const long x = strtol(v, &end, 10);
            const long least = a == "--contam-minhits" ? 1 : 0, most = a == "--contam-minhits" ? 0x7FFFFFFFl : 100;
            if (end == v || *end != 0 || x < least || x > most) { fprintf(stderr, "raxtax-hip: %s takes a whole number, %ld .. %ld, not '%s'\n", a.c_str(), least, most, v); return 64; }
            (a == "--contam-minhits" ? contam.min_hits : contam.min_pct) = (uint32_t)x;
            contam_opts += (contam_opts.empty() ? "" : " ") + a;
        }
        else if (a == "--tags") tags_file = val();
        else if (a == "--tags-both-orientations") { tags_both = true; tag_opts += (tag_opts.empty() ? "" : " ") + a; }
        else if (a == "--tag-mismatches" || a == "--tag-offset") {
            const char *v = val();
            char *end = nullptr;
            const long x = strtol(v, &end, 10);
            const long most = a == "--tag-mismatches" ? (long)RTX_DEMUX_MAX_MISMATCHES : (long)RTX_DEMUX_MAX_OFFSET;
            if (end == v || *end != 0 || x < 0 || x > most) { fprintf(stderr, "raxtax-hip: %s takes a whole number, 0 .. %ld, not '%s'\n", a.c_str(), most, v); return 64; }
            (a == "--tag-mismatches" ? tag_params.max_mismatches : tag_params.max_offset) = (uint32_t)x;
            tag_opts += (tag_opts.empty() ? "" : " ") + a;
        }
        else if (a == "--profile") {
            char *end = nullptr;
            const char *v = val();
            const double x = strtod(v, &end);
            const long c = end != v && *end == '\0' && x > 0.0 && x <= 1.0 ? lround(x * 100.0) : 0;
            if (c < 1 || c > 100) { fprintf(stderr, "raxtax-hip: --profile takes a confidence cutoff in (0, 1], such as 0.8\n"); return 64; }
            profile_cutoff = (uint32_t)c;
        }
        else if (a == "--uniques") uniques = true;
        else if (a == "--uniques-minsize" || a == "--uniques-max-entries" || a == "--uniques-max-bytes") {
            char *end = nullptr;
            const char *v = val();
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end != '\0' || x < 1 || (a == "--uniques-max-entries" && x > 0x7FFFFFFELL)) { fprintf(stderr, "raxtax-hip: %s takes a positive integer\n", a.c_str()); return 64; }
            (a == "--uniques-minsize" ? uniques_minsize : a == "--uniques-max-entries" ? uniques_max_entries : uniques_max_bytes) = (uint64_t)x;
            uniques_opts += (uniques_opts.empty() ? "" : " ") + a;
        }
        else if (a == "--otus") otus = true;
        else if (a == "--otus-minsize") {
            char *end = nullptr;
            const char *v = val();
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end != '\0' || x < 1) { fprintf(stderr, "raxtax-hip: --otus-minsize takes a positive integer\n"); return 64; }
            otus_minsize = (uint64_t)x;
            otus_minsize_given = true;
        }
        else if (a == "--batch") chunk = (size_t)atoll(val());
        else if (a == "--block-bytes") block_bytes = std::max<size_t>(1, (size_t)atoll(val()));
        else {
            fprintf(stderr, "usage: raxtax-hip -d DB.(fasta|bin) [-i QUERIES.(fasta|fastq)] [-o PREFIX] [--skip-exact-matches] [--raw-confidence] "
                            "[--tsv] [--only-db] [--skip-db] [-c] [--redo] [--device N | --gpus N | --devices a,b,..] [--batch N] [--block-bytes N] [--device-format] [--strand plus|both] [--hits] [--identity] [--profile CUTOFF] [--derep] [--primers FWD:REV [--primer-errors PCT] [--primer-window N]] [--fastq-ascii 33|64] [--trunclen N] [--truncq Q] [--truncee E] [--minlen N] [--maxlen N] [--maxns N] [--maxee E] [--maxee-rate R] [--reverse R2.fastq [--merge-minovlen N] [--merge-maxdiffs N] [--merge-maxdiffpct N] [--merge-qcap N]] [--chimera [--chimera-mindelta N] [--chimera-segments S]] [--tags SHEET [--tag-mismatches N] [--tag-offset N] [--tags-both-orientations]] [--contaminants FILE [--contam-minhits N] [--contam-minpct P]] [--uniques [--uniques-minsize N] [--uniques-max-entries N] [--uniques-max-bytes N] [--otus [--otus-minsize N]]]\n"
                            "       (-t/--threads N, --pin, -v, -q of the reference are accepted and ignored)\n");
            return 64;
        }
    }
    if (devices.empty()) { fprintf(stderr, "raxtax-hip: --gpus / --devices need at least one device\n"); return 64; }
    if (db.empty() || (qf.empty() && !only_db) || (only_db && skip_db)) {
        fprintf(stderr, "raxtax-hip: -d is required, -i unless --only-db; --only-db conflicts with --skip-db\n");
        return 64;
    }
    // FASTQ or FASTA: the first non-blank byte of the query file.  A filter option needs quality strings: refused here, before the database is read
    bool fastq = false;
    if (!qf.empty()) {
        Input f;
        if (f.open(qf)) {
            char c = 0;
            while (f.read(&c, 1) == 1 && isspace((unsigned char)c)) c = 0;
            fastq = c == '@';
            f.close();
        }
    }
    const bool qual_on = !qual_spec.empty();
    if (qual_on && !fastq) {
        fprintf(stderr, "raxtax-hip: the quality filter (%s) needs FASTQ input: %s does not start with '@'\n", qual_spec.c_str(), qf.empty() ? "-i" : qf.c_str());
        return 64;
    }
    if (qual_on) qual_spec += ";ascii=" + std::to_string(qual.ascii_base);
    // --reverse: paired input, merged before anything else.  Refused here as well -- before the database is read -- where it cannot work
    const bool merge_on = !rev_file.empty();
    if (!merge_opts.empty() && !merge_on) {
        fprintf(stderr, "raxtax-hip: %s sets how pairs are merged and needs --reverse FILE (the reverse mates)\n", merge_opts.c_str());
        return 64;
    }
    if (merge_on && !fastq) {
        fprintf(stderr, "raxtax-hip: --reverse needs FASTQ input: %s does not start with '@'\n", qf.empty() ? "-i" : qf.c_str());
        return 64;
    }
    // --chimera: refused here as well where it cannot work
    if (!chim_opts.empty() && !chim_on) {
        fprintf(stderr, "raxtax-hip: %s sets how reads are checked for chimeras and needs --chimera\n", chim_opts.c_str());
        return 64;
    }
    if (chim_on && both_strands) {
        fprintf(stderr, "raxtax-hip: --chimera checks a read in the orientation given and cannot go with --strand both\n");
        return 64;
    }
    const std::string chim_spec = chim_on ? "segments=" + std::to_string(chim.segments) + ";mindelta=" + std::to_string(chim.mindelta) : std::string();
    std::string merge_spec;
    if (merge_on) {
        merge.ascii_base = qual.ascii_base;
        merge_spec = "reverse=" + rev_file + ";minovlen=" + std::to_string(merge.min_overlap) + ";maxdiffs=" + std::to_string(merge.max_diffs) + ";maxdiffpct=" +
                     std::to_string(merge.max_diff_pct) + ";qcap=" + std::to_string(merge.q_cap) + ";ascii=" + std::to_string(merge.ascii_base);
    }
    // --primers: the pattern list, checked here -- before the database is read and any device is touched
    struct Primer { std::string name; std::vector<uint8_t> codes; uint32_t end; };
    std::vector<Primer> primers;
    std::string primer_spec;
    for (const auto &pr : primer_pairs) {
        std::vector<uint8_t> fwd, rev;
        for (int side = 0; side < 2; side++) {
            const std::string &oligo = side ? pr.second : pr.first;
            for (char ch : oligo) {
                const uint8_t c = iupac_code(ch);
                if (!c) { fprintf(stderr, "raxtax-hip: --primers: '%c' in primer %s is no IUPAC code\n", ch, oligo.c_str()); return 64; }
                (side ? rev : fwd).push_back(c);
            }
            if (oligo.size() > RTX_TRIM_MAX_PATTERN) { fprintf(stderr, "raxtax-hip: --primers: primer %s has %zu bases (at most %d)\n", oligo.c_str(), oligo.size(), RTX_TRIM_MAX_PATTERN); return 64; }
        }
        auto rc_of = [](const std::vector<uint8_t> &x) { std::vector<uint8_t> y(x.size() + 1); (void)rtx_revcomp(x.data(), x.size(), y.data()); y.resize(x.size()); return y; };
        auto add = [&](const std::string &name, const std::vector<uint8_t> &codes, uint32_t end) {
            if (!codes.empty()) primers.push_back({name, codes, end});
        };
        add(pr.first, fwd, RTX_TRIM_5P);
        add("revcomp(" + pr.second + ")", rc_of(rev), RTX_TRIM_3P);
        if (both_strands) {
            add(pr.second, rev, RTX_TRIM_5P);
            add("revcomp(" + pr.first + ")", rc_of(fwd), RTX_TRIM_3P);
        }
        if (primers.size() > RTX_TRIM_MAX_PATTERNS) {
            fprintf(stderr, "raxtax-hip: --primers: %s:%s makes %zu patterns (at most %d%s)\n", pr.first.c_str(), pr.second.c_str(), primers.size(), RTX_TRIM_MAX_PATTERNS,
                    both_strands ? "; --strand both registers every oligo at both ends" : "");
            return 64;
        }
        primer_spec += (primer_spec.empty() ? "" : ",") + pr.first + ":" + pr.second;
    }
    if (!primer_spec.empty()) primer_spec += ";errors=" + std::to_string(primer_pct) + ";window=" + std::to_string(primer_window);
    // --tags: the sample sheet, read and checked here as well
    struct Tag { std::string name; std::vector<uint8_t> codes; uint32_t end; };
    std::vector<Tag> tags;
    std::vector<rtx_demux_pair> tag_pairs;
    std::vector<std::string> sample_names;
    std::string tag_spec;
    const bool tags_on = !tags_file.empty();
    if (!tag_opts.empty() && !tags_on) { fprintf(stderr, "raxtax-hip: %s sets how reads are assigned to samples and needs --tags SHEET\n", tag_opts.c_str()); return 64; }
    if (tags_on) {
        if (derep && profile_cutoff) {
            fprintf(stderr, "raxtax-hip: --tags cannot go with --derep and --profile together: copies from different samples would be counted as one read\n");
            return 64;
        }
        std::string sheet;
        if (!slurp(tags_file, sheet)) { fprintf(stderr, "raxtax-hip: --tags: cannot read %s\n", tags_file.c_str()); return 66; }
        auto rc_of = [](const std::vector<uint8_t> &x) { std::vector<uint8_t> y(x.size() + 1); (void)rtx_revcomp(x.data(), x.size(), y.data()); y.resize(x.size()); return y; };
        auto strip = [](std::string s) {
            while (!s.empty() && isspace((unsigned char)s.back())) s.pop_back();
            size_t a = 0;
            while (a < s.size() && isspace((unsigned char)s[a])) a++;
            return s.substr(a);
        };
        auto tag_of = [&](const std::string &name, const std::vector<uint8_t> &codes, uint32_t end) -> uint32_t {  // a tag that several lines share is listed once
            for (size_t k = 0; k < tags.size(); k++)
                if (tags[k].end == end && tags[k].codes == codes) return (uint32_t)k;
            tags.push_back({name, codes, end});
            return (uint32_t)tags.size() - 1u;
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
            if (f.size() < 2 || f.size() > 3 || f[0].empty() || f[1].empty()) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: expected sample<TAB>fwd_tag<TAB>rev_tag\n", tags_file.c_str(), line_no); return 64; }
            std::vector<uint8_t> fwd, rev;
            const bool single = f.size() == 2 || f[2].empty() || f[2] == "-";
            for (int side = 0; side < (single ? 1 : 2); side++)
                for (char ch : f[1 + side]) {
                    const uint8_t c = iupac_code(ch);
                    if (!c) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: '%c' is no IUPAC code\n", tags_file.c_str(), line_no, ch); return 64; }
                    (side ? rev : fwd).push_back(c);
                }
            size_t s = 0;
            while (s < sample_names.size() && sample_names[s] != f[0]) s++;
            if (s == sample_names.size()) sample_names.push_back(f[0]);
            tag_pairs.push_back({tag_of(f[1], fwd, RTX_TRIM_5P), single ? RTX_DEMUX_NO_TAG : tag_of("revcomp(" + f[2] + ")", rc_of(rev), RTX_TRIM_3P), (uint32_t)s});
            if (tags_both) {
                if (single) { fprintf(stderr, "raxtax-hip: --tags: %s line %u: --tags-both-orientations needs a rev_tag\n", tags_file.c_str(), line_no); return 64; }
                tag_pairs.push_back({tag_of(f[2], rev, RTX_TRIM_5P), tag_of("revcomp(" + f[1] + ")", rc_of(fwd), RTX_TRIM_3P), (uint32_t)s});
            }
        }
        std::vector<rtx_demux_tag> ct;
        for (const Tag &t : tags) ct.push_back({t.codes.data(), (uint32_t)t.codes.size(), t.end});
        uint32_t x[5];  // the checks of the library on the list (rtx_demux_create makes them again): one read through the host function
        if (rtx_demux_read(&tag_params, ct.data(), (uint32_t)ct.size(), tag_pairs.data(), (uint32_t)tag_pairs.size(), nullptr, 0, &x[0], &x[1], &x[2], &x[3], &x[4]) != RTX_OK) {
            fprintf(stderr, "raxtax-hip: --tags: %s: %s\n", tags_file.c_str(), rtx_last_error());
            return 64;
        }
        tag_spec = fingerprint(tags_file) + ";mismatches=" + std::to_string(tag_params.max_mismatches) + ";offset=" + std::to_string(tag_params.max_offset) + ";both=" + (tags_both ? "1" : "0");
    }
    // --contaminants: the set, built here as well -- before the database is read and any device is touched
    const bool screen_on = !contam_file.empty();
    if (!contam_opts.empty() && !screen_on) { fprintf(stderr, "raxtax-hip: %s sets how reads are screened and needs --contaminants FILE\n", contam_opts.c_str()); return 64; }
    rtx_screen_set *contam_set = nullptr;
    std::vector<std::string> contam_names;
    std::string contam_spec;
    if (screen_on) {
        std::string text;
        if (!slurp(contam_file, text)) { fprintf(stderr, "raxtax-hip: --contaminants: cannot read %s\n", contam_file.c_str()); return 66; }
        rtx_queries *cq = nullptr;  // (the query parser: the labels need no lineage)
        if (rtx_queries_parse_fasta(text.data(), text.size(), nullptr, 0, &cq) != RTX_OK) { fprintf(stderr, "raxtax-hip: --contaminants: %s: %s\n", contam_file.c_str(), rtx_last_error()); return 66; }
        const uint8_t *cb = nullptr;
        const uint64_t *co = nullptr;
        rtx_queries_data(cq, &cb, &co);
        const uint64_t nc = rtx_queries_len(cq);
        for (uint64_t i = 0; i < nc; i++) {
            const std::string label = rtx_queries_label(cq, i);
            contam_names.push_back(label.substr(0, label.find_first_of(" \t")));
        }
        uint64_t keys = 0, slots = 0, fp = 0;
        const int brc = rtx_screen_set_build(nc, cb, co, &contam_set);
        rtx_queries_destroy(cq);
        if (brc != RTX_OK || rtx_screen_set_info(contam_set, &keys, &slots, nullptr, nullptr, &fp) != RTX_OK) {
            fprintf(stderr, "raxtax-hip: --contaminants: %s: %s\n", contam_file.c_str(), rtx_last_error());
            return 64;
        }
        char hex[24];
        snprintf(hex, sizeof hex, "%016llx", (unsigned long long)fp);
        contam_spec = "file=" + contam_file + ";minhits=" + std::to_string(contam.min_hits) + ";minpct=" + std::to_string(contam.min_pct) + ";keys=" + hex;
        fprintf(stderr, "[INFO ] --contaminants: %llu record(s) of %s, %llu distinct 16-mers in %llu slots; a read is a contaminant from %u hit(s) and %u %% of its windows on\n",
                (unsigned long long)nc, contam_file.c_str(), (unsigned long long)keys, (unsigned long long)slots, contam.min_hits, contam.min_pct);
    }
    const std::string demux_path = prefix + "/raxtax.demux", samples_path = prefix + "/raxtax.samples", screen_path = prefix + "/raxtax.screen";
    const std::string ckp_json = prefix + "/raxtax.json", ckp_path = prefix + "/raxtax.ckp", trim_path = prefix + "/raxtax.trim", qc_path = prefix + "/raxtax.qc", merge_path = prefix + "/raxtax.merge", chim_path = prefix + "/raxtax.chimera";
    const std::string out_path = prefix + "/raxtax.out", tsv_path = prefix + "/raxtax.tsv", strand_path = prefix + "/raxtax.strand", hits_path = prefix + "/raxtax.hits", profile_path = prefix + "/raxtax.profile";
    const std::string uniques_path = prefix + "/raxtax.uniques", uniques_table_path = prefix + "/raxtax.uniques.tsv";
    if (!uniques_opts.empty() && !uniques) { fprintf(stderr, "raxtax-hip: %s sets how the distinct reads are kept and written and needs --uniques\n", uniques_opts.c_str()); return 64; }
    const std::string otus_path = prefix + "/raxtax.otus", otus_map_path = prefix + "/raxtax.otus.map", otus_table_path = prefix + "/raxtax.otus.tsv";
    if (otus_minsize_given && !otus) { fprintf(stderr, "raxtax-hip: --otus-minsize sets what is written of the OTUs and needs --otus\n"); return 64; }
    if (otus && !uniques) { fprintf(stderr, "raxtax-hip: --otus clusters the distinct reads of the run and needs --uniques\n"); return 64; }
    const std::string otus_spec = otus ? "minsize=" + std::to_string(otus_minsize) : std::string();
    std::string uniques_spec;
    if (uniques) uniques_spec = "minsize=" + std::to_string(uniques_minsize) + " max_entries=" + std::to_string(uniques_max_entries) + " max_bytes=" + std::to_string(uniques_max_bytes);
    if (device_format && derep) {
        fprintf(stderr, "[INFO ] --derep: the result lines are formatted on the host (--device-format has no effect)\n");
        device_format = false;
    }
    if (device_format && both_strands) {
        fprintf(stderr, "[INFO ] --strand both: the result lines are formatted on the host (--device-format has no effect)\n");
        device_format = false;
    }
    // ---- checkpoint (io.rs:202-263)
    std::set<std::string> done;
    const std::string want_ckp = checkpoint_json(fingerprint(db), raw, skip_exact, tsv, both_strands, want_hits, profile_cutoff, want_identity, primer_spec, qual_spec, merge_spec, chim_spec, tag_spec, contam_spec, uniques_spec, otus_spec);
    bool resume = false;
    if (!redo && is_file(ckp_json)) {
        std::string have;
        slurp(ckp_json, have);
        if (have == want_ckp) {  // checkpoint_valid (io.rs:288-302)
            std::ifstream p(ckp_path);
            std::string l;
            while (std::getline(p, l)) done.insert(l);
            if (profile_cutoff && !done.empty()) {  // the queries of the earlier run are not classified again: their share of the sample is gone
                fprintf(stderr, "raxtax-hip: --profile cannot resume a checkpoint with processed queries (%zu in %s): the profile would miss them; "
                                "run with --redo to classify the whole sample again\n", done.size(), ckp_path.c_str());
                return 64;
            }
            if (uniques && !done.empty()) {  // (likewise: the table would miss the reads of the earlier run)
                fprintf(stderr, "raxtax-hip: --uniques cannot resume a checkpoint with processed queries (%zu in %s): the table would miss them; "
                                "run with --redo to classify the whole sample again\n", done.size(), ckp_path.c_str());
                return 64;
            }
            purge_incomplete(out_path, done);
            if (tsv) purge_incomplete(tsv_path, done);
            if (both_strands) purge_incomplete(strand_path, done);
            if (want_hits) purge_incomplete(hits_path, done);
            if (!primers.empty()) purge_incomplete(trim_path, done, true);
            if (qual_on) purge_incomplete(qc_path, done, true);
            if (merge_on) purge_incomplete(merge_path, done, true);
            if (chim_on) purge_incomplete(chim_path, done, true);
            if (tags_on) purge_incomplete(demux_path, done, true);
            if (screen_on) purge_incomplete(screen_path, done, true);
            resume = true;
            fprintf(stderr, "[INFO ] Restarting from checkpoint %s\n", ckp_json.c_str());
        }
    }
    if (is_dir(prefix) && !is_file(ckp_json) && !redo) {
        fprintf(stderr, "[ERROR] Output folder %s already exists! Please specify another folder with -o <PATH> or run with --redo "
                        "to force overriding existing files!\n", prefix.c_str());
        return 73;  // exitcode::CANTCREAT
    }
    mkdir(prefix.c_str(), 0777);

    // ---- database: try the binary format first, then FASTA (parser.rs:37-44)
    rtx_tree *tree = nullptr;
    bool store_db = false;
    if (rtx_tree_load_bin(db.c_str(), &tree) != RTX_OK) {
        std::string db_text;
        // Tree.k_mer_map is only needed for the .bin cache: the device index is built from the sequences
        if (!slurp(db, db_text) || rtx_tree_parse_reference_fasta_ex(db_text.data(), db_text.size(), RTX_TREE_SKIP_KMER_MAP, &tree) != RTX_OK) {
            fprintf(stderr, "[ERROR] Failed to parse %s: %s\n", db.c_str(), rtx_last_error());
            return 66;  // exitcode::NOINPUT
        }
        store_db = true;
    }
    lap("database");
    std::string db_bin;
    if (store_db && !skip_db) {  // main.rs:72-86, io.rs:269-286
        std::string base = db.substr(db.find_last_of('/') == std::string::npos ? 0 : db.find_last_of('/') + 1);
        const size_t dot = base.find_last_of('.');
        db_bin = prefix + "/" + (dot == std::string::npos ? base : base.substr(0, dot)) + ".bin";
        if (is_file(db_bin) && !redo && !resume) {
            fprintf(stderr, "[ERROR] Output database file %s already exists! Delete it or run with --redo\n", db_bin.c_str());
            return 73;
        }
    }
    // the database cache is written on a thread of its own while the queries are parsed and classified
    std::thread bin_writer;
    int bin_rc = RTX_OK;
    std::string bin_err;
    auto start_bin_writer = [&]() {
        if (db_bin.empty()) return;
        bin_writer = std::thread([&]() {
            bin_rc = rtx_tree_save_bin(tree, db_bin.c_str());
            if (bin_rc != RTX_OK) bin_err = rtx_last_error();
        });
    };
    auto join_bin_writer = [&]() -> bool {
        if (bin_writer.joinable()) bin_writer.join();
        if (bin_rc != RTX_OK) { fprintf(stderr, "[ERROR] Failed to write database: %s\n", bin_err.c_str()); return false; }
        return true;
    };
    {
        const std::string tmp = ckp_json + ".tmp";  // Checkpoint::save: tmp + rename (io.rs:72-78)
        std::ofstream f(tmp, std::ios::trunc);
        f << (resume ? want_ckp : checkpoint_json(fingerprint(db), raw, skip_exact, tsv, both_strands, want_hits, profile_cutoff, want_identity, primer_spec, qual_spec, merge_spec, chim_spec, tag_spec, contam_spec, uniques_spec, otus_spec));
        f.close();
        rename(tmp.c_str(), ckp_json.c_str());
    }
    if (only_db) {
        start_bin_writer();
        const bool ok = join_bin_writer();
        lap("database_cache");
        if (timing) fprintf(stderr, "{%s}\n", t_log.str().c_str());
        return ok ? 0 : 74;
    }

    // ---- queries: the file is read and parsed block by block on a thread of its own (cut in front of header lines,
    // rtx_fasta_block_end; FASTQ: behind whole records, rtx_fastq_block_end), so that ingest overlaps with classification and memory stays bounded for very large
    // files (the reference reads the whole file, parser.rs:112-115).  Already finished labels are dropped
    // (parser.rs:150-153).
    std::vector<const char *> skip;
    for (const std::string &l : done) skip.push_back(l.c_str());
    struct Parsed { rtx_queries *qs = nullptr; int rc = RTX_OK; std::string err; bool end = false; double merge_s[3] = {0, 0, 0}; float merge_ms = 0; };
    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<Parsed> ready;  // at most two blocks ahead
    bool stop_reader = false;
    std::thread reader([&]() {
        auto push = [&](Parsed &&pz) {
            std::unique_lock<std::mutex> g(qmu);
            qcv.wait(g, [&] { return ready.size() < 2 || stop_reader; });
            ready.push_back(std::move(pz));
            qcv.notify_all();
        };
        if (merge_on) {
            // Paired input: both files block by block, cut at the same record (rtx_fastq_block_end_n), parsed, and merged on the first device
            // of the run; what is queued is the handle of merged reads.  Nothing behind the queue knows.
            auto fail = [&](int rc, const std::string &msg) { Parsed e; e.rc = rc; e.err = msg; e.end = true; push(std::move(e)); };
            Input in[2];
            const std::string *name[2] = {&qf, &rev_file};
            if (!in[0].open(qf)) { fail(RTX_ERR_PARSE, "cannot open file"); return; }
            if (!in[1].open(rev_file)) { in[0].close(); fail(RTX_ERR_PARSE, "cannot open " + rev_file); return; }
            rtx_merge *stage = nullptr;
            if (const int mrc = rtx_merge_create(devices[0], &merge, &stage)) { fail(mrc, std::string("paired-end merging on device ") + std::to_string(devices[0]) + ": " + rtx_last_error()); in[0].close(); in[1].close(); return; }
            std::string buf[2];
            bool eof[2] = {false, false};
            uint64_t records = 0;  // pairs handed on so far
            bool force = false;
            for (;;) {
                bool failed = false;
                for (int k = 0; k < 2 && !failed; k++) {
                    if (eof[k] || (buf[k].size() >= block_bytes && !force)) continue;
                    const size_t have = buf[k].size();
                    buf[k].resize(have + block_bytes);
                    const size_t got = in[k].read(&buf[k][have], block_bytes);
                    if (got == (size_t)-1) { fail(RTX_ERR_PARSE, "read error in " + *name[k] + " (corrupt gzip stream?)"); failed = true; break; }
                    buf[k].resize(have + got);
                    eof[k] = got < block_bytes;
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
                        fail(RTX_ERR_PARSE, "paired FASTQ: " + *name[out] + " ends after record " + std::to_string(records) + ", " + *name[1 - out] + " goes on");
                        break;
                    }
                    force = true;  // no whole record of one file yet: read on
                    continue;
                }
                for (int k = 0; k < 2; k++) end[k] = last ? buf[k].size() : rtx_fastq_block_end_n(buf[k].data(), buf[k].size(), take, nullptr);
                auto blank = [](const std::string &t) { return t.find_first_not_of(" \t\r\n\v\f") == std::string::npos; };
                Parsed pz;
                pz.end = last;
                if (last && blank(buf[0]) && blank(buf[1])) { push(std::move(pz)); break; }  // both files ended with the block before
                if (last && n_rec[0] != n_rec[1]) {  // the files run out at different records
                    const int out = n_rec[0] < n_rec[1] ? 0 : 1;
                    fail(RTX_ERR_PARSE, "paired FASTQ: " + *name[out] + " ends after record " + std::to_string(records + n_rec[out]) + ", " + *name[1 - out] + " goes on");
                    break;
                }
                rtx_queries *mates[2] = {nullptr, nullptr};
                for (int k = 0; k < 2 && pz.rc == RTX_OK; k++) {
                    pz.rc = rtx_queries_parse_fastq_block(buf[k].data(), end[k], nullptr, 0, qual.ascii_base, 0u, &mates[k]);
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
                push(std::move(pz));
                if (failed || last) break;
                for (int k = 0; k < 2; k++) buf[k].erase(0, end[k]);
                {
                    std::lock_guard<std::mutex> g(qmu);
                    if (stop_reader) break;
                }
            }
            rtx_merge_destroy(stage);
            in[0].close();
            in[1].close();
            return;
        }
        Input f;
        if (!f.open(qf)) { Parsed e; e.rc = RTX_ERR_PARSE; e.err = "cannot open file"; e.end = true; push(std::move(e)); return; }
        std::string buf;
        bool first = true, eof = false;
        while (!eof) {
            const size_t have = buf.size();
            buf.resize(have + block_bytes);
            const size_t got = f.read(&buf[have], block_bytes);
            if (got == (size_t)-1) { Parsed e; e.rc = RTX_ERR_PARSE; e.err = "read error (corrupt gzip stream?)"; e.end = true; push(std::move(e)); break; }
            buf.resize(have + got);
            eof = got < block_bytes;
            uint64_t end = buf.size();
            uint32_t flags = first ? 0u : RTX_FASTA_NOT_FIRST;
            if (!eof) {
                end = fastq ? rtx_fastq_block_end(buf.data(), buf.size()) : rtx_fasta_block_end(buf.data(), buf.size());
                if (end == 0) continue;  // no header (FASTQ: no whole record) inside the block yet: read on
                flags |= RTX_FASTA_MORE_FOLLOWS;
            }
            Parsed pz;
            pz.rc = fastq ? rtx_queries_parse_fastq_block(buf.data(), end, skip.empty() ? nullptr : skip.data(), skip.size(), qual.ascii_base, flags, &pz.qs)
                          : rtx_queries_parse_fasta_block(buf.data(), end, skip.empty() ? nullptr : skip.data(), skip.size(), flags, &pz.qs);
            if (pz.rc != RTX_OK) pz.err = rtx_last_error();
            pz.end = eof || pz.rc != RTX_OK;
            const bool failed = pz.rc != RTX_OK;
            push(std::move(pz));
            if (failed) break;
            buf.erase(0, end);
            first = false;
            {
                std::lock_guard<std::mutex> g(qmu);
                if (stop_reader) break;
            }
        }
        f.close();
    });
    auto stop_and_join_reader = [&]() {
        {
            std::lock_guard<std::mutex> g(qmu);
            stop_reader = true;
            qcv.notify_all();
        }
        reader.join();
        for (Parsed &pz : ready) rtx_queries_destroy(pz.qs);
    };
    // one index handle per device, created side by side (each on a thread of its own: the builds run on their GPUs)
    std::vector<rtx_index *> indices(devices.size(), nullptr);
    std::vector<rtx_tally *> tallies(uniques ? devices.size() : 0, nullptr);  // --uniques: one object per handle, alive over the blocks of the file
    {
        std::vector<int> rcs(devices.size(), RTX_OK);
        std::vector<std::string> errs(devices.size());
        std::vector<std::thread> th;
        for (size_t k = 0; k < devices.size(); k++)
            th.emplace_back([&, k] {
                rcs[k] = rtx_index_create_from_tree(devices[k], tree, &indices[k]);
                if (rcs[k] == RTX_OK && device_format) rcs[k] = rtx_index_set_option(indices[k], RTX_OPT_DEVICE_TEXT, 1);
                if (rcs[k] == RTX_OK && both_strands) rcs[k] = rtx_index_set_option(indices[k], RTX_OPT_STRAND, 1);
                if (rcs[k] == RTX_OK && want_hits) rcs[k] = rtx_index_set_option(indices[k], RTX_OPT_NEAREST, 1);
                if (rcs[k] == RTX_OK && want_identity) rcs[k] = rtx_index_set_option(indices[k], RTX_OPT_IDENTITY, 1);
                if (rcs[k] == RTX_OK && derep) rcs[k] = rtx_index_set_option(indices[k], RTX_OPT_DEREP, 1);
                if (rcs[k] == RTX_OK && !primers.empty()) {
                    std::vector<rtx_trim_pattern> pats;
                    for (const Primer &p : primers) pats.push_back({p.codes.data(), (uint32_t)p.codes.size(), p.end, (uint32_t)(p.codes.size() * primer_pct / 100u), primer_window});
                    rcs[k] = rtx_index_set_primers(indices[k], pats.data(), (uint32_t)pats.size());
                }
                if (rcs[k] == RTX_OK && tags_on) {
                    std::vector<rtx_demux_tag> ct;
                    for (const Tag &t : tags) ct.push_back({t.codes.data(), (uint32_t)t.codes.size(), t.end});
                    rcs[k] = rtx_index_set_tags(indices[k], ct.data(), (uint32_t)ct.size(), tag_pairs.data(), (uint32_t)tag_pairs.size(), &tag_params);
                }
                if (rcs[k] == RTX_OK && qual_on) rcs[k] = rtx_index_set_quality(indices[k], &qual);
                if (rcs[k] == RTX_OK && screen_on) rcs[k] = rtx_index_set_screen(indices[k], contam_set, &contam);
                if (rcs[k] == RTX_OK && chim_on) rcs[k] = rtx_index_set_chimera(indices[k], &chim);
                if (rcs[k] == RTX_OK && uniques) {
                    const rtx_tally_params tp{tags_on ? (uint32_t)sample_names.size() : 0u, uniques_max_entries, uniques_max_bytes, 0, 0};
                    rcs[k] = rtx_tally_create(devices[k], &tp, &tallies[k]);
                    if (rcs[k] == RTX_OK) rcs[k] = rtx_index_set_tally(indices[k], tallies[k]);
                }
                if (rcs[k] == RTX_OK && profile_cutoff && tags_on)  // ... with a column of counters per sample (PREFIX/raxtax.samples)
                    rcs[k] = rtx_index_profile_begin_samples(indices[k], profile_cutoff, (skip_exact ? RTX_SKIP_EXACT_MATCHES : 0u) | (raw ? RTX_RAW_CONFIDENCE : 0u),
                                                             (uint32_t)sample_names.size());
                else if (rcs[k] == RTX_OK && profile_cutoff)
                    rcs[k] = rtx_index_profile_begin(indices[k], profile_cutoff, (skip_exact ? RTX_SKIP_EXACT_MATCHES : 0u) | (raw ? RTX_RAW_CONFIDENCE : 0u));
                if (rcs[k] != RTX_OK) errs[k] = rtx_last_error();
            });
        for (auto &t : th) t.join();
        for (size_t k = 0; k < devices.size(); k++)
            if (rcs[k] != RTX_OK) {
                fprintf(stderr, "[ERROR] device %d: %s\n", devices[k], errs[k].c_str());
                stop_and_join_reader();
                return 71;  // exitcode::OSERR
            }
    }
    rtx_screen_set_free(contam_set);  // (the handles keep what they need)
    contam_set = nullptr;
    lap("index");
    if (timing) {  // the handle's own verdict on tile pruning (rtx_index_self_sample: a property of the database)
        int on = 1;
        double share = -1.0;
        if (rtx_index_prune_verdict(indices[0], &on, &share) == RTX_OK && share >= 0.0)
            fprintf(stderr, "[TIMING] tile pruning %s: a sample of the database's own references keeps %.1f %% of its tiles live\n", on ? "on" : "off", 100.0 * share);
    }
    start_bin_writer();  // after the index: rtx_index_create_from_tree looks at the tree's k-mer map
    Sink sink;
    const auto mode = (redo || !resume) ? std::ios::trunc : std::ios::app;
    sink.out.open(out_path, mode);
    sink.ckp.open(ckp_path, mode);
    sink.want_tsv = tsv;
    if (tsv) sink.tsv.open(tsv_path, mode);
    if (both_strands) sink.strand.open(strand_path, mode);
    else if (mode == std::ios::trunc) remove(strand_path.c_str());  // (a run that starts over in a folder of a --strand both run: its file would describe other lines)
    if (want_hits) sink.hits.open(hits_path, mode);
    else if (mode == std::ios::trunc) remove(hits_path.c_str());  // (likewise)
    if (mode == std::ios::trunc) remove(profile_path.c_str());  // (written at the end of a run with --profile)
    if (mode == std::ios::trunc) { remove(uniques_path.c_str()); remove(uniques_table_path.c_str()); remove(otus_path.c_str()); remove(otus_map_path.c_str()); remove(otus_table_path.c_str()); }  // (written at the end of a run with --uniques)
    if (!primers.empty()) {
        const bool header = mode == std::ios::trunc || !is_file(trim_path);
        sink.trim.open(trim_path, mode);
        if (header) sink.trim << "label\tlength\tstart\tend\tprimer5\terrors5\tprimer3\terrors3\n";
        for (size_t k = 0; k < primers.size(); k++)
            fprintf(stderr, "[INFO ] --primers: pattern %zu at the %s end: %s, at most %zu error(s)\n", k, primers[k].end == RTX_TRIM_3P ? "3'" : "5'", primers[k].name.c_str(),
                    primers[k].codes.size() * primer_pct / 100u);
    } else if (mode == std::ios::trunc) remove(trim_path.c_str());  // (likewise)
    if (mode == std::ios::trunc) remove(samples_path.c_str());  // (written at the end of a run with --tags and --profile)
    if (tags_on) {
        const bool header = mode == std::ios::trunc || !is_file(demux_path);
        sink.demux.open(demux_path, mode);
        sink.sample_names = &sample_names;
        if (header) sink.demux << "label\tsample\tverdict\ttag5\tmm5\toff5\ttag3\tmm3\toff3\tlo\thi\n";
        for (size_t k = 0; k < tags.size(); k++)
            fprintf(stderr, "[INFO ] --tags: tag %zu at the %s end: %s\n", k, tags[k].end == RTX_TRIM_3P ? "3'" : "5'", tags[k].name.c_str());
        fprintf(stderr, "[INFO ] --tags: %zu samples, %zu pairs, at most %u mismatch(es), at most %u base(s) in front of a tag\n", sample_names.size(), tag_pairs.size(),
                tag_params.max_mismatches, tag_params.max_offset);
    } else if (mode == std::ios::trunc) remove(demux_path.c_str());  // (likewise)
    if (qual_on) {
        const bool header = mode == std::ios::trunc || !is_file(qc_path);
        sink.qc.open(qc_path, mode);
        if (header) sink.qc << "label\tlength\tstart\tend\texpected_errors\tverdict\n";
    } else if (mode == std::ios::trunc) remove(qc_path.c_str());  // (likewise)
    if (merge_on) {
        const bool header = mode == std::ios::trunc || !is_file(merge_path);
        sink.merge.open(merge_path, mode);
        if (header) sink.merge << "label\tforward_length\treverse_length\toverlap\tdiffs\tmerged_length\tverdict\n";
        fprintf(stderr, "[INFO ] --reverse: pairs of %s and %s are merged on device %d: overlap at least %u, at most %u diffs and %u %% of the overlap, Q capped at %u\n", qf.c_str(),
                rev_file.c_str(), devices[0], merge.min_overlap, merge.max_diffs, merge.max_diff_pct, merge.q_cap);
    } else if (mode == std::ios::trunc) remove(merge_path.c_str());  // (likewise)
    if (chim_on) {
        const bool header = mode == std::ios::trunc || !is_file(chim_path);
        sink.chimera.open(chim_path, mode);
        if (header) sink.chimera << "label\tstatus\twindows\tsingle\tparent_id\tseg\tpos\tleft\ta_id\tright\tb_id\tdelta\tchimera\tparent\ta\tb\n";
        fprintf(stderr, "[INFO ] --chimera: %u segments, a read is flagged from delta %u on\n", chim.segments, chim.mindelta);
    } else if (mode == std::ios::trunc) remove(chim_path.c_str());  // (likewise)
    if (screen_on) {
        const bool header = mode == std::ios::trunc || !is_file(screen_path);
        sink.screen.open(screen_path, mode);
        sink.contam_names = &contam_names;
        if (header) sink.screen << "label\tlength\twindows\thits\tfirst\tsource\tverdict\n";
    } else if (mode == std::ios::trunc) remove(screen_path.c_str());  // (likewise)
    sink.want_qc = qual_on;
    sink.want_strand = both_strands;
    sink.want_hits = want_hits;
    sink.tree = tree;
    // the writer of main.rs:127-135: result lines, then the label into the progress file
    auto sender = [](void *c, const char *label, const char *lines, const char *tsv_lines) -> int {
        Sink *s = static_cast<Sink *>(c);
        if (s->want_tsv && tsv_lines) s->tsv << tsv_lines << '\n';
        s->out << lines << '\n';
        s->ckp << label << '\n';
        return s->out.good() && s->ckp.good() ? 0 : 1;
    };
    // ... and in front of them, under --strand both, which orientation the lines are of
    // ... and, under --hits, which reference they look like: peak, t, ties, id and lineage of the nearest reference ('-' twice where no reference shares a k-mer)
    auto info = [](void *c, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t, uint32_t) -> int {   // (in the shape of --identity's callback)
        Sink *s = static_cast<Sink *>(c);
        if (s->want_strand) s->strand << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\n';
        if (s->want_hits) {
            s->hits << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\t' << ties << '\t';
            if (nearest == RTX_NO_REF) s->hits << "-\t-\n";
            else s->hits << nearest << '\t' << rtx_tree_lineage(s->tree, nearest) << '\n';
        }
        return (!s->want_strand || s->strand.good()) && (!s->want_hits || s->hits.good()) ? 0 : 1;
    };
    // ... and, under --identity, how far the query is from it: the edit distance and the identity in percent behind the line of --hits
    auto align = [](void *c, const char *label, int strand, uint32_t peak, uint32_t t, uint32_t nearest, uint32_t ties, uint32_t dist, uint32_t qlen) -> int {
        Sink *s = static_cast<Sink *>(c);
        if (s->want_strand) s->strand << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\n';
        s->hits << label << '\t' << (strand ? '-' : '+') << '\t' << peak << '\t' << t << '\t' << ties << '\t';
        if (nearest == RTX_NO_REF) s->hits << "-\t-";
        else s->hits << nearest << '\t' << rtx_tree_lineage(s->tree, nearest);
        if (dist == RTX_NO_DIST || qlen == 0u) {
            s->hits << "\t-\t-\n";
        } else {
            const uint64_t h = ((uint64_t)(qlen - dist) * 10000u + qlen / 2u) / qlen;  // hundredths of a percent
            char pct[32];
            snprintf(pct, sizeof pct, "%llu.%02llu", (unsigned long long)(h / 100u), (unsigned long long)(h % 100u));
            s->hits << '\t' << dist << '\t' << pct << '\n';
        }
        return (!s->want_strand || s->strand.good()) && s->hits.good() ? 0 : 1;
    };
    // ... and, under --primers, what was cut off every query (also one that has no result lines: an emptied read)
    auto trimmed = [](void *c, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint32_t hit) -> int {
        Sink *s = static_cast<Sink *>(c);
        const uint32_t p5 = hit & 0xFFu, e5 = (hit >> 8) & 0xFFu, p3 = (hit >> 16) & 0xFFu, e3 = hit >> 24;
        s->trim << label << '\t' << raw_len << '\t' << lo << '\t' << hi << '\t';
        if (p5 == RTX_TRIM_NO_PATTERN) s->trim << "-\t-\t";
        else s->trim << p5 << '\t' << e5 << '\t';
        if (p3 == RTX_TRIM_NO_PATTERN) s->trim << "-\t-\n";
        else s->trim << p3 << '\t' << e3 << '\n';
        return s->trim.good() ? 0 : 1;
    };
    // ... and, with a quality filter, what it made of every query (also one without result lines: a discarded read)
    auto filtered = [](void *c, const char *label, uint32_t raw_len, uint32_t lo, uint32_t hi, uint64_t ee, uint32_t verdict) -> int {
        static const char *const names[7] = {"bad_quality", "short_for_trunc_len", "too_short", "too_long", "too_many_n", "max_ee", "max_ee_rate"};
        Sink *s = static_cast<Sink *>(c);
        s->screen_len = verdict ? 0u : hi - lo;  // (what the contaminant screen is given of this query)
        if (!s->want_qc) return 0;
        char frac[8];  // six decimals of ee / 2^40, truncated: from the integer, no floating point
        snprintf(frac, sizeof frac, "%06llu", (unsigned long long)(((ee & ((1ull << 40) - 1)) * 1000000ull) >> 40));
        s->qc << label << '\t' << raw_len << '\t' << lo << '\t' << hi << '\t' << (ee >> 40) << '.' << frac << '\t';
        if (!verdict) s->qc << "pass";
        for (uint32_t b = 0, first = 1; b < 7u; b++)
            if ((verdict >> b) & 1u) { s->qc << (first ? "" : "+") << names[b]; first = 0; }
        s->qc << '\n';
        return s->qc.good() ? 0 : 1;
    };
    // ... and, under --chimera, what the check made of every query (also one without result lines: a flagged read)
    auto checked = [](void *c, const char *label, const rtx_chimera_rec *r) -> int {
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
    };
    // ... and, under --contaminants, what the screen made of every query (also one without result lines: a contaminant)
    auto screened = [](void *c, const char *label, uint32_t windows, uint32_t hits, uint32_t first, uint32_t source, uint32_t verdict) -> int {
        Sink *s = static_cast<Sink *>(c);
        s->screen << label << '\t' << s->screen_len << '\t' << windows << '\t' << hits << '\t';
        if (first == RTX_SCREEN_NONE) s->screen << '-';
        else s->screen << first;
        s->screen << '\t';
        if (source == RTX_SCREEN_NONE || source >= s->contam_names->size()) s->screen << '-';
        else s->screen << (*s->contam_names)[source];
        s->screen << '\t' << (verdict ? "contaminant" : "pass") << '\n';
        return s->screen.good() ? 0 : 1;
    };
    // ... and, under --tags, which sample every query belongs to (also one without result lines: a read that is not assigned)
    auto assigned = [](void *c, const char *label, uint32_t, uint32_t sample, uint32_t lo, uint32_t hi, uint32_t hit, uint32_t info) -> int {
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
    };
    int rc = RTX_OK;
    uint64_t n = 0;
    uint64_t trim_total[4] = {0, 0, 0, 0};  // --primers: over the blocks of the file (rtx_raxtax_last_trim)
    double trim_busy = 0;
    uint64_t qual_total[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the quality filter: queries, passed, cut short, the seven reasons (rtx_raxtax_last_qual)
    double qual_busy = 0;
    uint64_t chim_total[3] = {0, 0, 0};  // --chimera: queries, reads checked, queries flagged (rtx_raxtax_last_chimera)
    double chim_busy = 0;
    uint64_t screen_total[3] = {0, 0, 0};  // --contaminants: queries, screened, contaminants (rtx_raxtax_last_screen)
    double screen_busy = 0;
    uint64_t demux_total[7] = {0, 0, 0, 0, 0, 0, 0};  // --tags: queries, assigned, and the queries of every verdict (rtx_raxtax_last_demux)
    double demux_busy = 0;
    uint64_t derep_queries = 0, derep_distinct = 0;  // --derep: over the blocks of the file (rtx_raxtax_last_derep)
    double derep_busy = 0;
    uint64_t merge_total[6] = {0, 0, 0, 0, 0, 0};  // --reverse: pairs, merged, and not merged for each of the four reasons (RTX_MG_*)
    double merge_busy = 0;
    bool parse_failed = false;
    for (;;) {
        Parsed pz;
        {
            std::unique_lock<std::mutex> g(qmu);
            qcv.wait(g, [&] { return !ready.empty(); });
            pz = std::move(ready.front());
            ready.pop_front();
            qcv.notify_all();
        }
        if (pz.rc != RTX_OK) {
            fprintf(stderr, "[ERROR] Failed to parse %s: %s\n", qf.c_str(), pz.err.c_str());
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
            if (merge_on) {  // what the merge made of every pair of the block, before the block is classified
                static const char *const names[4] = {"bad_quality", "too_long", "too_short", "no_overlap"};
                const uint32_t *mnf, *mnr, *mov, *md, *mv;
                if (rtx_queries_merge_report(pz.qs, &mnf, &mnr, &mov, &md, &mv) == RTX_OK)
                    for (uint64_t i = 0; i < nb; i++) {
                        const char *verdict = "merged";
                        merge_total[0]++;
                        if (!mv[i]) merge_total[1]++;
                        for (uint32_t b = 0; b < 4u; b++)
                            if ((mv[i] >> b) & 1u) { verdict = names[b]; merge_total[2 + b]++; break; }
                        sink.merge << labels[i] << '\t' << mnf[i] << '\t' << mnr[i] << '\t' << mov[i] << '\t' << md[i] << '\t' << (off[i + 1] - off[i]) << '\t' << verdict << '\n';
                    }
                merge_busy += pz.merge_s[2];
                if (timing) fprintf(stderr, "[TIMING] merging of this block: %llu pairs, kernel %.3f ms, staging %.3f s, copies and wait %.3f s, all %.3f s (on the reader's thread, beside the classification of the block before)\n",
                                    (unsigned long long)nb, pz.merge_ms, pz.merge_s[0], pz.merge_s[1], pz.merge_s[2]);
            }
            // Chunks of 131 072 queries are what a device handles best (two sub-batches of 65 536 on its two streams, the next chunk enqueued ahead:
            // 43 ms per 524 288 queries against 101-113 with chunks of 32 768, the default until round 6); smaller ones when the block would
            // otherwise leave a device without two chunks of its own, never below 32 768.
            const size_t per_dev = (size_t)((nb + 2 * indices.size() - 1) / (2 * indices.size()));
            const size_t chunk_now = chunk ? chunk : std::min<size_t>(131072, std::max<size_t>(32768, per_dev));
            // one entry point takes everything a run can bring: an option that is off passes no callback
            const uint8_t *quals = nullptr;
            if (qual_on) rtx_queries_quals(pz.qs, &quals);
            rc = rtx_raxtax_multi_ex8(indices.data(), (uint32_t)indices.size(), tree, nb, labels.data(), bases, off, skip_exact, raw, chunk_now, sender, &sink, tsv,
                                      want_identity ? +align : (both_strands || want_hits ? +info : nullptr), &sink, primers.empty() ? nullptr : +trimmed, &sink,
                                      quals, qual_on || screen_on ? +filtered : nullptr, &sink, chim_on ? +checked : nullptr, &sink, tags_on ? +assigned : nullptr, &sink,
                                      screen_on ? +screened : nullptr, &sink);
            n += nb;
            if (screen_on) {
                uint64_t sq[3] = {0, 0, 0};
                double sb = 0;
                if (rtx_raxtax_last_screen(&sq[0], &sq[1], &sq[2], &sb) == RTX_OK) { for (int k = 0; k < 3; k++) screen_total[k] += sq[k]; screen_busy += sb; }
                if (timing) fprintf(stderr, "[TIMING] contaminant screen of this block: %llu queries, busy %.3f s (ahead of the device stage)\n", (unsigned long long)sq[0], sb);
            }
            if (tags_on) {
                uint64_t xq[7] = {0, 0, 0, 0, 0, 0, 0};
                double xb = 0;
                if (rtx_raxtax_last_demux(&xq[0], &xq[1], xq + 2, &xb) == RTX_OK) { for (int k = 0; k < 7; k++) demux_total[k] += xq[k]; demux_busy += xb; }
                if (timing) fprintf(stderr, "[TIMING] demultiplexing of this block: %llu queries, busy %.3f s (ahead of the device stage)\n", (unsigned long long)xq[0], xb);
            }
            if (!primers.empty()) {
                uint64_t tq[4] = {0, 0, 0, 0};
                double tb = 0;
                if (rtx_raxtax_last_trim(&tq[0], &tq[1], &tq[2], &tq[3], &tb) == RTX_OK) { for (int k = 0; k < 4; k++) trim_total[k] += tq[k]; trim_busy += tb; }
                if (timing) fprintf(stderr, "[TIMING] primer trimming of this block: %llu queries, busy %.3f s (ahead of the device stage)\n", (unsigned long long)tq[0], tb);
            }
            if (qual_on) {
                uint64_t qq[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                double qb = 0;
                if (rtx_raxtax_last_qual(&qq[0], &qq[1], &qq[2], qq + 3, &qb) == RTX_OK) { for (int k = 0; k < 10; k++) qual_total[k] += qq[k]; qual_busy += qb; }
                if (timing) fprintf(stderr, "[TIMING] quality filter of this block: %llu queries, busy %.3f s (ahead of the device stage)\n", (unsigned long long)qq[0], qb);
            }
            if (chim_on) {
                uint64_t cq[3] = {0, 0, 0};
                double cb = 0;
                if (rtx_raxtax_last_chimera(&cq[0], &cq[1], &cq[2], &cb) == RTX_OK) { for (int k = 0; k < 3; k++) chim_total[k] += cq[k]; chim_busy += cb; }
                if (timing) fprintf(stderr, "[TIMING] chimera check of this block: %llu queries, %llu reads checked, busy %.3f s (ahead of the device stage)\n", (unsigned long long)cq[0], (unsigned long long)cq[1], cb);
            }
            if (derep) {
                uint64_t dq = 0, du = 0;
                double db_ = 0;
                if (rtx_raxtax_last_derep(&dq, &du, &db_) == RTX_OK) { derep_queries += dq; derep_distinct += du; derep_busy += db_; }
                if (timing) fprintf(stderr, "[TIMING] dereplication of this block: %llu queries, %llu distinct, busy %.3f s (ahead of the device stage)\n", (unsigned long long)dq, (unsigned long long)du, db_);
            }
            if (timing) {  // busy seconds of the pipeline stages of this block (which stage bounds the run)
                double busy[4];
                uint64_t nch = 0;
                if (rtx_raxtax_last_timing(busy, &nch) == RTX_OK)
                    fprintf(stderr, "[TIMING] pipeline busy seconds over %llu chunk(s) on %zu handle(s): lookup %.3f, device %.3f (busiest handle), format %.3f, sender %.3f\n",
                            (unsigned long long)nch, indices.size(), busy[0], busy[1], busy[2], busy[3]);
                uint64_t ahead = 0, abandoned = 0;  // RTX_OPT_RUN_AHEAD (the first handle, since its creation)
                if (rtx_index_run_ahead_stats(indices[0], &ahead, &abandoned) == RTX_OK)
                    fprintf(stderr, "[TIMING] chunks enqueued ahead of the end of the chunk before them: %llu, abandoned: %llu (queries of this block: %llu)\n", (unsigned long long)ahead,
                            (unsigned long long)abandoned, (unsigned long long)nb);
            }
        }
        rtx_queries_destroy(pz.qs);
        if (rc != RTX_OK || pz.end) break;
    }
    stop_and_join_reader();
    sink.out.flush();
    sink.ckp.flush();
    if (tsv) sink.tsv.flush();
    if (both_strands) sink.strand.flush();
    if (want_hits) sink.hits.flush();
    if (!primers.empty()) sink.trim.flush();
    if (qual_on) sink.qc.flush();
    if (merge_on) sink.merge.flush();
    if (chim_on) sink.chimera.flush();
    if (tags_on) sink.demux.flush();
    if (screen_on) sink.screen.flush();
    if (parse_failed) { join_bin_writer(); return 66; }
    lap("classify_and_write");
    if (merge_on) {
        fprintf(stderr, "[INFO ] --reverse: %llu pairs, %llu merged; not merged for bad_quality %llu, too_long %llu, too_short %llu, no_overlap %llu\n", (unsigned long long)merge_total[0],
                (unsigned long long)merge_total[1], (unsigned long long)merge_total[2], (unsigned long long)merge_total[3], (unsigned long long)merge_total[4], (unsigned long long)merge_total[5]);
        if (timing) t_log << ", \"merge_busy\": " << merge_busy;
    }
    if (tags_on) {
        fprintf(stderr, "[INFO ] --tags: %llu queries, %llu assigned to a sample; not assigned for no_tag5 %llu, no_tag3 %llu, ambiguous %llu, unknown_pair %llu\n",
                (unsigned long long)demux_total[0], (unsigned long long)demux_total[1], (unsigned long long)demux_total[3], (unsigned long long)demux_total[4],
                (unsigned long long)demux_total[5], (unsigned long long)demux_total[6]);
        if (timing) t_log << ", \"demux_busy\": " << demux_busy;
    }
    if (!primers.empty()) {
        fprintf(stderr, "[INFO ] --primers: %llu queries, %llu with a 5' primer, %llu with a 3' primer, %llu left empty\n", (unsigned long long)trim_total[0],
                (unsigned long long)trim_total[1], (unsigned long long)trim_total[2], (unsigned long long)trim_total[3]);
        if (timing) t_log << ", \"trim_busy\": " << trim_busy;
    }
    if (qual_on) {
        fprintf(stderr, "[INFO ] quality filter: %llu queries, %llu passed (%llu of them cut short); discarded for bad_quality %llu, short_for_trunc_len %llu, too_short %llu, "
                        "too_long %llu, too_many_n %llu, max_ee %llu, max_ee_rate %llu\n", (unsigned long long)qual_total[0], (unsigned long long)qual_total[1],
                (unsigned long long)qual_total[2], (unsigned long long)qual_total[3], (unsigned long long)qual_total[4], (unsigned long long)qual_total[5],
                (unsigned long long)qual_total[6], (unsigned long long)qual_total[7], (unsigned long long)qual_total[8], (unsigned long long)qual_total[9]);
        if (timing) t_log << ", \"qual_busy\": " << qual_busy;
    }
    if (screen_on) {
        fprintf(stderr, "[INFO ] --contaminants: %llu queries, %llu screened, %llu contaminants\n", (unsigned long long)screen_total[0], (unsigned long long)screen_total[1],
                (unsigned long long)screen_total[2]);
        if (timing) t_log << ", \"screen_busy\": " << screen_busy;
    }
    if (chim_on) {
        fprintf(stderr, "[INFO ] --chimera: %llu queries, %llu reads checked, %llu queries flagged\n", (unsigned long long)chim_total[0], (unsigned long long)chim_total[1],
                (unsigned long long)chim_total[2]);
        if (timing) t_log << ", \"chimera_busy\": " << chim_busy;
    }
    if (derep) {  // (per chunk: a copy in another chunk counts as a distinct read of its own)
        fprintf(stderr, "[INFO ] --derep: %llu queries, %llu distinct\n", (unsigned long long)derep_queries, (unsigned long long)derep_distinct);
        if (timing) t_log << ", \"derep_busy\": " << derep_busy;
    }
    if (!join_bin_writer()) return 74;
    lap("database_cache_wait");
    if (timing) fprintf(stderr, "{\"n_queries\": %llu, %s}\n", (unsigned long long)n, t_log.str().c_str());
    if (rc != RTX_OK) {
        fprintf(stderr, "[ERROR] %s\nRerun raxtax-hip to continue from the last checkpoint.\n", rtx_last_error());
        return rc == RTX_ERR_SENDER ? 75 : 70;  // exitcode::TEMPFAIL / SOFTWARE
    }
    if (profile_cutoff) {  // the taxon profile of the whole run: the sum over the handles, written once
        std::vector<rtx_profile_view> views(indices.size());
        std::vector<rtx_profile_view *> ptrs(indices.size());
        int prc = RTX_OK;
        for (size_t k = 0; k < indices.size() && prc == RTX_OK; k++) {
            prc = rtx_index_profile_read(indices[k], &views[k]);
            ptrs[k] = &views[k];
        }
        std::vector<uint64_t> acc(prc == RTX_OK ? 3 * (size_t)views[0].n_nodes : 0);
        uint64_t totals[4] = {0, 0, 0, 0};
        const size_t nn = prc == RTX_OK ? views[0].n_nodes : 0;
        if (prc == RTX_OK) prc = rtx_profile_merge(ptrs.data(), (uint32_t)ptrs.size(), acc.data(), acc.data() + nn, acc.data() + 2 * nn, totals);
        std::string text;
        if (prc == RTX_OK) {
            const int64_t need = rtx_profile_format(tree, acc.data(), acc.data() + nn, acc.data() + 2 * nn, totals, profile_cutoff, nullptr, 0);
            if (need < 0) prc = (int)need;
            else {
                text.resize((size_t)need);
                const int64_t got = rtx_profile_format(tree, acc.data(), acc.data() + nn, acc.data() + 2 * nn, totals, profile_cutoff, &text[0], text.size());
                if (got != need) prc = got < 0 ? (int)got : RTX_ERR_STATE;
            }
        }
        if (prc != RTX_OK) { fprintf(stderr, "[ERROR] taxon profile: %s\n", rtx_last_error()); return 70; }
        std::ofstream pf(profile_path, std::ios::trunc);
        pf << text;
        pf.close();
        if (!pf.good()) { fprintf(stderr, "[ERROR] cannot write %s\n", profile_path.c_str()); return 74; }
    }
    if (profile_cutoff && tags_on) {  // ... and the taxon x sample table beside it: the per-sample counters summed over the handles
        std::vector<rtx_sample_profile_view> views(indices.size());
        std::vector<rtx_sample_profile_view *> ptrs(indices.size());
        int prc = RTX_OK;
        for (size_t k = 0; k < indices.size() && prc == RTX_OK; k++) {
            prc = rtx_index_profile_read_samples(indices[k], &views[k]);
            ptrs[k] = &views[k];
        }
        const size_t nn = prc == RTX_OK ? views[0].n_nodes : 0, ns = sample_names.size();
        std::vector<uint64_t> direct(ns * nn + 1), totals(ns * 4);
        if (prc == RTX_OK) prc = rtx_sample_profile_merge(ptrs.data(), (uint32_t)ptrs.size(), direct.data(), totals.data());
        std::vector<const char *> names;
        for (const std::string &s : sample_names) names.push_back(s.c_str());
        std::string text;
        if (prc == RTX_OK) {
            const int64_t need = rtx_sample_table_format(tree, (uint32_t)ns, names.data(), direct.data(), totals.data(), profile_cutoff, nullptr, 0);
            if (need < 0) prc = (int)need;
            else {
                text.resize((size_t)need);
                const int64_t got = rtx_sample_table_format(tree, (uint32_t)ns, names.data(), direct.data(), totals.data(), profile_cutoff, &text[0], text.size());
                if (got != need) prc = got < 0 ? (int)got : RTX_ERR_STATE;
            }
        }
        if (prc != RTX_OK) { fprintf(stderr, "[ERROR] sample table: %s\n", rtx_last_error()); return 70; }
        std::ofstream sf(samples_path, std::ios::trunc);
        sf << text;
        sf.close();
        if (!sf.good()) { fprintf(stderr, "[ERROR] cannot write %s\n", samples_path.c_str()); return 74; }
    }
    if (uniques) {  // the distinct reads of the whole run: the tables of the handles' objects read, summed and written once
        std::vector<rtx_tally_table *> tables(tallies.size(), nullptr);
        rtx_tally_table *sum = nullptr;
        int trc = RTX_OK;
        for (size_t k = 0; k < tallies.size() && trc == RTX_OK; k++) trc = rtx_tally_read(tallies[k], &tables[k]);
        if (trc == RTX_OK) trc = rtx_tally_table_merge(tables.data(), (uint32_t)tables.size(), &sum);
        rtx_tally_view view{};
        if (trc == RTX_OK) trc = rtx_tally_table_view(sum, &view);
        std::vector<const char *> names;
        for (const std::string &s : sample_names) names.push_back(s.c_str());
        std::string fasta, table;
        auto format = [&](std::string &text, auto fn) {  // the two-pass protocol of the formatters
            const int64_t need = fn(nullptr, 0);
            if (need < 0) { trc = (int)need; return; }
            text.resize((size_t)need);
            const int64_t got = fn(&text[0], text.size());
            if (got != need) trc = got < 0 ? (int)got : RTX_ERR_STATE;
        };
        if (trc == RTX_OK) format(fasta, [&](char *buf, uint64_t cap) { return rtx_tally_format_fasta(sum, uniques_minsize, buf, cap); });
        if (trc == RTX_OK && tags_on) format(table, [&](char *buf, uint64_t cap) { return rtx_tally_format_table(sum, names.data(), uniques_minsize, buf, cap); });
        if (trc != RTX_OK) { fprintf(stderr, "[ERROR] distinct reads: %s\n", rtx_last_error()); return 70; }
        fprintf(stderr, "[INFO ] --uniques: %llu reads, %llu distinct\n", (unsigned long long)view.totals[0], (unsigned long long)view.totals[1]);
        if (view.totals[2])
            fprintf(stderr, "[INFO ] --uniques: %llu of %llu reads belong to sequences beyond the caps (--uniques-max-entries, --uniques-max-bytes) and are in no entry\n",
                    (unsigned long long)view.totals[2], (unsigned long long)view.totals[0]);
        std::ofstream uf(uniques_path, std::ios::trunc);
        uf << fasta;
        uf.close();
        if (!uf.good()) { fprintf(stderr, "[ERROR] cannot write %s\n", uniques_path.c_str()); return 74; }
        if (tags_on) {
            std::ofstream tf(uniques_table_path, std::ios::trunc);
            tf << table;
            tf.close();
            if (!tf.good()) { fprintf(stderr, "[ERROR] cannot write %s\n", uniques_table_path.c_str()); return 74; }
        }
        if (otus) {  // the OTUs of the run: the summed table, whole, clustered on the first device
            rtx_otu *o = nullptr;
            rtx_otu_view_t ov{};
            std::string otu_fasta, otu_map, otu_table;
            trc = rtx_otu_cluster(devices[0], sum, nullptr, &o);
            if (trc == RTX_OK) trc = rtx_otu_view(o, &ov);
            if (trc == RTX_OK) format(otu_fasta, [&](char *buf, uint64_t cap) { return rtx_otu_format_fasta(o, sum, otus_minsize, buf, cap); });
            if (trc == RTX_OK) format(otu_map, [&](char *buf, uint64_t cap) { return rtx_otu_format_map(o, buf, cap); });
            if (trc == RTX_OK && tags_on) format(otu_table, [&](char *buf, uint64_t cap) { return rtx_otu_format_table(o, names.data(), otus_minsize, buf, cap); });
            if (trc != RTX_OK) { fprintf(stderr, "[ERROR] OTUs: %s\n", rtx_last_error()); return 70; }
            fprintf(stderr, "[INFO ] --otus: %llu distinct reads, %llu links, %llu OTUs, %u rounds\n", (unsigned long long)ov.n_rows, (unsigned long long)ov.n_links,
                    (unsigned long long)ov.n_otus, ov.rounds);
            if (ov.long_rows)
                fprintf(stderr, "[INFO ] --otus: %llu distinct reads are longer than %d bases and stand alone\n", (unsigned long long)ov.long_rows, RTX_OTU_MAX_LEN);
            const std::pair<const std::string *, const std::string *> files[] = {{&otus_path, &otu_fasta}, {&otus_map_path, &otu_map}, {&otus_table_path, &otu_table}};
            for (size_t k = 0; k < (tags_on ? 3u : 2u); k++) {
                std::ofstream of(*files[k].first, std::ios::trunc);
                of << *files[k].second;
                of.close();
                if (!of.good()) { fprintf(stderr, "[ERROR] cannot write %s\n", files[k].first->c_str()); return 74; }
            }
            rtx_otu_destroy(o);
        }
        rtx_tally_table_destroy(sum);
        for (rtx_tally_table *t : tables) rtx_tally_table_destroy(t);
    }
    if (clean) {  // Checkpoint::cleanup (io.rs:80-89)
        remove(ckp_json.c_str());
        remove(ckp_path.c_str());
        if (!db_bin.empty()) remove(db_bin.c_str());
    }
    for (rtx_index *ix : indices) rtx_index_destroy(ix);
    for (rtx_tally *t : tallies) rtx_tally_destroy(t);
    rtx_tree_destroy(tree);
    return 0;
}

// Arithmetic shared by the HIP kernels and the host-side emulation used by the CPU
// tests (tests/test_device_math_cpu.py drives it through rtx_emul_* in rtx_emul.cpp).
// Everything here is `RTX_HD` so that the exact same source runs on gfx950 and on x86.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RTX_HD __host__ __device__ __forceinline__
#else
#define RTX_HD inline
#endif

namespace rtx {

// segment classes (rtx_kernels.hpp): entries of a slot, the most references of a sparse (row, tile) segment, the most sparse segments
// of a (query, tile) -- here because the CPU emulation of the epilogue's merge (rtx_emul.cpp) applies the same cap
constexpr uint32_t kSegSlotEntries = 16, kSegSparseMax = 16, kSegMaxSparseRows = 255;

// ---------------------------------------------------------------------------
// Bit-sliced ("vertical") counters.
//
// hit_count adds one 32-reference bitmap word per query k-mer into NP bit planes:
// plane p holds bit p of the 32 per-reference counters.  Eight words are folded per
// step with a carry-save adder tree (7 CSAs -> one carry of weight 8) followed by a
// ripple into planes 3..NP-1.  count[r] = |K(q) ∩ K(r)| (src/raxtax.rs:58-64) exactly:
// the planes are an exact binary representation as long as count < 2^NP.
// ---------------------------------------------------------------------------

// ---------------------------------------------------------------------------
// Where reference r (local id) sits in a bitmap row.  A tile = 8192 references = 64 lanes x 16 B of the
// row; the last tile of a row spans only L = (stride - tile*1024)/16 lanes.  hit_count unpacks the
// 128 counters of a lane as 16 groups of 8 (group g = word g/4, bits 8(g%4)..+7); group g of lane l
// holds references tile*8192 + (g*L + l)*8 + [0, 8), so that the sixteen 16-byte count stores of a
// wave are each contiguous across lanes (stored lane-major they cost 4 of hit_count's 24 ms).
// ---------------------------------------------------------------------------
RTX_HD uint32_t tile_lanes(uint32_t stride_bytes, uint32_t tile) {
    const uint32_t rem = stride_bytes - tile * 1024u;
    return rem >= 1024u ? 64u : rem >> 4;
}
// The bitmap is stored TILE-major: [tile][row][256 words] (n_rows1 = rows + the all-zero row).  The segments a
// (query, tile) wave reads lie in one region of n_rows1 KiB, so that a row is a 32-bit offset (row << 10) from the
// tile's base whatever the size of the database: one buffer descriptor per wave, the row offset as the load's SGPR.
RTX_HD size_t bitmap_word(uint32_t row, uint32_t word, uint32_t n_rows1) {
    return ((size_t)(word >> 8) * n_rows1 + row) * 256u + (word & 255u);
}
// word index within the row and bit within the word
RTX_HD void ref_slot(uint32_t r, uint32_t stride_bytes, uint32_t &word, uint32_t &bit) {
    const uint32_t tile = r >> 13, rl = r & 8191u;
    const uint32_t L = tile_lanes(stride_bytes, tile);
    const uint32_t c = rl >> 3, l = c % L, g = c / L;
    word = tile * 256u + l * 4u + (g >> 2);
    bit = (g & 3u) * 8u + (rl & 7u);
}

// ---------------------------------------------------------------------------
// Where the count of local reference rl of a tile sits in what the dense epilogues of hit_count store (nearest_kernel, rtx_nearest.hip;
// taxon_prefix reads the same places chunk by chunk).  Group g of lane l goes to offset (g*L + l)*8 of the tile's stretch of the row, which
// is where its references are: the stored counts are in REFERENCE order, in a full tile and in the short last one alike, whatever lane
// held them.  u16 counts: element rl.  Packed counts (10 bits): the low byte at byte rl, the two high bits at bits 2 (rl & 7) of the u16
// of chunk rl >> 3 (the tile's high-bit words begin at u16 tile * 1024 of the row's high part).
// ---------------------------------------------------------------------------
RTX_HD void packed_count_pos(uint32_t rl, uint32_t &byte, uint32_t &hi_word, uint32_t &hi_shift) {
    byte = rl;
    hi_word = rl >> 3;
    hi_shift = (rl & 7u) * 2u;
}
// nearest_kernel scans a tile in steps of 64 lanes, every lane `per_lane` consecutive references (16 packed: 16 bytes of low bytes and
// two high-bit words; 8 as u16: 16 bytes): the first local reference of a lane.  Ascending in (step, lane), so the lowest lane of the
// first step with a match holds the lowest reference.
RTX_HD uint32_t nearest_lane_base(uint32_t step, uint32_t lane, uint32_t per_lane) { return (step * 64u + lane) * per_lane; }
// bit j: reference base + j (base a multiple of 16, below in_tile = the references the tile holds) has the count `peak`.
// lo: its 16 low bytes, hi2: the high-bit words of chunks base >> 3 (low half) and (base >> 3) + 1 (high half)
RTX_HD uint32_t nearest_match16(const uint32_t (&lo)[4], uint32_t hi2, uint32_t peak, uint32_t base, uint32_t in_tile) {
    uint32_t m = 0;
    for (uint32_t j = 0; j < 16u; j++) {
        uint32_t byte, hw, hs;
        packed_count_pos(base + j, byte, hw, hs);
        byte -= base;
        hw -= base >> 3;
        const uint32_t c = ((lo[byte >> 2] >> ((byte & 3u) * 8u)) & 0xFFu) | (((hi2 >> (hw * 16u + hs)) & 3u) << 8);
        if (c == peak && base + j < in_tile) m |= 1u << j;
    }
    return m;
}
// the same over 8 u16 counts (w: four words, base a multiple of 8)
RTX_HD uint32_t nearest_match8(const uint32_t (&w)[4], uint32_t peak, uint32_t base, uint32_t in_tile) {
    uint32_t m = 0;
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t c = (w[j >> 1] >> ((j & 1u) * 16u)) & 0xFFFFu;
        if (c == peak && base + j < in_tile) m |= 1u << j;
    }
    return m;
}

// ---------------------------------------------------------------------------
// Alignment identity (identity_kernel, rtx_identity.hip; rtx_semiglobal_distance on the host; emul_identity on x86): the semi-global
// edit distance of a query against its nearest reference by Myers' bit-vector algorithm in its block form (Myers 1999, in Hyyro's
// formulation).  The pattern is the query in blocks of 64 bases, the text the reference; the horizontal delta that enters row 0 is 0 in
// every column (the text's overhang is free), the score of the query's last row starts at qlen.
// No per-symbol Peq: a block keeps the four one-hot bit PLANES of its 64 codes (bit j of plane x = code j has bit x), and Eq of a text
// code c is the OR of the planes whose bit c holds -- two codes match when both are codes (1 .. 15) and intersect, a byte that is 0 or
// above 15 has no bit in any plane and selects none.
// ---------------------------------------------------------------------------
struct IdentityBlock {
    uint64_t pv, mv;        // vertical deltas +1 / -1 of the block's rows in the column last processed (column -1: all +1)
    uint64_t plane[4];
};
// the code a text or pattern byte contributes: itself if it is one (1 .. 15), else 0
RTX_HD uint32_t identity_code(uint32_t byte) { return byte > 15u ? 0u : byte; }
// base i of the query in the orientation that was classified: fetch(j) = byte j as the caller gave it; minus = the reverse complement
// (index reversed, the four bits of a code reversed, a byte above 15 unchanged: complement_code)
template <class F>
RTX_HD uint32_t identity_query_byte(const F &fetch, uint32_t qlen, uint32_t i, bool minus) {
    if (!minus) return fetch(i);
    const uint32_t b = fetch(qlen - 1u - i);
    return b > 15u ? b : (((b & 1u) << 3) | ((b & 2u) << 1) | ((b & 4u) >> 1) | ((b & 8u) >> 3));
}
// block `blk` of a query of qlen bases (blk * 64 < qlen) before the first column
template <class F>
RTX_HD void identity_block_init(IdentityBlock &b, const F &fetch, uint32_t qlen, uint32_t blk, bool minus) {
    b.pv = ~0ull;
    b.mv = 0ull;
    b.plane[0] = b.plane[1] = b.plane[2] = b.plane[3] = 0ull;
    const uint32_t i0 = blk * 64u, n = qlen - i0 < 64u ? qlen - i0 : 64u;
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t c = identity_code(identity_query_byte(fetch, qlen, i0 + j, minus));
        b.plane[0] |= (c & 1u) << j;
        b.plane[1] |= ((c >> 1) & 1u) << j;
        b.plane[2] |= ((c >> 2) & 1u) << j;
        b.plane[3] |= ((c >> 3) & 1u) << j;
    }
}
// One column through one block.  code: identity_code of the text byte; hin: the horizontal delta at the block's top (-1, 0, +1: 0 for the
// first block, the block above's result otherwise); out_mask: the one bit of the row of the block whose horizontal delta is returned -- row 63
// hands it to the block below, row (qlen - 1) % 64 of the last block is the change of the score of the query's last row (identity_out_mask;
// a mask and not a bit number: a 64-bit shift by a register is the slowest thing the step could hold).
RTX_HD uint64_t identity_out_mask(uint32_t qlen, uint32_t blk) { return 1ull << ((blk + 1u) * 64u >= qlen ? (qlen - 1u) & 63u : 63u); }
RTX_HD int identity_step(IdentityBlock &b, uint32_t code, int hin, uint64_t out_mask) {
    uint64_t eq = ((code & 1u) ? b.plane[0] : 0ull) | ((code & 2u) ? b.plane[1] : 0ull) | ((code & 4u) ? b.plane[2] : 0ull) |
                  ((code & 8u) ? b.plane[3] : 0ull);
    const uint64_t pv = b.pv, mv = b.mv;
    const uint64_t xv = eq | mv;
    if (hin < 0) eq |= 1ull;
    const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;  // (the only carry chain)
    uint64_t ph = mv | ~(xh | pv);
    uint64_t mh = pv & xh;
    const int hout = ((ph & out_mask) != 0ull ? 1 : 0) - ((mh & out_mask) != 0ull ? 1 : 0);
    ph = (ph << 1) | (hin > 0 ? 1ull : 0ull);
    mh = (mh << 1) | (hin < 0 ? 1ull : 0ull);
    b.pv = mh | ~(xv | ph);
    b.mv = ph & xv;
    return hout;
}
// hundredths of a percent of the query's bases that the alignment keeps (what the CLI prints): ((qlen - dist) 10000 + qlen / 2) / qlen
RTX_HD uint32_t identity_hundredths(uint32_t dist, uint32_t qlen) {
    return qlen ? (uint32_t)(((uint64_t)(qlen - dist) * 10000u + qlen / 2u) / qlen) : 0u;
}

// ---------------------------------------------------------------------------
// Primer trimming (trim_kernel, rtx_trim.hip; rtx_primer_search on the host; emul_trim_* on x86): Sellers' search of a pattern of at most
// 64 codes in the first w bases of a text, by the block step above with the roles swapped -- the PATTERN is the block, the read the text.
// E[j] = the least distance of the whole pattern to a substring that ends at j (the text in front is free: horizontal delta 0 into row 0,
// E[0] = m); the answer is the least E and the LARGEST j that has it, found when it is at most k.
// The text arrives as the stage packs it (trim_stage_row): two bases per byte, base j in nibble j, a byte above 15 as 0 (both match nothing),
// a 3' window reversed, in chunks of 32 bases = 16 bytes (TrimWords: one load of the lane's own row).
// ---------------------------------------------------------------------------
struct TrimPattern {     // one pattern as the kernel argument carries it (uniform over a wave: scalar registers)
    uint64_t plane[4];   // bit j of plane x: code j of the pattern AS IT IS SEARCHED (a 3' pattern reversed) has bit x
    uint32_t m, k, w;    // codes, errors allowed (k < m), window (resolved by trim_window: 1 .. 256)
    uint32_t index;      // its place in the caller's list (what the hit word names)
};
struct TrimWords { uint32_t w[4]; };
constexpr uint32_t kTrimNone = 0xFFu;          // the hit word's pattern where nothing was found
constexpr uint32_t kTrimNoDist = 0xFFFFFFFFu;  // (RTX_NO_DIST)
RTX_HD uint32_t trim_window(uint32_t m, uint32_t k, uint32_t window) {
    if (window) return window;
    const uint32_t d = m + k + 32u;
    return d < 256u ? d : 256u;
}
RTX_HD uint32_t trim_row_stride(uint32_t w) { return (w + 31u) / 32u * 16u; }  // bytes of a row that holds w bases: whole 16-byte loads
// codes: the pattern as given (m of them, every one 1 .. 15); reversed: a 3' pattern (it is searched in the reversed read)
RTX_HD void trim_pattern_init(TrimPattern &p, const uint8_t *codes, uint32_t m, uint32_t k, uint32_t window, bool reversed, uint32_t index) {
    p.plane[0] = p.plane[1] = p.plane[2] = p.plane[3] = 0ull;
    for (uint32_t j = 0; j < m; j++) {
        const uint64_t c = identity_code(codes[reversed ? m - 1u - j : j]);
        p.plane[0] |= (c & 1u) << j;
        p.plane[1] |= ((c >> 1) & 1u) << j;
        p.plane[2] |= ((c >> 2) & 1u) << j;
        p.plane[3] |= ((c >> 3) & 1u) << j;
    }
    p.m = m;
    p.k = k;
    p.w = trim_window(m, k, window);
    p.index = index;
}
// the first min(len, w) bases of x (reversed: the last ones, last base first) into a row of trim_row_stride(w) bytes; what lies behind them is zero
RTX_HD void trim_stage_row(const uint8_t *x, uint64_t len, uint32_t w, bool reversed, uint8_t *row) {
    const uint32_t n = len < w ? (uint32_t)len : w, stride = trim_row_stride(w);
    for (uint32_t b = 0; b < stride; b++) {
        const uint32_t j0 = 2u * b, j1 = j0 + 1u;
        const uint32_t c0 = j0 < n ? identity_code(x[reversed ? len - 1u - j0 : j0]) : 0u;
        const uint32_t c1 = j1 < n ? identity_code(x[reversed ? len - 1u - j1 : j1]) : 0u;
        row[b] = (uint8_t)(c0 | (c1 << 4));
    }
}
// load(c): bases 32 c .. 32 c + 31 of the text; len: the bases the read has (the text is its first min(len, p.w)).  The chunk loop is
// uniform over a wave (p.w is), a lane whose text has ended sits the steps out.  cut = 0 and err = kTrimNoDist when not found.
template <class L>
RTX_HD void trim_search(const TrimPattern &p, const L &load, uint32_t len, uint32_t &cut, uint32_t &err) {
    IdentityBlock b;
    b.pv = ~0ull;
    b.mv = 0ull;
    b.plane[0] = p.plane[0]; b.plane[1] = p.plane[1]; b.plane[2] = p.plane[2]; b.plane[3] = p.plane[3];
    const uint64_t out_mask = 1ull << (p.m - 1u);
    const uint32_t n = len < p.w ? len : p.w;
    uint32_t score = p.m, best = p.m, best_j = 0u;
    for (uint32_t c = 0; c * 32u < p.w; c++) {
        const TrimWords t = load(c);
#pragma unroll
        for (uint32_t i = 0; i < 32u; i++) {
            const uint32_t j = c * 32u + i;
            if (j < n) {
                score += (uint32_t)identity_step(b, (t.w[i >> 3] >> ((i & 7u) * 4u)) & 15u, 0, out_mask);
                if (score <= best) { best = score; best_j = j + 1u; }  // (<=: the latest j of the least E)
            }
        }
    }
    const bool found = best <= p.k;
    cut = found ? best_j : 0u;
    err = found ? best : kTrimNoDist;
}
// One read against the patterns of both ends (pat[0 .. n5): 5', pat[n5 .. n5 + n3): 3', each end in the order of the caller's list): the
// least errors win, then the lowest index; the ends are searched independently on the untrimmed read.  load5 / load3: the read's rows.
template <class L5, class L3>
RTX_HD void trim_read(const TrimPattern *pat, uint32_t n5, uint32_t n3, const L5 &load5, const L3 &load3, uint32_t len, uint32_t &lo,
                      uint32_t &hi, uint32_t &hit) {
    uint32_t cut5 = 0u, err5 = kTrimNoDist, pat5 = kTrimNone, cut3 = 0u, err3 = kTrimNoDist, pat3 = kTrimNone;
    for (uint32_t i = 0; i < n5; i++) {
        uint32_t c, e;
        trim_search(pat[i], load5, len, c, e);
        if (e < err5) { err5 = e; cut5 = c; pat5 = pat[i].index; }
    }
    for (uint32_t i = n5; i < n5 + n3; i++) {
        uint32_t c, e;
        trim_search(pat[i], load3, len, c, e);
        if (e < err3) { err3 = e; cut3 = c; pat3 = pat[i].index; }
    }
    lo = cut5;
    hi = len - cut3;
    if (hi < lo) hi = lo;  // the cuts overlap: the read is left empty
    hit = pat5 | ((pat5 == kTrimNone ? 0u : err5) << 8) | (pat3 << 16) | ((pat3 == kTrimNone ? 0u : err3) << 24);
}

// ---------------------------------------------------------------------------
// Sample demultiplexing (demux_kernel, rtx_demux.hip; rtx_demux_read on the host; emul_demux_reads on x86): which inline tag stands at
// each end of a read, by Hamming distance over the admissible offsets -- include/raxtax_hip.h has the semantics.
// A tag is at most 32 codes, packed like the text: code j in nibble j of two 64-bit words, the nibbles behind the tag zero (they match
// nothing, which is the length mask: no second mask is carried).  The text arrives as trim_stage_row packs it: the first (3': the last,
// reversed) max_offset + 32 bases of the read, a byte above 15 as 0, what lies behind them zero -- 47 nibbles at the most, three words.
// Placing a tag at offset s is a shift of the window by 4 s bits; the matching positions are the nibbles where tag AND window is not zero,
// folded to one bit each and counted: d = m - popcount.
// ---------------------------------------------------------------------------
struct DemuxTag {        // one tag as the kernel reads it, by a wave-uniform index (scalar loads)
    uint64_t w[2];       // code j AS IT IS SEARCHED (a 3' tag reversed) in nibble j
    uint32_t m, index;   // codes; its place in the caller's list (what the hit word names)
};
struct DemuxWindow { uint64_t w[3]; };
constexpr uint32_t kDemuxNoTag = 0xFFFFu, kDemuxNone = 0xFFFFFFFFu, kDemuxMaxMismatches = 8u;
enum : uint32_t { kDemuxOk = 0u, kDemuxNoTag5 = 1u, kDemuxNoTag3 = 2u, kDemuxAmbiguous = 3u, kDemuxUnknownPair = 4u };
RTX_HD uint32_t demux_window(uint32_t max_offset) { return max_offset + 32u; }  // bases of an end that are staged
RTX_HD void demux_tag_init(DemuxTag &t, const uint8_t *codes, uint32_t m, bool reversed, uint32_t index) {
    t.w[0] = t.w[1] = 0ull;
    for (uint32_t j = 0; j < m; j++) t.w[j >> 4] |= (uint64_t)identity_code(codes[reversed ? m - 1u - j : j]) << ((j & 15u) * 4u);
    t.m = m;
    t.index = index;
}
// the window of a staged row of `stride` bytes (trim_row_stride: 16 or 32), word by word
RTX_HD DemuxWindow demux_window_of(const uint8_t *row, uint32_t stride) {
    DemuxWindow x{{0ull, 0ull, 0ull}};
    for (uint32_t b = 0; b < (stride < 24u ? stride : 24u); b++) x.w[b >> 3] |= (uint64_t)row[b] << ((b & 7u) * 8u);
    return x;
}
// bit 4 j: nibble j of x is not zero
RTX_HD uint64_t demux_fold(uint64_t x) {
    x |= x >> 1;
    x |= x >> 2;
    return x & 0x1111111111111111ull;
}
// One end: tags[0 .. n) against the window at the offsets 0 .. max_offset (both loops uniform over a wave; a placement with s + m > len
// sits out).  best = the least distance (~0: no placement), tag / off = the first (offset, tag) that reaches it -- when one tag alone
// reaches it, that tag at its least offset -- and two = another tag reaches it as well.
RTX_HD void demux_end(const DemuxTag *tags, uint32_t n, const DemuxWindow &x, uint32_t len, uint32_t max_offset, uint32_t &best,
                      uint32_t &tag, uint32_t &off, bool &two) {
    best = ~0u;
    tag = 0u;
    off = 0u;
    two = false;
    uint64_t x0 = x.w[0], x1 = x.w[1], x2 = x.w[2];
    for (uint32_t s = 0; s <= max_offset; s++) {
        for (uint32_t i = 0; i < n; i++) {
            const DemuxTag &t = tags[i];
            const uint32_t hits = (uint32_t)__builtin_popcountll(demux_fold(t.w[0] & x0)) + (uint32_t)__builtin_popcountll(demux_fold(t.w[1] & x1));
            const uint32_t d = s + t.m <= len ? t.m - hits : ~0u;  // (selects, no branches: the lanes of a wave differ here all the time)
            const bool less = d < best;
            two = !less && (two || (d == best && i != tag));  // (while best is ~0 this may hold: `two` counts only once something is found)
            tag = less ? i : tag;
            off = less ? s : off;
            best = less ? d : best;
        }
        x0 = (x0 >> 4) | (x1 << 60);
        x1 = (x1 >> 4) | (x2 << 60);
        x2 >>= 4;
    }
}
// One read against the tags of both ends (tags[0 .. n5): 5', tags[n5 .. n5 + n3): 3', each end in the order of the caller's list).
// pair(i5, i3): the sample of the pair of the i5-th 5' tag (n5: none) and the i3-th 3' tag (n3: none), kDemuxNone when the table has no
// such pair.  An end has a tag when its least distance is at most max_mismatches and one tag alone reaches it.
template <class P>
RTX_HD void demux_read(const DemuxTag *tags, uint32_t n5, uint32_t n3, const P &pair, uint32_t max_mismatches, uint32_t max_offset,
                       const DemuxWindow &x5, const DemuxWindow &x3, uint32_t len, uint32_t &sample, uint32_t &lo, uint32_t &hi, uint32_t &hit,
                       uint32_t &info) {
    uint32_t d5 = ~0u, t5 = 0u, s5 = 0u, d3 = ~0u, t3 = 0u, s3 = 0u;
    bool two5 = false, two3 = false;
    if (n5) demux_end(tags, n5, x5, len, max_offset, d5, t5, s5, two5);
    if (n3) demux_end(tags + n5, n3, x3, len, max_offset, d3, t3, s3, two3);
    const bool found5 = d5 <= max_mismatches, found3 = d3 <= max_mismatches;
    const bool has5 = found5 && !two5, has3 = found3 && !two3;
    const uint32_t i5 = has5 ? t5 : n5, i3 = has3 ? t3 : n3;
    uint32_t verdict = kDemuxOk;
    sample = kDemuxNone;
    if ((found5 && two5) || (found3 && two3)) verdict = kDemuxAmbiguous;
    else if (n5 && !found5) verdict = kDemuxNoTag5;
    else if (n3 && !found3) verdict = kDemuxNoTag3;
    else {
        sample = pair(i5, i3);
        if (sample == kDemuxNone) verdict = kDemuxUnknownPair;
    }
    lo = has5 ? s5 + tags[i5].m : 0u;
    hi = has3 ? len - (s3 + tags[n5 + i3].m) : len;
    if (hi < lo) hi = lo;  // the cuts overlap: the read is left empty
    hit = (has5 ? tags[i5].index : kDemuxNoTag) | ((has3 ? tags[n5 + i3].index : kDemuxNoTag) << 16);
    info = verdict | ((has5 ? d5 : 0u) << 8) | ((has3 ? d3 : 0u) << 16) | ((has5 ? s5 : 0u) << 24) | ((has3 ? s3 : 0u) << 28);
}
// The dense pair table the kernel looks up: (n5 + 1) x (n3 + 1) samples, row i5 (n5: no 5' tag), column i3 (n3: no 3' tag), kDemuxNone
// where there is no pair.  rank[t]: the place of tag t of the caller's list within its end.
RTX_HD size_t demux_table_size(uint32_t n5, uint32_t n3) { return (size_t)(n5 + 1u) * (n3 + 1u); }
RTX_HD size_t demux_table_slot(uint32_t n3, uint32_t i5, uint32_t i3) { return (size_t)i5 * (n3 + 1u) + i3; }

// ---------------------------------------------------------------------------
// Quality filter (qual_kernel, rtx_qual.hip; rtx_qual_read on the host; emul_qual_read on x86): where a read is cut and why it is discarded,
// from its FASTQ quality string -- include/raxtax_hip.h has the semantics.  Exact integers: the error probability of quality Q is
// e[Q] = llround(10^(-Q/10) * 2^40), computed once on the host (qual_table), a threshold x is floor(x * 2^40); a read has at most 2^20 bases,
// so no sum exceeds 2^60.
// The read arrives as the stage packs it: one byte per base, the raw quality byte in bits 0-6, bit 7 set where the base is no A/C/G/T, in
// pieces of 16 bytes (QualWords: one load).  A piece is worked in two halves, because the cut of trunc_ee needs the sum of everything in
// front of the piece: qual_piece_sum (the piece's own prefix sums and totals), then -- after the scan over the pieces of a step, across the
// lanes of a group on the device, a plain loop in qual_read_serial -- qual_piece_stop (the first position to cut in front of).
// ---------------------------------------------------------------------------
constexpr uint32_t kQualMaxQ = 93u;                // Q = 0 .. 93: the printable ASCII range above base 33
constexpr uint32_t kQualMaxRead = 1u << 20;        // RTX_QUAL_MAX_READ
constexpr uint32_t kQualPiece = 16u;               // bytes of a piece
constexpr uint32_t kQualGroup = 16u;               // pieces of a step: the lanes of a group
constexpr uint64_t kQualOff = ~0ull;               // a threshold that is off (a given one is at most 2^63)
constexpr uint32_t kQcBadQuality = 1u, kQcShortForTruncLen = 2u, kQcTooShort = 4u, kQcTooLong = 8u, kQcTooManyN = 16u, kQcMaxEe = 32u,
                   kQcMaxEeRate = 64u;             // RTX_QC_*
struct QualCfg {           // rtx_qual_params as integers (host_qual.cpp: qual_cfg_init); uniform over a wave
    uint32_t base;         // 33 or 64
    uint32_t trunc_len;    // 0: off
    int32_t trunc_qual;    // < 0: off
    uint64_t trunc_ee;     // kQualOff: off
    uint32_t min_len, max_len;  // 0: off
    int32_t max_ns;        // < 0: off
    uint64_t max_ee;       // kQualOff: off
    uint64_t max_ee_rate;  // kQualOff: off
};
struct QualWords { uint32_t w[4]; };
struct QualPiece {
    uint64_t c[kQualPiece];  // inclusive prefix sums of e over the piece's bytes (a byte at or behind `end` adds 0)
    uint32_t ns;             // bit j: byte j is an N in front of `end`
    uint32_t low;            // bit j: byte j lies in front of `end` and has Q <= trunc_qual
    bool bad;                // a byte in front of `len` has Q outside 0 .. 93
};
// The piece at bytes pos .. pos + 15 of a range of len bytes, of which [0, end) stand for truncation (end <= len: trunc_len applied).
RTX_HD void qual_piece_sum(const QualCfg &cfg, const uint64_t *table, const QualWords &t, uint32_t pos, uint32_t len, uint32_t end, QualPiece &p) {
    uint64_t run = 0;
    p.ns = p.low = 0u;
    p.bad = false;
#pragma unroll
    for (uint32_t j = 0; j < kQualPiece; j++) {
        const uint32_t b = (t.w[j >> 2] >> ((j & 3u) * 8u)) & 0xFFu;
        const uint32_t q = (b & 0x7Fu) - cfg.base;  // (wraps below the base: above 93 as well)
        const bool in_len = pos + j < len, in_end = pos + j < end;
        p.bad = p.bad || (in_len && q > kQualMaxQ);
        const uint64_t e = table[q > kQualMaxQ ? 0u : q];
        run += in_end ? e : 0ull;
        p.c[j] = run;
        p.ns |= (uint32_t)(in_end && (b & 0x80u) != 0u) << j;
        p.low |= (uint32_t)(in_end && cfg.trunc_qual >= 0 && q <= (uint32_t)cfg.trunc_qual) << j;
    }
}
// before: the sum of e over everything of the range in front of the piece.  The first byte j of the piece to cut in front of -- Q <= trunc_qual,
// or before + c[j] above trunc_ee -- or kQualPiece when it has none; ee / ns: what the piece adds in front of that byte.
RTX_HD uint32_t qual_piece_stop(const QualCfg &cfg, const QualPiece &p, uint64_t before, uint32_t pos, uint32_t end, uint64_t &ee, uint32_t &ns) {
    uint32_t stop = kQualPiece;
#pragma unroll
    for (uint32_t j = kQualPiece; j-- > 0u;) {
        const bool over = cfg.trunc_ee != kQualOff && pos + j < end && before + p.c[j] > cfg.trunc_ee;
        if (over || ((p.low >> j) & 1u)) stop = j;
    }
    ee = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < kQualPiece; j++)
        if (j + 1u == stop) ee = p.c[j];
    const uint32_t m = p.ns & ((1u << stop) - 1u);
#if defined(__HIP_DEVICE_COMPILE__)
    ns = (uint32_t)__popc(m);
#else
    ns = (uint32_t)__builtin_popcount(m);
#endif
    return stop;
}
// is ee above rate * kept?  (rate up to 2^63, kept below 2^21: the product in 96 bits)
RTX_HD bool qual_rate_exceeded(uint64_t ee, uint64_t rate, uint32_t kept) {
    const uint64_t p0 = (rate & 0xFFFFFFFFull) * kept, p1 = (rate >> 32) * kept;  // the product is (p1 << 32) + p0
    const uint64_t mid = p1 + (p0 >> 32);
    if (mid >> 32) return false;  // 2^64 or more: no sum reaches it
    return ee > ((mid << 32) | (p0 & 0xFFFFFFFFull));
}
// len: the bytes of the input range; short_tl: it was shorter than trunc_len; kept / ee / ns: of [0, kept)
RTX_HD uint32_t qual_verdict(const QualCfg &cfg, bool bad, bool short_tl, uint32_t kept, uint64_t ee, uint32_t ns) {
    if (bad) return kQcBadQuality;
    uint32_t v = short_tl ? kQcShortForTruncLen : 0u;
    if (cfg.min_len && kept < cfg.min_len) v |= kQcTooShort;
    if (cfg.max_len && kept > cfg.max_len) v |= kQcTooLong;
    if (cfg.max_ns >= 0 && ns > (uint32_t)cfg.max_ns) v |= kQcTooManyN;
    if (cfg.max_ee != kQualOff && ee > cfg.max_ee) v |= kQcMaxEe;
    if (cfg.max_ee_rate != kQualOff && qual_rate_exceeded(ee, cfg.max_ee_rate, kept)) v |= kQcMaxEeRate;
    return v;
}
// [0, end) of a range of len bytes stands for truncation: trunc_len cuts it, a range shorter than trunc_len keeps its length (and is discarded)
RTX_HD uint32_t qual_end(const QualCfg &cfg, uint32_t len, bool &short_tl) {
    short_tl = cfg.trunc_len != 0u && len < cfg.trunc_len;
    return cfg.trunc_len != 0u && !short_tl ? cfg.trunc_len : len;
}
// One range of len bytes, the steps and pieces of qual_kernel one after the other.  load(i): bytes 16 i .. 16 i + 15 of the range.
template <class L>
RTX_HD void qual_read_serial(const QualCfg &cfg, const uint64_t *table, const L &load, uint32_t len, uint32_t &kept, uint64_t &ee, uint32_t &verdict) {
    bool short_tl, bad = false, done = false;
    const uint32_t end = qual_end(cfg, len, short_tl);
    uint64_t carry_e = 0;
    uint32_t carry_n = 0, hi = end;
    for (uint32_t pos = 0; pos < len; pos += kQualPiece) {
        QualPiece p;
        qual_piece_sum(cfg, table, load(pos / kQualPiece), pos, len, end, p);
        bad = bad || p.bad;
        if (done) continue;
        uint64_t e;
        uint32_t n;
        const uint32_t stop = qual_piece_stop(cfg, p, carry_e, pos, end, e, n);
        carry_e += e;
        carry_n += n;
        if (stop != kQualPiece) { hi = pos + stop; done = true; }
    }
    kept = bad ? 0u : hi;
    ee = bad ? 0ull : carry_e;
    verdict = qual_verdict(cfg, bad, short_tl, hi, carry_e, carry_n);
}

// ---------------------------------------------------------------------------
// Contaminant screen (screen_kernel, rtx_screen.hip; rtx_screen_read on the host; emul_screen_read on x86): the 16-mers of a read looked up
// in a set of canonical 16-mers -- include/raxtax_hip.h has the semantics and the table's layout.  Exact integers.
// The read arrives as its 4-bit codes, one byte per base, in pieces of 16 bytes (ScreenWords: one load).  A piece is the 16 window
// positions that START in it: screen_piece takes the piece and the one behind it (the 15 bases beyond), rolls the forward and the
// reverse-complement word over the 31 bases and probes every valid window (screen_probe).  Nothing is carried from piece to piece.
// ---------------------------------------------------------------------------
constexpr uint32_t kScreenK = 16u;                 // RTX_SCREEN_K
constexpr uint32_t kScreenNone = 0xFFFFFFFFu;      // RTX_SCREEN_NONE; as a key: an empty slot (no canonical value is all ones)
constexpr uint32_t kScreenMaxRead = 1u << 20;      // RTX_SCREEN_MAX_READ
constexpr uint32_t kScreenPiece = 16u;             // window positions of a piece: the bytes of one load
constexpr uint32_t kScreenGroup = 16u;             // pieces of a step: the lanes of a group
constexpr uint32_t kScreenMinSlots = 1024u;
constexpr uint32_t kScreenHashMul = 0x9E3779B1u;
struct ScreenWords { uint32_t w[4]; };
struct alignas(8) ScreenSlot { uint32_t key, src; };
struct ScreenTable { const ScreenSlot *slots; uint32_t log2m; };   // m = 1 << log2m slots, at least one of them empty
struct ScreenAcc { uint32_t windows, hits, first, source; };       // of the pieces a lane has seen; first / source: kScreenNone without a hit

RTX_HD uint32_t screen_home(uint32_t c, uint32_t log2m) { return (uint32_t)(c * kScreenHashMul) >> (32u - log2m); }
// The reverse complement of a 16-mer word: base j is 3 - base 15 - j
RTX_HD uint32_t screen_rc(uint32_t w) {
    w = ~w;
    w = (w >> 2 & 0x33333333u) | (w & 0x33333333u) << 2;
    w = (w >> 4 & 0x0F0F0F0Fu) | (w & 0x0F0F0F0Fu) << 4;
    w = (w >> 8 & 0x00FF00FFu) | (w & 0x00FF00FFu) << 8;
    return w >> 16 | w << 16;
}
// One chain: from the home slot of c to c (true, src set) or to an empty slot (false).  At most m slots are looked at.
RTX_HD bool screen_probe(const ScreenTable &t, uint32_t c, uint32_t &src) {
    const uint32_t mask = (1u << t.log2m) - 1u;
    uint32_t h = screen_home(c, t.log2m);
    for (uint32_t i = 0; i <= mask; i++) {
        const ScreenSlot s = t.slots[h];
        if (s.key == c) { src = s.src; return true; }
        if (s.key == kScreenNone) return false;
        h = (h + 1u) & mask;
    }
    return false;
}
// The windows that start at pos .. pos + 15 of a range of len bases; a: bytes pos .. pos + 15, b: bytes pos + 16 .. pos + 31 (anything where
// they lie at or behind len).  Adds to acc; the pieces of a lane come in ascending order, so the first hit ever seen stays.
RTX_HD void screen_piece(const ScreenTable &t, const ScreenWords &a, const ScreenWords &b, uint32_t pos, uint32_t len, ScreenAcc &acc) {
    uint32_t fw = 0u, rc = 0u, run = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 2u * kScreenPiece - 1u; j++) {
        const uint32_t code = ((j < kScreenPiece ? a.w[j >> 2] : b.w[(j - kScreenPiece) >> 2]) >> (8u * (j & 3u))) & 0xFFu;
        const bool acgt = pos + j < len && (code == 1u || code == 2u || code == 4u || code == 8u);
        const uint32_t two = (code >> 1 & 1u) | (code >> 2 & 1u) << 1 | (code >> 3 & 1u) * 3u;  // 1, 2, 4, 8 -> 0, 1, 2, 3
        fw = fw << 2 | two;
        rc = rc >> 2 | (3u - two) << 30;
        run = acgt ? run + 1u : 0u;
        if (j >= kScreenK - 1u && run >= kScreenK) {  // the window that starts at pos + j - 15 and ends with this base
            const uint32_t c = fw < rc ? fw : rc;
            uint32_t src = kScreenNone;
            acc.windows++;
            if (screen_probe(t, c, src)) {
                acc.hits++;
                if (acc.first == kScreenNone) { acc.first = pos + j - (kScreenK - 1u); acc.source = src; }
            }
        }
    }
}
RTX_HD uint32_t screen_verdict(uint32_t hits, uint32_t windows, uint32_t min_hits, uint32_t min_pct) {
    return hits >= min_hits && 100ull * hits >= (uint64_t)min_pct * windows ? 1u : 0u;
}

// ---------------------------------------------------------------------------
// Paired-end merging (merge_kernel, rtx_merge.hip; rtx_merge_pair on the host; emul_merge_pair on x86): the two mates of a pair overlapped
// into one read -- include/raxtax_hip.h has the semantics.  Exact integers.
// A mate is staged as nibble words -- 16 base codes to a uint64, base p in bits 4 (p & 15) of word p >> 4 -- and a byte of Q per base; the
// reverse mate as its reverse complement R', so that candidate ov sets F[nf - ov + i] against R'[i]: an unaligned read of F (merge_word_at),
// an aligned one of R', an AND, and the zero nibbles of it under the tail mask (merge_word_diffs).  merge_stage4 builds four bases of either
// array, merge_candidate walks one candidate and returns its key, merge_base_at gives one base of the merged read.
// ---------------------------------------------------------------------------
constexpr uint32_t kMergeMaxRead = 1024u;          // RTX_MERGE_MAX_READ
constexpr uint32_t kMergeMismatchCost = 5u;        // RTX_MERGE_MISMATCH_COST
constexpr uint32_t kMergeStride = 64u;             // candidates of a step: the lanes of a wave
constexpr uint32_t kMergeWords = kMergeMaxRead / 16u + 2u;  // words of a staged mate: the unaligned read of the last word takes its neighbour (and one to keep 16 bytes)
constexpr uint32_t kMergeKeyOvBits = 11u;          // ov <= 1024
constexpr uint32_t kMgBadQuality = 1u, kMgTooLong = 2u, kMgTooShort = 4u, kMgNoOverlap = 8u;  // RTX_MG_*
struct MergeCfg { uint32_t base, min_overlap, max_diffs, max_diff_pct, q_cap; };  // rtx_merge_params, checked (host_merge.cpp: merge_check_params)

RTX_HD uint32_t merge_code(uint32_t b) { return b > 15u ? 0u : b; }  // a byte that is no 4-bit code counts as 0
RTX_HD uint32_t merge_comp(uint32_t c) { return ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3); }  // rtx_revcomp of one code
RTX_HD bool merge_bad_byte(const MergeCfg &cfg, uint32_t byte) { return byte - cfg.base > kQualMaxQ; }  // (wraps below the base)
// the verdicts that need no candidate, in their order; 0: the candidates decide
RTX_HD uint32_t merge_pre_verdict(const MergeCfg &cfg, bool bad, uint32_t nf, uint32_t nr) {
    if (bad) return kMgBadQuality;
    if (nf > kMergeMaxRead || nr > kMergeMaxRead) return kMgTooLong;
    if (nf < cfg.min_overlap || nr < cfg.min_overlap) return kMgTooShort;
    return 0u;
}
// Bases 4 h .. 4 h + 3 of a staged mate of n bases (n <= kMergeMaxRead; rev: of its reverse complement): their codes as 16 bits of a nibble word,
// their quality bytes as they came (little-endian), 0 behind the mate's end; bad: one of them has Q outside 0 .. 93.
template <class LC, class LQ>
RTX_HD void merge_stage4(const MergeCfg &cfg, const LC &code_at, const LQ &qual_at, uint32_t n, bool rev, uint32_t h, uint32_t &nib16, uint32_t &q32, bool &bad) {
    nib16 = q32 = 0u;
    bad = false;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t p = 4u * h + k;
        if (p >= n) continue;
        const uint32_t at = rev ? n - 1u - p : p;
        const uint32_t c = merge_code(code_at(at)), q = qual_at(at);
        nib16 |= (rev ? merge_comp(c) : c) << (4u * k);
        q32 |= (q & 0xFFu) << (8u * k);
        bad = bad || merge_bad_byte(cfg, q & 0xFFu);
    }
}
RTX_HD uint64_t merge_tail_mask(uint32_t nibbles) { return nibbles >= 16u ? ~0ull : (1ull << (4u * nibbles)) - 1ull; }  // the first `nibbles` of a word
// the nibbles of x & y that are zero, among those of the mask: the diffs of one candidate in one word
RTX_HD uint32_t merge_word_diffs(uint64_t x, uint64_t y, uint64_t mask) {
    uint64_t z = x & y;
    z |= z >> 1;
    z |= z >> 2;  // bit 0 of every nibble: the nibble is not zero
    const uint64_t zero = ~z & 0x1111111111111111ull & mask;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(zero);
#else
    return (uint32_t)__builtin_popcountll(zero);
#endif
}
// 16 nibbles from nibble `nib` (0 .. 15) of lo on, continued in hi
RTX_HD uint64_t merge_word_at(uint64_t lo, uint64_t hi, uint32_t nib) { return nib ? (lo >> (4u * nib)) | (hi << (64u - 4u * nib)) : lo; }
RTX_HD uint32_t merge_nibble(uint64_t w, uint32_t p) { return (uint32_t)(w >> (4u * (p & 15u))) & 15u; }
// (score, ov) as one integer: the best candidate is the maximum, among equal scores the larger ov.  Only for an accepted candidate
// (ov >= 5 d + min_overlap >= 1): never 0, which stands for none.
RTX_HD uint32_t merge_key(uint32_t ov, uint32_t d) { return ((ov - kMergeMismatchCost * d) << kMergeKeyOvBits) | ov; }
RTX_HD void merge_key_read(uint32_t key, uint32_t &ov, uint32_t &d) {
    ov = key & ((1u << kMergeKeyOvBits) - 1u);
    d = (ov - (key >> kMergeKeyOvBits)) / kMergeMismatchCost;
}
RTX_HD bool merge_accept(const MergeCfg &cfg, uint32_t ov, uint32_t d) {  // (d <= ov <= 1024: nothing wraps)
    return d <= cfg.max_diffs && 100u * d <= cfg.max_diff_pct * ov && ov >= kMergeMismatchCost * d + cfg.min_overlap;
}
// Candidate ov (min_overlap <= ov <= min(nf, nr)): its key, or 0 when it is not accepted.  word_f(w) / word_r(w): word w of the staged F / R'.
// Left as soon as d is above max_diffs.
template <class WF, class WR>
RTX_HD uint32_t merge_candidate(const MergeCfg &cfg, const WF &word_f, const WR &word_r, uint32_t nf, uint32_t ov) {
    const uint32_t f0 = nf - ov, w0 = f0 >> 4, nib = f0 & 15u;
    uint32_t d = 0;
    uint64_t lo = word_f(w0);
    for (uint32_t w = 0; 16u * w < ov; w++) {
        const uint64_t hi = word_f(w0 + w + 1u);
        d += merge_word_diffs(merge_word_at(lo, hi, nib), word_r(w), merge_tail_mask(ov - 16u * w));
        if (d > cfg.max_diffs) return 0u;
        lo = hi;
    }
    return merge_accept(cfg, ov, d) ? merge_key(ov, d) : 0u;
}
// one position of an overlap: a, qa of F against b, qb of R' (Q values, 0 .. 93)
RTX_HD void merge_consensus(const MergeCfg &cfg, uint32_t a, uint32_t qa, uint32_t b, uint32_t qb, uint32_t &code, uint32_t &q) {
    const uint32_t hi = qa > qb ? qa : qb;
    if (a == b && a != 0u) {
        const uint32_t sum = qa + qb, capped = sum < cfg.q_cap ? sum : cfg.q_cap;
        code = a;
        q = hi > capped ? hi : capped;
    } else if ((a & b) != 0u) {
        code = a & b;
        q = hi;
    } else {
        const uint32_t diff = qa > qb ? qa - qb : qb - qa;
        code = qb > qa ? b : a;
        q = diff > 2u ? diff : 2u;
    }
}
// Base p of the read merged at overlap ov (p < nf + nr - ov): its code and its quality BYTE.  qual_f(p) / qual_r(i): the quality byte of F[p] / R'[i].
template <class WF, class WR, class QF, class QR>
RTX_HD void merge_base_at(const MergeCfg &cfg, const WF &word_f, const WR &word_r, const QF &qual_f, const QR &qual_r, uint32_t nf, uint32_t ov, uint32_t p,
                          uint32_t &code, uint32_t &byte) {
    const uint32_t f0 = nf - ov;
    if (p < f0) {
        code = merge_nibble(word_f(p >> 4), p);
        byte = qual_f(p);
    } else if (p >= nf) {
        code = merge_nibble(word_r((p - f0) >> 4), p - f0);
        byte = qual_r(p - f0);
    } else {
        uint32_t q;
        merge_consensus(cfg, merge_nibble(word_f(p >> 4), p), qual_f(p) - cfg.base, merge_nibble(word_r((p - f0) >> 4), p - f0), qual_r(p - f0) - cfg.base, code, q);
        byte = cfg.base + q;
    }
}
// One pair whose mates are staged, the candidates one after the other: the best key, 0 for none.
template <class WF, class WR>
RTX_HD uint32_t merge_best_serial(const MergeCfg &cfg, const WF &word_f, const WR &word_r, uint32_t nf, uint32_t nr) {
    uint32_t best = 0;
    for (uint32_t ov = cfg.min_overlap; ov <= (nf < nr ? nf : nr); ov++) {
        const uint32_t k = merge_candidate(cfg, word_f, word_r, nf, ov);
        best = k > best ? k : best;
    }
    return best;
}

// ---------------------------------------------------------------------------
// Hash of an encoded sequence for the exact-match lookup (Tree.sequences.get, raxtax.rs:42) on the device.  The bytes are taken
// as 8-byte little-endian words (the last one zero-padded); every word is mixed with its position and the mixes are ADDED, so
// that the lanes of a wave can hash their words independently and meet in one sum.  Equal sequences hash equal; a collision only
// costs a byte compare (the lookup verifies every candidate byte by byte).  The host builds the table with the same functions.
// ---------------------------------------------------------------------------
RTX_HD uint64_t em_mix_word(uint64_t w, uint64_t j) {
    uint64_t v = w + 0x9E3779B97F4A7C15ull * (j + 1u);
    v ^= v >> 32;
    v *= 0xD6E8FEB86659FD93ull;
    v ^= v >> 29;
    v *= 0xFF51AFD7ED558CCDull;
    v ^= v >> 32;
    return v;
}
RTX_HD uint64_t em_finish(uint64_t sum, uint64_t len) {
    uint64_t h = sum ^ (len * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 29;
    return h;
}
// slot of a hash in a table of 2^bits slots, and the 32-bit tag kept beside the group (never 0: 0 marks an empty slot)
RTX_HD uint32_t em_slot(uint64_t h, uint32_t bits) { return (uint32_t)(h >> (64u - bits)); }
RTX_HD uint32_t em_tag(uint64_t h) { const uint32_t t = (uint32_t)h; return t ? t : 1u; }

// full adder on bit vectors: (a + b + c) -> sum (weight 1), carry (weight 2)
RTX_HD void csa(uint32_t a, uint32_t b, uint32_t c, uint32_t &sum, uint32_t &carry) {
#if defined(__HIP_DEVICE_COMPILE__)
    // gfx950 v_bitop3_b32: any 3-input boolean in one op.  0x96 = a^b^c, 0xE8 = majority(a,b,c)
    // (the carry first: the sum can then take the register of `a`, the plane it replaces)
    const uint32_t c_ = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    sum = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
    carry = c_;
#else
    uint32_t u = a ^ b;
    uint32_t s_ = u ^ c;
    carry = (a & b) | (u & c);
    sum = s_;
#endif
}

template <int NP>
RTX_HD void planes_add8(uint32_t (&pl)[NP], uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4,
                        uint32_t a5, uint32_t a6, uint32_t a7) {
    uint32_t t1a, t1b, t1c, t1d, t2a, t2b, e;
    csa(pl[0], a0, a1, pl[0], t1a);
    csa(pl[0], a2, a3, pl[0], t1b);
    csa(pl[1], t1a, t1b, pl[1], t2a);
    csa(pl[0], a4, a5, pl[0], t1c);
    csa(pl[0], a6, a7, pl[0], t1d);
    csa(pl[1], t1c, t1d, pl[1], t2b);
    csa(pl[2], t2a, t2b, pl[2], e);
#pragma unroll
    for (int p = 3; p < NP; p++) {  // ripple the weight-8 carry upwards
        uint32_t c = pl[p] & e;
        pl[p] ^= e;
        e = c;
    }
}

// Harley-Seal style tree: folds eight words into planes 0..2 and RETURNS the carry of weight 8
// (7 CSAs, 21 ops); the caller combines such carries pairwise with further CSAs on planes 3, 4
// (32 inputs = 31 CSAs) before one ripple, 3.2 ops per input word instead of 4.4 for planes_add8.
template <int NP>
RTX_HD uint32_t planes_tree8(uint32_t (&pl)[NP], uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4,
                             uint32_t a5, uint32_t a6, uint32_t a7) {
    uint32_t t1a, t1b, t1c, t1d, t2a, t2b, e;
    csa(pl[0], a0, a1, pl[0], t1a);
    csa(pl[0], a2, a3, pl[0], t1b);
    csa(pl[1], t1a, t1b, pl[1], t2a);
    csa(pl[0], a4, a5, pl[0], t1c);
    csa(pl[0], a6, a7, pl[0], t1d);
    csa(pl[1], t1c, t1d, pl[1], t2b);
    csa(pl[2], t2a, t2b, pl[2], e);
    return e;
}

// adds a carry vector of weight 2^L into planes L..NP-1
template <int NP, int L>
RTX_HD void planes_ripple(uint32_t (&pl)[NP], uint32_t e) {
#pragma unroll
    for (int p = L; p < NP; p++) {
        uint32_t c = pl[p] & e;
        pl[p] ^= e;
        e = c;
    }
}

// ---- bit-sliced numbers as values (the two-level bounds pass, rtx_bounds2.hip: lanes that took different rows of a load instruction hold
// partial counters of the same columns)
// a += b (the sum fits NP planes: partial counts of disjoint rows of a query with t < 2^NP)
template <int NP>
RTX_HD void planes_add(uint32_t (&a)[NP], const uint32_t (&b)[NP]) {
    uint32_t c = a[0] & b[0];
    a[0] ^= b[0];
#pragma unroll
    for (int p = 1; p < NP; p++) {
        uint32_t sum, carry;
        csa(a[p], b[p], c, sum, carry);
        a[p] = sum;
        c = carry;
    }
}
// the largest of the 32 counters of a bit-sliced word, and the counters that hold it (bit by bit from the top)
template <int NP>
RTX_HD uint32_t planes_max(const uint32_t (&r)[NP], uint32_t &cand) {
    uint32_t m = 0;
    cand = 0xFFFFFFFFu;
#pragma unroll
    for (int p = NP - 1; p >= 0; p--) {
        const uint32_t x = cand & r[p];
        const bool nz = x != 0u;
        cand = nz ? x : cand;
        m |= nz ? 1u << p : 0u;
    }
    return m;
}

// bit r: counter r of the bit-sliced word is > c (c < 2^NP) -- a comparison with a constant from the top plane down, ~3 operations
// per plane (rec_epilogue, rtx_hit_common.hpp: the candidates above a pruned query's threshold)
template <int NP>
RTX_HD uint32_t planes_gt(const uint32_t (&pl)[NP], uint32_t c) {
    uint32_t gt = 0, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int b = NP - 1; b >= 0; b--) {
        const uint32_t cb = (c >> b) & 1u ? 0xFFFFFFFFu : 0u;  // scalar
        gt |= eq & pl[b] & ~cb;
        eq &= ~(pl[b] ^ cb);
    }
    return gt;
}

// Spreads the 4 bits x[3:0] into the low bit of the 4 bytes of the result.
RTX_HD uint32_t spread4(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(x & 0xFu, 0x00204081u) & 0x01010101u;  // v_mul_u32_u24 is full rate, v_mul_lo_u32 is not
#else
    return ((x & 0xFu) * 0x00204081u) & 0x01010101u;
#endif
}

// Counters of references 4g..4g+3 of a 32-reference word: low 8 bits of each counter in
// the bytes of `lo`, bits 8.. in the bytes of `hi`.
template <int NP>
RTX_HD void planes_unpack4(const uint32_t (&pl)[NP], int g, uint32_t &lo, uint32_t &hi) {
    lo = 0;
    hi = 0;
#pragma unroll
    for (int p = 0; p < NP; p++) {
        uint32_t s = spread4(pl[p] >> (4 * g));
        if (p < 8) lo |= s << p;
        else hi |= s << (p - 8);
    }
}

// Counters of references 8b..8b+7 of a 32-reference word (byte b of every plane) at once: the low 8 bits of the
// counters of references 8b..8b+3 in the bytes of lo0, of 8b+4..8b+7 in lo1, bits 8.. in hi0 / hi1 (as
// planes_unpack4 gives them for g = 2b and 2b+1).  The low eight planes are an 8 x 8 bit matrix per reference group --
// byte p = plane p, bit j = reference j -- and transposing it costs 6 byte gathers + 22 bit operations for eight
// references, against 64 for the nibble-spreading multiplies of planes_unpack4; the planes above come from those.
RTX_HD uint32_t pick_bytes(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int by) {  // byte `by` of a, b, c, d -> bytes 0..3
#if defined(__HIP_DEVICE_COMPILE__)
    // v_perm_b32(hi, lo, sel): selector byte 0-3 = byte of lo, 4-7 = byte of hi
    const uint32_t s2 = 0x0C0C0000u | (uint32_t)by | ((uint32_t)(by + 4) << 8);  // bytes: lo.by, hi.by, 0, 0
    const uint32_t ab = __builtin_amdgcn_perm(b, a, s2), cd = __builtin_amdgcn_perm(d, c, s2);
    return __builtin_amdgcn_perm(cd, ab, 0x05040100u);                           // ab.b0, ab.b1, cd.b0, cd.b1
#else
    const int sh = 8 * by;
    return ((a >> sh) & 0xFFu) | (((b >> sh) & 0xFFu) << 8) | (((c >> sh) & 0xFFu) << 16) | (((d >> sh) & 0xFFu) << 24);
#endif
}

template <int NP>
RTX_HD void planes_unpack8(const uint32_t (&pl)[NP], int b, uint32_t &lo0, uint32_t &hi0, uint32_t &lo1, uint32_t &hi1) {
    static_assert(NP >= 8, "at least eight planes");
    uint32_t x0 = pick_bytes(pl[0], pl[1], pl[2], pl[3], b);  // 64-bit matrix x1:x0, row (byte) p = plane p
    uint32_t x1 = pick_bytes(pl[4], pl[5], pl[6], pl[7], b);
    // 8 x 8 bit transpose (three delta swaps; the first two stay inside the halves)
    uint32_t t0 = (x0 ^ (x0 >> 7)) & 0x00AA00AAu, t1 = (x1 ^ (x1 >> 7)) & 0x00AA00AAu;
    x0 ^= t0 ^ (t0 << 7);
    x1 ^= t1 ^ (t1 << 7);
    t0 = (x0 ^ (x0 >> 14)) & 0x0000CCCCu;
    t1 = (x1 ^ (x1 >> 14)) & 0x0000CCCCu;
    x0 ^= t0 ^ (t0 << 14);
    x1 ^= t1 ^ (t1 << 14);
    const uint32_t t = (x0 ^ ((x0 >> 28) | (x1 << 4))) & 0xF0F0F0F0u;
    x0 ^= t ^ (t << 28);
    x1 ^= t >> 4;
    lo0 = x0;  // byte j = the low eight counter bits of reference 8b + j
    lo1 = x1;
    hi0 = 0;
    hi1 = 0;
#pragma unroll
    for (int p = 8; p < NP; p++) {
        hi0 |= spread4(pl[p] >> (8 * b)) << (p - 8);
        hi1 |= spread4(pl[p] >> (8 * b + 4)) << (p - 8);
    }
}

// v_perm_b32(hi, lo, sel): byte k of the result is byte sel[k] of the eight bytes hi:lo (0-3 = lo, 4-7 = hi; 0x0C = the constant 0)
RTX_HD uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t s = (sel >> (8 * k)) & 0xFFu;
        if (s < 8u) r |= (uint32_t)((v >> (8 * s)) & 0xFFu) << (8 * k);
    }
    return r;
#endif
}

// The low eight planes of a whole 32-reference word at once: lo[b][h] = what planes_unpack8 gives as lo0 (h = 0) / lo1 (h = 1) for
// byte b.  Three delta swaps BETWEEN the plane registers (plane bit p_k against reference bit r_k: two shifts and two bit-field
// inserts per pair of registers) leave register r with the counts of references 8b + r in its bytes b; two rounds of byte
// gathers then bring the counts of references 8b + 4h .. + 3 together: 48 + 16 operations for 32 references, where four calls of
// planes_unpack8 take 112 (the dense epilogue unpacks every word of a tile: a quarter of its instructions were this).
RTX_HD void delta_swap_regs(uint32_t &a, uint32_t &b, int s, uint32_t m) {  // a takes b's elements at m into m << s, b takes a's at m << s into m
    const uint32_t na = (a & m) | ((b & m) << s), nb = ((a >> s) & m) | (b & ~m);
    a = na;
    b = nb;
}
template <int NP>
RTX_HD void planes_unpack32(const uint32_t (&pl)[NP], uint32_t (&lo)[4][2]) {
    static_assert(NP >= 8, "at least eight planes");
    uint32_t r[8];
#pragma unroll
    for (int p = 0; p < 8; p++) r[p] = pl[p];
#pragma unroll
    for (int p = 0; p < 4; p++) delta_swap_regs(r[p], r[p + 4], 4, 0x0F0F0F0Fu);
#pragma unroll
    for (int p = 0; p < 8; p++)
        if (!(p & 2)) delta_swap_regs(r[p], r[p + 2], 2, 0x33333333u);
#pragma unroll
    for (int p = 0; p < 8; p += 2) delta_swap_regs(r[p], r[p + 1], 1, 0x55555555u);
    // r[j] byte b = the count of reference 8b + j
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint32_t x0 = byte_perm(r[4 * h + 1], r[4 * h], 0x05010400u), x1 = byte_perm(r[4 * h + 1], r[4 * h], 0x07030602u);
        const uint32_t y0 = byte_perm(r[4 * h + 3], r[4 * h + 2], 0x05010400u), y1 = byte_perm(r[4 * h + 3], r[4 * h + 2], 0x07030602u);
        lo[0][h] = byte_perm(y0, x0, 0x05040100u);
        lo[1][h] = byte_perm(y0, x0, 0x07060302u);
        lo[2][h] = byte_perm(y1, x1, 0x05040100u);
        lo[3][h] = byte_perm(y1, x1, 0x07060302u);
    }
}
// the planes above the eighth, as planes_unpack8 gives them (hi0 / hi1 for byte b)
template <int NP>
RTX_HD void planes_unpack8_hi(const uint32_t (&pl)[NP], int b, uint32_t &hi0, uint32_t &hi1) {
    hi0 = 0;
    hi1 = 0;
#pragma unroll
    for (int p = 8; p < NP; p++) {
        hi0 |= spread4(pl[p] >> (8 * b)) << (p - 8);
        hi1 |= spread4(pl[p] >> (8 * b + 4)) << (p - 8);
    }
}

// ---------------------------------------------------------------------------
// prob.rs restated for the device: the reference builds ln pmf_m(i) for every distinct
// hit count m and every i in 0..=n (prob.rs:121-170), exponentiates, accumulates ln cmf,
// sums hist[m]*ln cmf over m (prob.rs:62-73) and evaluates
//     table[m] = sum_i exp(ln pmf_m(i) + prod(i) - ln cmf_m(i))        (prob.rs:74-90).
// Here pmf_m(i) = C(m+i-1,i) C(t-m+n-i-1,n-i) / C(t+n-1,n) is advanced in the linear
// domain by its exact ratio
//     pmf_m(i)/pmf_m(i-1) = (m+i-1)(n-i+1) / (i (t-m+n-i))
// starting from pmf_m(0) = exp(lnC(t-m+n-1,n) - lnC(t+n-1,n)).  Because the start can be
// far below DBL_MIN for long sequences the value is carried as v * 2^(-512 k): whenever v
// exceeds 2^100 it is rescaled (to ~2^-412, still a normal double) and k decremented.
// While k > 0 the true pmf and cmf are < 2^-412 (~1e-124); such terms are treated as 0
// (ln cmf = -inf), which is what exp() underflow does to them in the reference at a slightly
// lower threshold, and cannot matter: Z = sum_r table[count_r] >= 1.
// ---------------------------------------------------------------------------
struct PmfState {
    double v;  // scaled pmf_m(i)
    double c;  // scaled cmf_m(i) = sum_{j<=i} pmf_m(j)
    int k;     // scale exponent: true value = v * 2^(-512 k)
};

constexpr double kScaleLn = 354.89135644669199;  // 512 * ln 2
constexpr double kScaleUp = 1.2676506002282294e30;    // 2^100: rescale threshold
constexpr double kScaleDown = 7.458340731200207e-155; // 2^-512

// ln_total = lnC(t+n-1, n); lf = ln-factorial table, lf[x] = ln(x!)
RTX_HD double ln_binom_tab(const double *lf, uint32_t n, uint32_t k) { return lf[n] - lf[k] - lf[n - k]; }

RTX_HD PmfState pmf_start(const double *lf, uint32_t t, uint32_t n, uint32_t m, double ln_total) {
    // 0 < m < t.  ln pmf_m(0) = lnC(t-m+n-1, n) - ln_total  (prob.rs:143-146,158)
    double x0 = ln_binom_tab(lf, t - m + n - 1, n) - ln_total;
    PmfState s;
    s.k = 0;
    if (x0 < -600.0) {
        s.k = (int)ceil((-600.0 - x0) / kScaleLn);
        x0 += (double)s.k * kScaleLn;
    }
    s.v = exp(x0);
    s.c = s.v;
    return s;
}

// The same state started at an arbitrary index i_s (closed-form ln pmf from the table) with
// cmf := pmf, i.e. dropping sum_{j<i_s} pmf_m(j).  Callers choose i_s so that this dropped mass
// is < (i_s+1) e^-100 (every earlier pmf is below e^-100 on the rising side).
RTX_HD double ln_pmf_tab(const double *lf, uint32_t t, uint32_t n, uint32_t m, uint32_t i, double ln_total);
RTX_HD PmfState pmf_start_at(const double *lf, uint32_t t, uint32_t n, uint32_t m, uint32_t i_s, double ln_total) {
    double x0 = ln_pmf_tab(lf, t, n, m, i_s, ln_total);
    PmfState s;
    s.k = 0;
    if (x0 < -600.0) {
        s.k = (int)ceil((-600.0 - x0) / kScaleLn);
        x0 += (double)s.k * kScaleLn;
    }
    s.v = exp(x0);
    s.c = s.v;
    return s;
}

// c^h for a non-negative integer h by square-and-multiply: prod(i) of prob.rs:62-73 is kept as
// the product  prod_m cmf_m(i)^hist[m]  instead of exp(sum hist[m] ln cmf_m(i)) -- no logarithms.
// Underflow to 0 means the true value is < 1e-308: P(i) is negligible there.
RTX_HD double pow_uint(double c, uint32_t h) {
    double r = 1.0, b = c;
    while (h) {
        if (h & 1u) r *= b;
        b *= b;
        h >>= 1;
    }
    return r;
}

// cmf_m(i)^h as a factor of P(i); 0 where the true cmf is below 2^-412
RTX_HD double pmf_cmf_pow(const PmfState &s, uint32_t h) {
    if (s.k > 0 || !(s.c > 0.0)) return 0.0;
    return pow_uint(s.c, h);
}

// advance from i-1 to i (1 <= i <= n); inv[x] = 1.0/x -- a table, or (InvDiv) the division itself where a table look-up would be a
// round trip to global memory per step (the same value: the table holds 1.0 / (double)x)
struct InvDiv {
    RTX_HD double operator[](uint32_t x) const { return 1.0 / (double)x; }
};
template <class Inv>
RTX_HD void pmf_step(PmfState &s, const Inv &inv, uint32_t t, uint32_t n, uint32_t m, uint32_t i) {
    // the ratio does not depend on v: it stays off the dependent chain v -> c
    const double ratio = ((double)(m + i - 1) * inv[i]) * ((double)(n - i + 1) * inv[t - m + n - i]);
    s.v *= ratio;
    s.c += s.v;
    if (s.k > 0 && s.v > kScaleUp) {
        s.v *= kScaleDown;
        s.c *= kScaleDown;
        s.k -= 1;
    }
}

RTX_HD double neg_inf() { return -INFINITY; }

// ln cmf, or -inf where the true value is below 2^-512 (or exactly 0)
RTX_HD double pmf_ln_cmf(const PmfState &s) {
    if (s.k > 0 || !(s.c > 0.0)) return neg_inf();
    return log(s.c);
}

// ---------------------------------------------------------------------------
// Work pruning of prob_table (all bounds are rigorous; Z >= 1 makes absolute errors of
// 1e-18 per reference irrelevant at the 1e-6 parity tolerance):
//  * i_lo: with M the largest hit count present, prod(i) <= ln cmf_M(i), and for i below the
//    mode cmf_M(i) <= (i+1) pmf_M(i).  Every i with ln pmf_M(i) < -100 on the rising side
//    therefore has exp(prod(i)) < e^-94: P(i) is taken as 0 and neither ln cmf nor the
//    pass-2 terms are evaluated there.
//  * group skip: a group of lanes whose largest count m_hi has its mode below i_lo and
//    (n-i_lo+1) pmf_{m_hi}(i_lo) < 1e-18 has cmf_m(i) >= 1 - 1e-18 for every i >= i_lo
//    (ln cmf = 0 to 1e-18) and pass-2 terms < 1e-18: the group is skipped (table[m] = 0).
//  * saturation: once cmf stops changing (pmf < 2^-53 cmf, past the mode) ln cmf is constant
//    and the remaining pass-2 terms are < 1e-16 pmf-sums: the lane group stops.
// ---------------------------------------------------------------------------
constexpr double kLnNegligibleP = -100.0;            // ln pmf_M(i) below this (rising side) => P(i) := 0
constexpr double kLnTailSkip = -41.446531673892822;  // ln 1e-18

// ln pmf_m(i), closed form (the `pmf` helper of the reference's tests, prob.rs:178-206), 0 < m < t
RTX_HD double ln_pmf_tab(const double *lf, uint32_t t, uint32_t n, uint32_t m, uint32_t i, double ln_total) {
    return ln_binom_tab(lf, m + i - 1, i) + ln_binom_tab(lf, t - m + n - i - 1, n - i) - ln_total;
}

// true if the lane group whose largest count is m_hi (> 0) contributes nothing for i >= i_lo
RTX_HD bool group_negligible(const double *lf, uint32_t t, uint32_t n, uint32_t m_hi, uint32_t i_lo, double ln_total) {
    if (i_lo == 0) return false;
    // pmf_{m_hi} must already be falling at i_lo: (m+i-1)(n-i+1) < i (t-m+n-i)
    const double up = (double)(m_hi + i_lo - 1) * (double)(n - i_lo + 1);
    const double dn = (double)i_lo * (double)(t - m_hi + n - i_lo);
    if (!(up < dn)) return false;
    return log((double)(n - i_lo + 1)) + ln_pmf_tab(lf, t, n, m_hi, i_lo, ln_total) < kLnTailSkip;
}

// Budget of the tile pruning (rtx_prune.hip): every probability and every sum of probabilities over any set of references moves by at
// most 2 (alpha + beta + gamma) / min(Z, Z') <= 4 eps (each of the three terms is held to eps / 2 or eps by the criteria, Z >= 1 - 2 eps).
// Round 3 ran with eps = 1e-12; eps = 1e-10 (round 4; worth ~12 counts of threshold at t ~ 640) puts that bound at 4e-10: a factor of 2.5
// under the 1e-9 the parity tests and bench.py's parity_sample assert, three and a half orders of magnitude under north_star's 1e-6; what the
// suites measure is 1e-11 .. 2e-11 (the criteria price every dropped reference at the threshold, real ones lie far below it).  A
// whole-database handle uses the tile-aware criterion (4), a reference shard criterion (3): the two arrive at different thresholds for the
// same query, so a replicated and a sharded run of one batch agree within this budget, not bit for bit.
constexpr double kPruneEpsHD = 1e-10;
constexpr double kPruneLnEpsHD = -23.025850929940457;  // ln 1e-10
constexpr double kPruneHalfEpsHD = 0.5e-10;
constexpr uint32_t kPruneFarGap = 40;    // tile-aware threshold: groups of tiles whose bound lies this far below the threshold of (2) are priced together
constexpr uint32_t kPruneMaxNear = 12;   // ... unless more groups than this lie nearer: then every group gets the value of its own bound

// ---------------------------------------------------------------------------
// Tile pruning, the tile-aware criterion (rtx_prune.hip, "(4)"): the window sums  S_A(m) = sum_l pmf_m(i1 + l) WA(l)  and
// S_B(m) = sum_l pmf_m(i1 + l) WB(l)  over l = 0 .. 63 (i1 + l <= n) for ONE count m, pmf_m advanced by its exact ratio
//     pmf_m(i + 1) / pmf_m(i) = (m + i)(n - i) / ((i + 1)(t - m + n - i - 1))
// from exp(ln pmf_m(i1)) (clamped from below at e^-700: a larger start only makes the criterion stricter).  In the kernel a lane
// runs this loop for the largest bound of its group of tiles; `wa(l)`, `wb(l)` hand out the weights of lane l (v_readlane there,
// array reads in the emulation).  m = 0: pmf_0 is the point mass at i = 0 < i1, both sums are 0.
// ---------------------------------------------------------------------------
template <class WAf, class WBf>
RTX_HD void prune_window_sums(const double *lf, const double *inv, uint32_t t, uint32_t n, uint32_t m, uint32_t i1, double ln_total,
                              WAf wa, WBf wb, double &sa, double &sb) {
    sa = 0.0;
    sb = 0.0;
    const bool ok = m != 0u && m < t;   // (no early exit: in the kernel the loop below is wave-uniform, the weights come by v_readlane)
    const uint32_t ms = ok ? m : 1u;
    double x0 = ln_pmf_tab(lf, t, n, ms, i1, ln_total);
    if (x0 < -700.0) x0 = -700.0;
    double P = ok ? exp(x0) : 0.0;
    for (uint32_t l = 0; l < 64u && i1 + l <= n; l++) {
        sa += P * wa(l);
        sb += P * wb(l);
        const uint32_t i = i1 + l;  // -> i + 1 (unused behind the last step)
        if (i < n) P *= ((double)(ms + i) * inv[i + 1u]) * ((double)(n - i) * inv[t - ms + n - i - 1u]);
    }
}

// prob.rs:105-119 with the table
RTX_HD double only_last_pmf_tab(const double *lf, uint32_t t, uint32_t n, uint32_t m, double ln_total) {
    if (m == t) return 1.0;
    if (m == 0) return 0.0;
    return exp(ln_binom_tab(lf, m + n - 1, n) - ln_total);
}

// ---------------------------------------------------------------------------
// Finalisation of the result rows of one query (lineage.rs:91-110, utils.rs:91-105), shared by finalise_kernel (rtx_finalise.hip)
// and the x86 emulation of the CPU tests.  A row arrives as {node, confidence per level in hundredths} (DevRow); its depth is the
// node's.  Every operation is a correctly rounded IEEE one in a fixed order and nothing is contracted into an FMA, so the
// device writes the doubles a host loop over the same rows writes.
// ---------------------------------------------------------------------------
// Does row x come before row y?  lineage.rs:91-93 sorts descending by confidence vector, a shorter prefix being the smaller one
// (Vec<f64> partial_cmp); the sort is stable: equal rows keep the order of the walk (ix, iy = their positions in it).  The
// hundredths order like the values they stand for.
RTX_HD bool fin_row_before(const uint8_t *kx, uint32_t dx, uint32_t ix, const uint8_t *ky, uint32_t dy, uint32_t iy) {
    const uint32_t n = dx < dy ? dx : dy;
    for (uint32_t d = 0; d < n; d++)
        if (kx[d] != ky[d]) return kx[d] > ky[d];
    if (dx != dy) return dx > dy;
    return ix < iy;
}
// The same on whole words (finalise_kernel's rank loop: a query of real barcodes can have two hundred rows, and a compare byte by byte from
// LDS was what the kernel spent its time on).  kx, ky: the rows' hundredths as big-endian words (level 0 in the top byte), ZERO beyond the
// row's depth (the walk writes them so).  The first differing byte decides as in fin_row_before when it lies inside the common prefix; beyond
// it the shorter row holds padding and the longer row the larger number -- the longer row is the larger one there too.  Equal numbers: the
// common prefix is equal, the depths decide, then the positions.
RTX_HD bool fin_row_before_words(const uint32_t *kx, uint32_t dx, uint32_t ix, const uint32_t *ky, uint32_t dy, uint32_t iy, uint32_t kw) {
    for (uint32_t w = 0; w < kw; w++)
        if (kx[w] != ky[w]) return kx[w] > ky[w];
    if (dx != dy) return dx > dy;
    return ix < iy;
}
RTX_HD uint32_t fin_be32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// Local signal of a row (lineage.rs:95-102): the euclidean distance (utils.rs:91-105: both vectors scaled to a sum of one) between the
// confidences and the expected shares |range of the ancestor| / N (lineage.rs:137-139), from the first level on whose expected share is
// below one (the last level if there is none).  The expected side depends on the node alone and is tabulated per node:
// fin_node_expected gives s0 and eb[d] = e[d] / sum of e from s0 on (0 in front of s0); size[d] = references below the ancestor at level d.
RTX_HD uint32_t fin_node_expected(const uint32_t *size, uint32_t depth, double n_total, double *eb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (depth == 0) return 0;
    uint32_t s0 = depth - 1u;
    for (uint32_t d = 0; d < depth; d++)
        if (1.0 > (double)size[d] / n_total) { s0 = d; break; }
    double b_sum = 0.0;
    for (uint32_t d = s0; d < depth; d++) b_sum += (double)size[d] / n_total;
    for (uint32_t d = 0; d < depth; d++) eb[d] = d < s0 ? 0.0 : ((double)size[d] / n_total) / b_sum;
    return s0;
}
// k(d): the row's hundredths at level d (an accessor: the kernel reads them from its staged words, the emulation from bytes).  The table
// entries of four levels are requested together (what a row waits for on the device is the chain of its loads, not its arithmetic); the
// additions keep the order of utils.rs:91-105.
template <class K>
RTX_HD double fin_local_signal(K k, const double *eb, uint32_t s0, uint32_t depth) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (depth == 0) return 0.0;
    double a_sum = 0.0;
    for (uint32_t d = s0; d < depth; d++) a_sum += (double)k(d) / 100.0;
    double s = 0.0;
    for (uint32_t d = s0; d < depth; d += 4u) {
        double e[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) e[u] = d + u < depth ? eb[d + u] : 0.0;
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            if (d + u < depth) {
                const double x = ((double)k(d + u) / 100.0) / a_sum - e[u];
                const double xx = x * x;
                s = s + xx;
            }
        }
    }
    return sqrt(s);
}

// ---------------------------------------------------------------------------
// Result text (rtx_text.hip), byte for byte what rtx_format_query (host_format.cpp) prints: lineage.rs:17-48, utils.rs:62-89.
// The generators below write through a sink S with put(char) and put_gen(n, f) (n bytes, byte i = f(i)): TextCount only counts
// (the measure pass), TextWindow keeps the bytes that fall into a window of the text (the write pass: a wave fills a window in LDS and
// stores it with wide stores; the host emulation takes one window as large as the text).
// ---------------------------------------------------------------------------
struct TextCount {
    uint64_t pos = 0;
    RTX_HD void put(char) { pos++; }
    template <class F>
    RTX_HD void put_gen(uint64_t n, F) { pos += n; }
};
struct TextWindow {
    char *buf;            // buf[i] holds byte w0 + i of the text
    uint64_t pos, w0, w1;  // bytes [w0, w1) of the text are kept
    RTX_HD void put(char c) {
        if (pos >= w0 && pos < w1) buf[pos - w0] = c;
        pos++;
    }
    template <class F>
    RTX_HD void put_gen(uint64_t n, F f) {
        const uint64_t lo = pos > w0 ? pos : w0, hi = pos + n < w1 ? pos + n : w1;
        for (uint64_t i = lo; i < hi; i++) buf[i - w0] = f(i - pos);
        pos += n;
    }
};

// decimal digits of v (v > 0), most significant first
template <class S>
RTX_HD void text_put_u64(S &s, uint64_t v) {
    uint32_t nd = 1;
    for (uint64_t p = 10; nd < 20 && v >= p; p *= 10) nd++;
    uint64_t div = 1;
    for (uint32_t i = 1; i < nd; i++) div *= 10;
    for (uint32_t i = 0; i < nd; i++) {
        s.put((char)('0' + v / div % 10));
        div /= 10;
    }
}

// the integer part of a double of 2^64 or more: m * 2^e exactly, in 32-bit limbs, nine digits at a time (what printf prints for it)
template <class S>
RTX_HD void text_put_big_int(S &s, double v) {
    int e2 = 0;
    const double fr = frexp(v, &e2);                      // v = fr * 2^e2, fr in [0.5, 1)
    uint64_t m = (uint64_t)ldexp(fr, 53);                 // v = m * 2^(e2 - 53), exactly
    const int sh = e2 - 53;                               // >= 11 here
    uint32_t limb[34] = {0};                              // 1088 bits
    const int w = sh / 32, b = sh % 32;
    limb[w] = (uint32_t)(m << b);
    limb[w + 1] = (uint32_t)(m >> (32 - b));
    limb[w + 2] = b ? (uint32_t)(m >> (64 - b)) : 0u;
    uint32_t chunk[40];
    int nc = 0, top = 33;
    while (top >= 0) {
        while (top >= 0 && limb[top] == 0) top--;
        if (top < 0) break;
        uint64_t rem = 0;
        for (int i = top; i >= 0; i--) {
            const uint64_t cur = rem << 32 | limb[i];
            limb[i] = (uint32_t)(cur / 1000000000u);
            rem = cur % 1000000000u;
        }
        chunk[nc++] = (uint32_t)rem;
    }
    text_put_u64(s, chunk[nc - 1]);
    for (int i = nc - 2; i >= 0; i--)
        for (uint32_t d = 100000000u; d; d /= 10) s.put((char)('0' + chunk[i] / d % 10));
}

// "{:.5}" (Rust) = "%.5f" (printf) of any double: the exact binary value rounded half to even at five decimals.  The integer part I = floor|v|
// and the fraction F = |v| - I are exact; p = F * 1e5 is rounded, and fma(F, 1e5, -p) is its exact residual: the distance of F * 1e5 to
// the half-way point between two integers is decided on exact values (no case is too close to call).  Non-finite: printf's "inf", "nan".
template <class S>
RTX_HD void text_put_fix5(S &s, double v) {
    const bool neg = std::signbit(v);
    if (std::isnan(v)) { if (neg) s.put('-'); s.put('n'); s.put('a'); s.put('n'); return; }
    if (neg) s.put('-');
    if (std::isinf(v)) { s.put('i'); s.put('n'); s.put('f'); return; }
    const double a = fabs(v);
    double I = floor(a);
    const double F = a - I;
    const double p = F * 1e5, e = fma(F, 1e5, -p);  // F * 1e5 = p + e exactly
    const double n = floor(p), f = p - n;           // F * 1e5 = n + f + e, f in [0, 1)
    bool up = false;
    if (f >= 0.25) {  // f - 0.5 is exact from here on (Sterbenz); |e| <= 2^-37
        const double d = f - 0.5;
        up = d > -e || (d == -e && fmod(n, 2.0) != 0.0);
    }
    uint32_t r = (uint32_t)n + (up ? 1u : 0u);
    if (r >= 100000u) { r -= 100000u; I += 1.0; }  // (F < 1 - 2^-53: only below 2^53, where I + 1 is exact)
    if (I < 18446744073709551616.0) text_put_u64(s, (uint64_t)I);
    else text_put_big_int(s, I);
    s.put('.');
    for (uint32_t d = 10000u; d; d /= 10u) s.put((char)('0' + r / d % 10u));
}

// "{:.2}" of a confidence given as hundredths (k / 100.0 of lineage.rs:128-129: the value k/100 rounded at two decimals is k)
template <class S>
RTX_HD void text_put_hund(S &s, uint32_t k) {
    text_put_u64(s, k / 100u);
    s.put('.');
    s.put((char)('0' + k / 10u % 10u));
    s.put((char)('0' + k % 10u));
}

// One result row.  ones: the single-exact-match override (raxtax.rs:73-84): every level 1.00.
struct TextRow {
    const char *label;
    uint64_t label_len;
    const char *lin;
    uint64_t lin_len;
    const uint8_t *hund;  // hundredths per level
    uint32_t depth;
    bool ones;
    double local, global;
};

// `.out` line (lineage.rs:17-29): label \t lineage \t c,c,...,c \t local \t global
template <class S>
RTX_HD void text_out_row(S &s, const TextRow &r) {
    s.put_gen(r.label_len, [&](uint64_t i) { return r.label[i]; });
    s.put('\t');
    s.put_gen(r.lin_len, [&](uint64_t i) { return r.lin[i]; });
    s.put('\t');
    for (uint32_t d = 0; d < r.depth; d++) {
        if (d) s.put(',');
        text_put_hund(s, r.ones ? 100u : r.hund[d]);
    }
    s.put('\t');
    text_put_fix5(s, r.local);
    s.put('\t');
    text_put_fix5(s, r.global);
}

// base code -> letter (utils.rs:70-81)
RTX_HD char text_base(uint8_t b) { return b == 1 ? 'A' : (b == 2 ? 'C' : (b == 4 ? 'G' : (b == 8 ? 'T' : '-'))); }

// `.tsv` line (lineage.rs:31-48): label, then the levels of the lineage interleaved with the confidences (the longer side drained),
// local, global, the decoded sequence; tab-separated.  base(i): code of base i of the query.
template <class S, class B>
RTX_HD void text_tsv_row(S &s, const TextRow &r, uint64_t seq_len, B base) {
    s.put_gen(r.label_len, [&](uint64_t i) { return r.label[i]; });
    s.put('\t');
    uint64_t pos = 0;
    uint32_t d = 0;
    bool lin_done = false, first = true;
    while (!lin_done || d < r.depth) {
        if (!lin_done) {
            uint64_t c = pos;
            while (c < r.lin_len && r.lin[c] != ',') c++;
            if (!first) s.put('\t');
            const char *lv = r.lin + pos;
            s.put_gen(c - pos, [&](uint64_t i) { return lv[i]; });
            first = false;
            if (c >= r.lin_len) lin_done = true;
            else pos = c + 1;
        }
        if (d < r.depth) {
            if (!first) s.put('\t');
            text_put_hund(s, r.ones ? 100u : r.hund[d]);
            first = false;
            d++;
        }
    }
    s.put('\t');
    text_put_fix5(s, r.local);
    s.put('\t');
    text_put_fix5(s, r.global);
    s.put('\t');
    s.put_gen(seq_len, [&](uint64_t i) { return text_base(base(i)); });
}

// Where the rows of a query's text come from: the lineage table (bytes of tree.lineages back to back, offsets, levels = commas + 1) and the
// final rows of a download (rtx_result_view: lineage, depth, hundredths [row][D], local signal).
struct TextSrc {
    const char *lin_bytes;
    const uint64_t *lin_off;
    const uint8_t *lin_depth;
    const uint32_t *row_lineage;
    const uint8_t *row_depth, *row_hund;
    const double *row_local;
    uint32_t D;
};
constexpr uint32_t kTextNoOverride = 0xFFFFFFFFu;

// Row i of a query whose rows start at r0.  one != kTextNoOverride: the id of the query's only exact match, which replaces the rows
// (raxtax.rs:73-84): its lineage, 1.00 on each of its levels, the local signal of the first row.
RTX_HD TextRow text_row(const TextSrc &t, const char *label, uint64_t label_len, uint64_t r0, uint64_t i, uint32_t one, double global) {
    TextRow r;
    r.label = label;
    r.label_len = label_len;
    r.ones = one != kTextNoOverride;
    const uint32_t li = r.ones ? one : t.row_lineage[r0 + i];
    r.lin = t.lin_bytes + t.lin_off[li];
    r.lin_len = t.lin_off[li + 1] - t.lin_off[li];
    r.depth = r.ones ? t.lin_depth[li] : t.row_depth[r0 + i];
    r.hund = t.row_hund + (r0 + i) * t.D;
    r.local = t.row_local[r0 + (r.ones ? 0 : i)];
    r.global = global;
    return r;
}

// ---------------------------------------------------------------------------
// Taxon profile (rtx_profile.hip): what one query adds.  Its BEST LINEAGE is the one `.out` prints first -- the Taxon leaf of its only
// exact match with 1.00 on every level where the override of raxtax.rs:73-84 applies (one != kTextNoOverride), else its first row.  The path
// a_0 .. a_{depth-1} runs from the child of the root down to that node; L = the leading levels whose hundredths reach the cutoff.  The
// query counts under a_0 .. a_{L-1} (clade, conf_sum) and ends at a_{L-1} (direct).
// ---------------------------------------------------------------------------
struct ProfileSrc {
    const uint8_t *status;                 // [queries] the per-query fields of the chosen orientation
    const uint32_t *row_count;
    const unsigned long long *row_begin;
    const uint32_t *row_node;              // the final rows (rtx_result_view)
    const uint8_t *row_depth, *row_hund;
    uint32_t D;
    const uint32_t *parent;                // [n_nodes] rtx_nodes_view numbering; the root has none
    const uint8_t *node_depth;             // [n_nodes]
    const uint32_t *ref_leaf;              // [n_refs] the Taxon node of a reference's own lineage
    uint32_t n_nodes, n_refs;
};
constexpr uint32_t kProfUnclassifiable = 0u, kProfUnclassified = 1u, kProfClassified = 2u;
struct ProfileStep {
    uint32_t kind;        // kProf*
    uint32_t node, L;     // a_{L-1} and L (classified only)
    const uint8_t *hund;  // hundredths per level of the best lineage; null: 100 on every level (the override)
    RTX_HD uint32_t at(uint32_t d) const { return hund ? hund[d] : 100u; }
};
RTX_HD ProfileStep profile_step(const ProfileSrc &s, uint64_t q, uint32_t one, uint32_t cutoff) {
    ProfileStep r{kProfUnclassifiable, 0u, 0u, nullptr};
    if (s.status[q] != 0 || s.row_count[q] == 0u) return r;  // (0: RTX_Q_OK)
    uint32_t node, depth;
    if (one != kTextNoOverride && one < s.n_refs) {
        node = s.ref_leaf[one];
        depth = node < s.n_nodes ? s.node_depth[node] : 0u;
    } else {
        const uint64_t row = s.row_begin[q];
        node = s.row_node[row];
        depth = s.row_depth[row];
        r.hund = s.row_hund + row * s.D;
    }
    uint32_t L = 0;
    while (L < depth && r.at(L) >= cutoff) L++;
    r.kind = L ? kProfClassified : kProfUnclassified;
    r.L = L;
    for (uint32_t d = depth; d > L && L && node < s.n_nodes; d--) node = s.parent[node];  // a_{depth-1} -> a_{L-1}
    r.node = node;
    return r;
}

// ---------------------------------------------------------------------------
// Chimera check (rtx_chimera.hip; rtx_chimera_read on the host; emul_chimera_* on x86) -- include/raxtax_hip.h has the definition.  Exact
// integers.  A read of n_pos windows is cut into S segments at b_s = floor(s n_pos / S); the scan kernel folds the bitmap rows of the
// windows in position order and looks at the planes after every segment (a checkpoint), so every segment of the row list is padded with
// the zero row to a multiple of eight rows: a checkpoint then falls between two fold groups.  Two lists per read: direction 0 holds the
// segments 0 .. S-1 (checkpoint k: P[k + 1]), direction 1 the segments S-1 .. 0 (checkpoint k: Suf[S - 1 - k]).
// ---------------------------------------------------------------------------
constexpr uint32_t kChimMaxSegments = 32u;     // RTX_CHIMERA_MAX_SEGMENTS
constexpr uint32_t kChimMaxQuery = 4096u;      // RTX_CHIMERA_MAX_QUERY: n_pos <= 4089 fits twelve planes
constexpr uint32_t kChimNoRef = 0xFFFFFFFFu;   // RTX_NO_REF
constexpr uint32_t kChimOk = 0u, kChimNoKmer = 1u, kChimTooLong = 2u;  // RTX_CHIM_*
constexpr uint32_t kChimListTail = 192u;       // zero rows behind a list: what the scan's look-ahead loads reach (chimera_scan_kernel)
RTX_HD uint32_t chimera_n_pos(uint32_t len) { return len > kChimMaxQuery || len < 8u ? 0u : len - 7u; }
RTX_HD uint32_t chimera_boundary(uint32_t n_pos, uint32_t S, uint32_t s) { return s * n_pos / S; }  // (s n_pos <= 32 * 4089)
// segment of direction `dir`'s k-th place
RTX_HD uint32_t chimera_seg_at(uint32_t S, uint32_t dir, uint32_t k) { return dir ? S - 1u - k : k; }
// off[k]: the first row of the k-th segment of direction `dir` in its list, off[S]: the rows of the list (a multiple of 8)
RTX_HD uint32_t chimera_layout(uint32_t n_pos, uint32_t S, uint32_t dir, uint32_t *off /*[S + 1]*/) {
    uint32_t at = 0;
    for (uint32_t k = 0; k < S; k++) {
        const uint32_t s = chimera_seg_at(S, dir, k);
        off[k] = at;
        at += (chimera_boundary(n_pos, S, s + 1u) - chimera_boundary(n_pos, S, s) + 7u) & ~7u;
    }
    off[S] = at;
    return at;
}
// rows of a list whatever the direction, and the entries a list of it is allotted (the tail, to whole groups of 64)
RTX_HD uint32_t chimera_list_rows(uint32_t n_pos, uint32_t S) {
    uint32_t at = 0;
    for (uint32_t s = 0; s < S; s++) at += (chimera_boundary(n_pos, S, s + 1u) - chimera_boundary(n_pos, S, s) + 7u) & ~7u;
    return at;
}
RTX_HD uint32_t chimera_list_cap(uint32_t rows) { return ((rows + 63u) & ~63u) + kChimListTail; }
// the window that entry j of direction `dir`'s list holds, or kChimNoRef: padding (off: chimera_layout of that direction)
RTX_HD uint32_t chimera_list_window(uint32_t n_pos, uint32_t S, uint32_t dir, const uint32_t *off, uint32_t j) {
    if (j >= off[S]) return kChimNoRef;
    uint32_t k = 0;
    while (k + 1u < S && off[k + 1u] <= j) k++;
    const uint32_t s = chimera_seg_at(S, dir, k);
    const uint32_t b0 = chimera_boundary(n_pos, S, s), b1 = chimera_boundary(n_pos, S, s + 1u);
    const uint32_t i = b0 + (j - off[k]);
    return i < b1 ? i : kChimNoRef;
}
// One lane's part of a checkpoint: the largest of its 128 counters and the lowest local reference of the tile that holds it (ref_slot
// inverted: bit b of word w of lane l is group g = 4 w + b / 8, local reference (g L + l) 8 + b % 8 -- ascending in (w, b)).
template <int NP>
RTX_HD void chimera_lane_best(const uint32_t (&pl)[4][NP], uint32_t lane, uint32_t L, uint32_t &m, uint32_t &rl) {
    m = 0;
    rl = kChimNoRef;
#pragma unroll
    for (int w = 0; w < 4; w++) {  // word by word (one candidate mask alive at a time): a later word wins only with a larger count
        uint32_t cand;
        const uint32_t mw = planes_max<NP>(pl[w], cand);
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t b = (uint32_t)__ffs((int)cand) - 1u;
#else
        const uint32_t b = (uint32_t)__builtin_ctz(cand);  // (planes_max never leaves cand empty)
#endif
        const uint32_t r = (((uint32_t)w * 4u + (b >> 3)) * L + lane) * 8u + (b & 7u);
        const bool take = w == 0 || mw > m;
        rl = take ? r : rl;
        m = take ? mw : m;
    }
}
// (count, reference) of one checkpoint over the tiles, in ascending order: a later tile wins only with a larger count
RTX_HD void chimera_take(uint32_t &best, uint32_t &ref, uint32_t count, uint32_t r) {
    if (count > best) { best = count; ref = r; }
}
// The record of a read from its checkpoints over all tiles: pm / pr [S + 1] = max_r P_r[s] and the lowest r (kChimNoRef where 0), sm / sr
// the same for Suf.  P[S] and Suf[0] are both `single`; the caller hands in what it has (pm[0], sm[S] are 0 by definition).
struct ChimRec { uint32_t status, n_valid, single, parent, seg, pos, left, parent_a, right, parent_b, delta, flag; };
RTX_HD ChimRec chimera_record(uint32_t len, uint32_t n_valid, uint32_t S, uint32_t mindelta, const uint32_t *pm, const uint32_t *pr,
                              const uint32_t *sm, const uint32_t *sr) {
    ChimRec r{kChimOk, 0u, 0u, kChimNoRef, 0u, 0u, 0u, kChimNoRef, 0u, kChimNoRef, 0u, 0u};
    if (len > kChimMaxQuery) { r.status = kChimTooLong; return r; }
    if (n_valid == 0u) { r.status = kChimNoKmer; return r; }
    const uint32_t n_pos = chimera_n_pos(len);
    r.n_valid = n_valid;
    r.single = pm[S];
    r.parent = r.single ? pr[S] : kChimNoRef;
    uint32_t best = 0;
    r.seg = 1u;
    for (uint32_t s = 1; s < S; s++) {
        const uint32_t two = pm[s] + sm[s];
        if (s == 1u || two > best) { best = two; r.seg = s; }
    }
    r.pos = chimera_boundary(n_pos, S, r.seg);
    r.left = pm[r.seg];
    r.parent_a = r.left ? pr[r.seg] : kChimNoRef;
    r.right = sm[r.seg];
    r.parent_b = r.right ? sr[r.seg] : kChimNoRef;
    r.delta = best - r.single;
    r.flag = r.delta >= mindelta ? 1u : 0u;
    return r;
}
// the 8-mer of window i of a read (sequence_to_kmers' rule: all eight bases plain codes), false: not valid
RTX_HD bool chimera_window_kmer(const uint8_t *seq, uint32_t i, uint32_t &k) {
    k = 0;
    bool ok = true;
    for (uint32_t j = 0; j < 8u; j++) {
        const uint32_t c = seq[i + j];
        ok = ok && (c == 1u || c == 2u || c == 4u || c == 8u);
        k = (k << 2) | (c == 2u ? 1u : (c == 4u ? 2u : (c == 8u ? 3u : 0u)));
    }
    return ok;
}

// ---------------------------------------------------------------------------
// De novo chimera check (rtx_denovo.hip; rtx_denovo_check_host on the host; emul_denovo_* on x86) -- include/raxtax_hip.h has the definition.
// The references of entry e are the entries below lim(e) that are not flagged: a PREFIX of the entry list and a live mask.  The scan is
// chimera_scan_kernel's with every plane word ANDed, at a checkpoint, with the lane's 16 bytes of that mask: a counter that is masked out
// is 0 and never a candidate.  The stage's own bitmap has the index's layout with the row of k-mer k at k, the zero row behind the 65 536
// k-mer rows and the live mask as one more row; its stride is a multiple of 16 bytes, so the last tile may span fewer than 64 lanes.
// ---------------------------------------------------------------------------
constexpr uint32_t kDenovoNoParent = 3u;                    // RTX_DENOVO_NO_PARENT
constexpr uint32_t kDenovoZeroRow = 65536u, kDenovoLiveRow = 65537u, kDenovoRows1 = 65538u;
constexpr uint32_t kDenovoMaxTiles = 32u;                   // RTX_DENOVO_DEFAULT_MAX_PARENTS / 8192
RTX_HD uint32_t denovo_stride_bytes(uint32_t n_parents) { return (((n_parents + 7u) >> 3) + 15u) & ~15u; }
RTX_HD uint32_t denovo_tiles(uint32_t lim) { return (lim + 8191u) >> 13; }
// The prefix mask of lim in the 16 bytes of `lane` of tile `tile` (L lanes): under ref_slot byte g of the lane holds the local entries
// (g L + lane) 8 + [0, 8), so byte g is the low min(8, lim - first entry) bits, or nothing.  A lane behind the tile's last one holds nothing.
RTX_HD void denovo_allow(uint32_t lane, uint32_t L, uint32_t tile, uint32_t lim, uint32_t *out /*[4]*/) {
    const uint64_t t0 = (uint64_t)tile << 13;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const uint64_t first = t0 + (uint64_t)((w * 4u + j) * L + lane) * 8u;
            const uint32_t n = lane < L && (uint64_t)lim > first ? (uint32_t)((uint64_t)lim - first < 8u ? (uint64_t)lim - first : 8u) : 0u;
            v |= ((1u << n) - 1u) << (8u * j);
        }
        out[w] = v;
    }
}
// chimera_lane_best over the planes ANDed with allow[w], word by word: only one masked word is alive at a time
template <int NP>
RTX_HD void denovo_lane_best(const uint32_t (&pl)[4][NP], const uint32_t (&allow)[4], uint32_t lane, uint32_t L, uint32_t &m, uint32_t &rl) {
    m = 0;
    rl = kChimNoRef;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        uint32_t row[NP], cand;
#pragma unroll
        for (int b = 0; b < NP; b++) row[b] = pl[w][b] & allow[w];
        const uint32_t mw = planes_max<NP>(row, cand);
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t b = (uint32_t)__ffs((int)cand) - 1u;
#else
        const uint32_t b = (uint32_t)__builtin_ctz(cand);  // (planes_max never leaves cand empty)
#endif
        // (mw > 0: every candidate has a plane bit set, so it is allowed; mw == 0: the candidates are all 32 counters, masked ones among
        // them, but a lane whose maximum is 0 names no entry: the scan decides that by M == 0 and by the wave maximum)
        const uint32_t r = (((uint32_t)w * 4u + (b >> 3)) * L + lane) * 8u + (b & 7u);
        const bool take = w == 0 || mw > m;
        rl = take ? r : rl;
        m = take ? mw : m;
    }
}

// ---------------------------------------------------------------------------
// Denoising (unoise_pair_kernel, rtx_unoise.hip; emul_unoise_distance on x86): the global (Levenshtein) distance of a pattern x of m codes
// and a text y of n codes under a threshold k <= 16, by Hyyro's bit-vector step on a band of 64 rows that slides down the diagonal.
//   band     column j (1 .. n; column 0 is the boundary) holds the rows i = j - 31 + b, b = 0 .. 63: every cell with |i - j| <= 16 and more.
//            Rows i <= 0 are virtual, D[i][j] = j - i (column 0 is V-shaped: vn below bit 32, vp from it), which leaves D[0][j] = j; rows
//            above m match nothing and nothing above them depends on them.  The top cell of a column ignores the cell above it and the
//            cell that enters at the bottom ignores the cell to its left: the band computes the minimum over the paths that stay inside
//            it, which is >= D and equal to D wherever D <= 16 (such a path never leaves |i - j| <= 16).
//   match    the pattern's match vectors are bit rows, one per code: bit i + 31 of row c is set iff x_i == c (i from 1), so that Eq of
//            column j is the 64 bits from bit j on (unoise_eq): no shift by a negative amount, no mask at either end.
//   cut-off  the cell on the final diagonal, S_j = D[j + m - n][j], never decreases with j and ends as D[m][n]: the pair stops at the first
//            column where S_j > k.  (S_j is at least the band's minimum, so this stops no later than Ukkonen's rule.)  A computed
//            S_j > k proves D > k, a computed S_n <= k is D.
// ---------------------------------------------------------------------------
constexpr uint32_t kUnoiseMaxDiffs = 16;
constexpr uint32_t kUnoiseNoDist = 0xFFFFFFFFu;
// k(e, p) of the definition: the largest d in 0 .. max_diffs with (wp >> (alpha d + 1)) >= we
RTX_HD uint32_t unoise_allowed(uint64_t wp, uint64_t we, uint32_t alpha, uint32_t max_diffs) {
    uint32_t k = 0;
    for (uint32_t d = 1; d <= max_diffs; d++) {
        const uint32_t sh = alpha * d + 1u;
        if (sh >= 64u || (wp >> sh) < we) break;  // (the left side never grows with d)
        k = d;
    }
    return k;
}
// 64-bit words of one code's bit row for a pattern of m codes: bits up to m + 31 are the pattern's, and Eq of column n <= m + 16 reads two words
RTX_HD uint32_t unoise_peq_words(uint32_t m) { return ((m + kUnoiseMaxDiffs) >> 6) + 2u; }
RTX_HD uint32_t unoise_peq_bit(uint32_t i0) { return i0 + 32u; }  // of code i0 of the pattern, from 0
RTX_HD uint64_t unoise_eq(const uint64_t *row, uint32_t j) {
    const uint32_t w = j >> 6, s = j & 63u;
    return (row[w] >> s) | ((row[w + 1u] << 1) << (63u - s));
}
// len codes (one per byte, below 16) as sixteen to a word, the first in the low bits; words: (len + 15) / 16, the last one zero-padded
RTX_HD void unoise_pack(const uint8_t *x, uint32_t len, uint64_t *words) {
    for (uint32_t t = 0; t * 16u < len; t++) {
        uint64_t w = 0;
        for (uint32_t i = 0; i < 16u && t * 16u + i < len; i++) w |= (uint64_t)(x[t * 16u + i] & 15u) << (4u * i);
        words[t] = w;
    }
}
struct UnoiseBand {
    uint64_t vp, vn;  // vertical deltas +1 / -1 of the band's rows in the column last processed, in that column's frame
};
RTX_HD void unoise_band_init(UnoiseBand &b) {
    b.vp = 0xFFFFFFFF00000000ull;
    b.vn = 0x00000000FFFFFFFFull;
}
// One column: the band moves down by one row (the deltas move one bit down), then Hyyro's step.  Returns D0: bit b set iff the cell of
// row b equals its diagonal predecessor.
RTX_HD uint64_t unoise_step(UnoiseBand &b, uint64_t eq) {
    const uint64_t vp = b.vp >> 1, vn = b.vn >> 1;
    const uint64_t d0 = (((eq & vp) + vp) ^ vp) | eq | vn;  // (the only carry chain)
    const uint64_t hp = (vn | ~(d0 | vp)) << 1;
    const uint64_t hn = (vp & d0) << 1;
    b.vp = hn | ~(d0 | hp);
    b.vn = d0 & hp;
    return d0;
}
// d(x, y) if it is at most k, else kUnoiseNoDist.  m, n: the lengths, |m - n| <= k <= 16 (the caller's length test); eq(c, j): Eq of code c
// in column j (unoise_eq of the row of c); text_word(t): codes 16 t .. 16 t + 15 of the text.  *finished: the last column was reached.
template <class EQ, class TW>
RTX_HD uint32_t unoise_distance(uint32_t m, uint32_t n, uint32_t k, const EQ &eq, const TW &text_word, bool &finished) {
    UnoiseBand b;
    unoise_band_init(b);
    const uint64_t diag = 1ull << (m + 31u - n);  // the final diagonal in the band (a mask: no 64-bit shift by a register per column)
    uint32_t s = m > n ? m - n : n - m;           // S_0
    uint64_t word = 0;
    finished = false;
    for (uint32_t j = 1; j <= n; j++) {
        if (((j - 1u) & 15u) == 0u) word = text_word((j - 1u) >> 4);
        const uint64_t d0 = unoise_step(b, eq((uint32_t)word & 15u, j));
        word >>= 4;
        s += (d0 & diag) ? 0u : 1u;
        if (s > k) return kUnoiseNoDist;
    }
    finished = true;
    return s;
}

}  // namespace rtx

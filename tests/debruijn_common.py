"""Exact inputs for the counting kernels: every reference and every query is a window of the linearised de Bruijn sequence B(4, 8)
(65 543 bases, every 8-mer exactly once), so every hit count has a closed form and the test author decides it.

A window that holds the k-mer positions [s, s + m) is the m + 7 bases from s on.  A query [a, a + t) and a reference [s, s + m) share
exactly max(0, min(a + t, s + m) - max(a, s)) k-mers, t = len - 7 exactly (no k-mer repeats), and the references that carry a k-mer are
the windows that cover its position -- so the number of references of a (row, tile) segment, which decides whether hit_count reaches it
through the sparse slots (1 .. 16 references of a full tile) or the bitmap (17 or more; every segment of the partial last tile), is the
number of windows of the tile that cover the position.

Two lemmas let one family of windows reach every case:
  * controlled segment class: the background references are short windows of a region no query touches (positions from BG0 on), so
    the class of every row of a query in every tile is decided by the planted windows alone;
  * partial last tile: the last tile of the database is partial and has no sparse path; references are planted there too.

The lineages come in sorted order (fixed-width names), so the tree keeps the database order: local reference 8 j + i of a tile is
byte i of group j of the epilogue's stores (ref_slot, rtx_math.hpp)."""
from __future__ import annotations

import functools

import numpy as np

TILE = 8192
BG0 = 24_000            # k-mer positions from here on belong to the background; queries and planted windows stay below
N_POS = 65_536          # k-mer positions of the sequence
PER_TAXON = 64          # references per leaf taxon: 513 leaf taxa in 4 tiles + 37


@functools.lru_cache(maxsize=1)
def de_bruijn_4_8():
    """B(4, 8) as encoded bases (1, 2, 4, 8), linearised: 4^8 + 7 bases that hold every 8-mer once (the standard Lyndon-word construction)."""
    k, n = 4, 8
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)                 # (nine levels deep)
    seq = seq + seq[:n - 1]
    out = (1 << np.array(seq, np.uint8)).astype(np.uint8)
    out.setflags(write=False)
    return out


def lineage_of(i: int) -> str:
    """Six levels, PER_TAXON references per leaf taxon; fixed-width names: ascending in i, as the tree sorts them."""
    x = i // PER_TAXON
    return f"R,a{x // 128:02d},b{x // 32:03d},c{x // 8:03d},d{x // 2:04d},e{x:04d}"


class Family:
    """A database of windows: `n_full` full tiles + `tail` references, short background windows (1 .. 39 k-mers from BG0 on) with the
    planted ones -- (tile, local reference, start, k-mers); tile -1: the partial last tile -- in their places."""

    def __init__(self, planted, n_full: int = 4, tail: int = 37):
        self.n_full, self.tail = n_full, tail
        self.n_refs = n_full * TILE + tail
        self.ntiles = n_full + (1 if tail else 0)
        i = np.arange(self.n_refs, dtype=np.int64)
        m = 1 + (i * 7) % 39
        s = BG0 + (i * 37) % (N_POS - BG0 - 40)
        self.planted_ids = []
        for tile, local, start, n_kmers in planted:
            t = n_full if tile < 0 else tile
            idx = t * TILE + local
            assert 0 <= idx < self.n_refs and (tile >= 0 or local < tail) and idx not in self.planted_ids
            assert 0 <= start and start + n_kmers <= BG0 and n_kmers >= 1
            s[idx], m[idx] = start, n_kmers
            self.planted_ids.append(idx)
        self.planted_ids = np.array(sorted(self.planted_ids), np.int64)
        self.start, self.n_kmers = s, m
        self.lineages = [lineage_of(int(j)) for j in i]
        assert self.lineages == sorted(self.lineages)
        self._cover = {}

    def flat(self):
        """(bases, offsets) for Tree.new_flat / Oracle.tree_new_flat, in database order."""
        seq = de_bruijn_4_8()
        lens = self.n_kmers + 7
        off = np.zeros(self.n_refs + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        idx = np.repeat(self.start - off[:-1].astype(np.int64), lens) + np.arange(int(off[-1]), dtype=np.int64)
        return np.ascontiguousarray(seq[idx]), off

    def expected_counts(self, a: int, t: int) -> np.ndarray:
        """The closed form: k-mers the query [a, a + t) shares with every reference, in database order."""
        return np.clip(np.minimum(a + t, self.start + self.n_kmers) - np.maximum(a, self.start), 0, None).astype(np.uint16)

    def cover(self, tile: int) -> np.ndarray:
        """References of `tile` that cover each k-mer position."""
        if tile not in self._cover:
            lo, hi = tile * TILE, min((tile + 1) * TILE, self.n_refs)
            d = np.zeros(N_POS + 1, np.int64)
            np.add.at(d, self.start[lo:hi], 1)
            np.add.at(d, self.start[lo:hi] + self.n_kmers[lo:hi], -1)
            self._cover[tile] = np.cumsum(d)[:N_POS]
        return self._cover[tile]

    def segments(self, a: int, t: int, tile: int):
        """(sparse, dense): the rows of the query [a, a + t) whose segment in `tile` holds 1 .. 16 references (a full tile: the sparse
        slots) / 17 or more (or any at all in the partial last tile: the bitmap)."""
        c = self.cover(tile)[a:a + t]
        full = (tile + 1) * TILE <= self.n_refs
        sparse = int(((c >= 1) & (c <= 16)).sum()) if full else 0
        return sparse, int((c >= 1).sum()) - sparse

    def split(self, a: int, t: int, ref: int):
        """(dense, sparse) parts of the count of reference `ref` for the query [a, a + t) when no cap applies: the shared rows by the
        class of their segment in the reference's tile."""
        tile = ref // TILE
        lo, hi = max(a, int(self.start[ref])), min(a + t, int(self.start[ref] + self.n_kmers[ref]))
        if hi <= lo:
            return 0, 0
        c = self.cover(tile)[lo:hi]
        full = (tile + 1) * TILE <= self.n_refs
        sp = int((c <= 16).sum()) if full else 0
        return hi - lo - sp, sp


def query(a: int, t: int) -> np.ndarray:
    """The read that holds the k-mer positions [a, a + t): t + 7 bases (t = 0: seven bases, no k-mer)."""
    assert 0 <= a and a + t <= BG0
    return de_bruijn_4_8()[a:a + t + 7].copy()


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off


# ---- the planted windows: (tile, local reference, start, k-mers); every case has a stretch of positions of its own ---------------------
def _planted():
    p = []
    # 8 planes (positions 1 000 .. 4 300)
    p.append((0, 97, 1000, 255))                                           # alone in its tile: 0 dense + 255 sparse; byte 1 of its group
    p += [(0, l, 1255 - c, 20) for c, l in zip(range(1, 8), (96, 98, 99, 100, 101, 102, 103))]     # its byte neighbours: counts 1 .. 7
    p += [(1, 200 + i, 2000 - i, 255 + 2 * i) for i in range(17)]          # 17 supersets in one tile: 255 dense + 0 sparse
    p += [(2, 240 + i, 3000, 255 if i == 1 else 128) for i in range(17)]   # one of 255 among 16 of its first 128: 128 dense + 127 sparse
    p += [(-1, 5, 4000, 255), (-1, 4, 4250, 30), (-1, 6, 4250, 30)]        # the partial last tile
    # 10 planes (5 000 .. 10 100)
    p += [(0, 320 + i, 5000, 1023 if i == 1 else 768) for i in range(17)]  # 768 dense + 255 sparse
    p += [(1, 400 + i, 7000 - i, 1023 + 2 * i) for i in range(17)]         # two groups of eight all at 1023 (high bits 3, low bytes 0xFF) beside one of all 0
    p += [(2, 80, 7000, 512), (2, 81, 7000, 511), (2, 82, 7000, 256), (2, 83, 7000, 255)]     # either side of the carries; 512 sparse rows: the cap
    p += [(-1, 9, 9000, 1023), (-1, 8, 9001, 1023)]
    # 11, 12 and 16 planes, the pairs (11 950 .. 19 901)
    p += [(1, 481, 12000, 7900), (1, 482, 12001, 7900), (1, 480, 12000, 1024), (1, 483, 12000, 1023)]
    p += [(2, 600 + i, 12000 - i, 2047 + 2 * i) for i in range(19)]                 # (19, not 17: no tie with the 17 of tile 0, no confidence of k / 8 or k / 40)
    p += [(-1, 20, 12000, 4096), (-1, 21, 11999, 4098), (-1, 22, 11998, 4100)]     # (three: the top-level taxa hold different numbers of references that contain a query)
    p += [(0, 1200 + i, 12000, 2047 if i == 1 else 1792) for i in range(17)]   # 1792 dense + 255 sparse
    p += [(3, 2000, 12000, 255), (3, 2001, 12000, 256), (3, 2002, 12000, 511), (3, 2003, 12000, 512)]   # either side of the carries
    # sparse segments per (query, tile) (19 970 .. 20 810)
    p += [(0, 700 + i, 19990 - i, 800 + 2 * i) for i in range(17)]         # the queries' own references: dense
    p += [(1, 800 + j, 19999 - j, 301 + j) for j in range(16)]             # exactly 16 cover 20 000 .. 20 299: sparse
    p += [(2, 900 + j, 19999 - j, 301 + j) for j in range(17)]             # exactly 17: dense
    p += [(3, 1000, 20000, 300)]                                           # one: sparse ...
    # ... in a tile that stays live for a pruned query: 18 references on the rest of the query, seven of them in the sparse one's block of
    # eight -- the bounds of the blocks of 64 and of 8 see all 400 k-mers there, so the counting pass visits the tile whatever K is
    p += [(3, 1001 + i, 20300, 500) for i in range(18)]
    return p


PLANTED = _planted()
SPARSE_TARGETS = (0, 1, 3, 4, 5, 63, 64, 65, 252, 253, 254, 255, 256, 300)
PAIR_OFFSETS = (0, 1, 8, 23, 24, 25, 63, 64, 65)    # pairs that share t - d rows
# windows of PAIR_T rows from PAIR_A + d on: for every d above the three min-hashes of the read are those of d = 0 (the smallest 12-mers lie
# in the part all of them share), so the stable sort leaves them in input order; the two disjoint windows sort behind them
PAIR_T, PAIR_A, PAIR_DISJOINT = 300, 12100, (12500, 12900)

# the designed queries of every case: (a, t)
QUERIES = {
    "p8": [(1000, 255), (2000, 255), (3000, 255), (4000, 255), (1001, 254), (2001, 254), (999, 255), (3000, 128), (2100, 8), (3100, 155)],
    "p10": [(5000, 1023), (7000, 1023), (6990, 1023), (7001, 1022), (9000, 1023), (9001, 1022), (7000, 512), (7000, 256), (5000, 600),
            (5500, 500)],
    "p10_long": [(6999, 1024)],
    "p11": [(12000, 2047), (12001, 2046), (12000, 1024), (11999, 2047), (12010, 1500)],
    "p12": [(12000, 1024), (12000, 2047), (12000, 2048), (12000, 4095), (12001, 4095)],
    "p16": [(12000, 4096)],
    "p16_global": [(12000, 7893)],
    "seg": [(20300 - k, 400) for k in SPARSE_TARGETS],
}
P11_BULK = 4100           # >= kMinMidClass (rtx_api_batch.hip) queries of 1 031 .. 2 054 bases form the eleven-plane class
P11_SAMPLE = 60           # of the bulk: held against the oracle's rows (every designed query is)


def p11_bulk():
    """Copies of a few windows at shifted offsets, every one inside the long planted reference (12 000 .. 19 900)."""
    return [(12000 + (i * 7) % 5000, 1024 + (i * 13) % 1024) for i in range(P11_BULK)]


def p11_queries():
    """The designed queries, then the bulk."""
    return QUERIES["p11"] + p11_bulk()


def p11_sampled():
    """Positions in p11_queries() that are held against the oracle row by row: every designed query and a stride of the bulk."""
    n = len(QUERIES["p11"])
    return list(range(n)) + list(range(n, n + P11_BULK, P11_BULK // P11_SAMPLE))


def family(n_full: int = 4, tail: int = 37) -> Family:
    return Family(PLANTED, n_full, tail)


# ---- the processing order without the locator (rtx_cluster.hip: sketch_kernel + class keys + a stable radix sort), restated -------------
def sketch_key(seq: np.ndarray) -> int:
    """Three bottom-1 min-hashes over the 12-mers of a read (21 bits each) as the sort sees them: 63 bits, two dropped for the class."""
    none = (1 << 21) - 1
    if len(seq) < 12:
        m = [none] * 3
    else:
        two = (np.log2(seq).astype(np.uint64)) & np.uint64(3)
        code = np.zeros(len(seq) - 11, np.uint64)
        for j in range(12):
            code = (code << np.uint64(2)) | two[j:len(seq) - 11 + j]
        m = [int(((code * np.uint64(c)) >> np.uint64(43)).min()) for c in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)]
    return ((m[0] << 42) | (m[1] << 21) | m[2]) >> 2


def expected_order(seqs) -> np.ndarray:
    """perm[position] = query for a batch of one length class with the locator off: ascending keys, input order among equals."""
    return np.argsort(np.array([sketch_key(s) for s in seqs], np.uint64), kind="stable")


def pair_queries():
    """The batch of the pair case: (a, t) per query, an odd number of them.  Windows at offsets PAIR_A + d beside a copy of the window
    itself, laid out so that the stable order pairs them; two disjoint windows; two reads too short for a 12-mer around one without a
    k-mer, which end the order: the first two form a pair, the last one is alone."""
    qs = []
    for d in PAIR_OFFSETS:
        qs += [(PAIR_A, PAIR_T), (PAIR_A + d, PAIR_T)]
    qs += [(x, PAIR_T) for x in PAIR_DISJOINT]
    qs += [(PAIR_A + 2000, 4), (PAIR_A + 2100, 0), (PAIR_A + 2200, 3)]     # 11, 7 and 10 bases
    assert len(qs) % 2 == 1
    return qs


def pairs_of(order: np.ndarray):
    """The pairs the pair kernel formed in a sub-batch: positions 2 i, 2 i + 1 (the last one alone if the number is odd)."""
    return [(int(order[i]), int(order[i + 1]) if i + 1 < len(order) else None) for i in range(0, len(order), 2)]


def pair_kinds(qs, order):
    """What the pairs of the processing order were: for two windows of PAIR_T rows, shared / A-only / B-only rows."""
    kinds = dict(identical=0, disjoint=0, odd_lists=0, single=0, no_kmers_inside=0, shifts=set())
    for x, y in pairs_of(order):
        if y is None:
            kinds["single"] += 1
            continue
        (a, ta), (b, tb) = qs[x], qs[y]
        if min(ta, tb) == 0:
            kinds["no_kmers_inside"] += max(ta, tb) > 0
            continue
        shared = max(0, min(a + ta, b + tb) - max(a, b))
        kinds["identical"] += (a, ta) == (b, tb)
        kinds["disjoint"] += shared == 0
        kinds["odd_lists"] += shared > 0 and (ta - shared) % 8 != 0 and (tb - shared) % 8 != 0
        if ta == tb == PAIR_T:
            kinds["shifts"].add(abs(a - b) if shared else PAIR_T)
    return kinds


# ---- the oracle's results of the designed queries, computed once per family and shared by the tests ------------------------------------
def case_queries(case):
    if case == "pairs":
        return [q for q in pair_queries() if q[1] > 0]          # (the read without a k-mer has no counts to compare)
    if case == "p11_sample":
        qs = p11_queries()
        return [qs[i] for i in p11_sampled()]
    return QUERIES[case]


class World:
    """A family with its oracle tree and, per case, the oracle's counts, probabilities and rows of the designed queries (computed once)."""

    def __init__(self, oracle, n_full, tail):
        self.oracle = oracle
        self.fam = family(n_full, tail)
        bases, off = self.fam.flat()
        self.otree = oracle.tree_new_flat(self.fam.lineages, bases, off)
        self._res = {}

    def case(self, name):
        if name not in self._res:
            qs = case_queries(name)
            b, o = concat([query(a, t) for a, t in qs])
            t_o, c_o = self.otree.hit_counts_batch(b, o, threads=8)
            tabs, z, rc = self.oracle.prob_tables_batch(t_o, c_o, threads=8)
            bad, rows, nrows = self.otree.classify_batch(b, o, raw_confidence=True, threads=8, cap=64)
            self._res[name] = dict(qs=qs, t=t_o, counts=c_o, tables=tabs, rc=rc, bad=bad, rows=[self.otree.rows_of(rows, nrows, j, 64) for j in range(len(qs))])
        return self._res[name]

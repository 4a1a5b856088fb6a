"""What the tests of the denoiser (rtx_otu_unoise, rtx_otu_unoise_host) share: the definition of raxtax_hip.h, "Denoising (UNOISE)", restated in
numpy -- a full Levenshtein table, k(e, p) with Python integers, solve() in row order -- and the worlds the tests run.  Every world names
its rows (marks: name -> rank); test_unoise_cpu.py proves from solve() alone that a world holds what it claims."""
import functools

import numpy as np

import raxtax_amd as rx
from tally_common import concat, random_seq

ZOTU, ABSORBED, LEFT, LONG = 0, 1, 2, 3
NONE = 0xFFFFFFFF
MAX_LEN = 4096
MAX_DIFFS = 16
PLAIN = (1, 2, 4, 8)


def lev_many(x, ys):
    """the Levenshtein distance of x to every y of ys: the full table, row by row, all of ys abreast (padded with a byte that matches nothing)"""
    x = np.asarray(x, np.uint8)
    lens = np.array([len(y) for y in ys], np.int64)
    width = int(lens.max()) if len(ys) else 0
    Y = np.full((len(ys), width), 255, np.uint8)
    for p, y in enumerate(ys):
        Y[p, :len(y)] = y
    ar = np.arange(width + 1, dtype=np.int64)
    prev = np.broadcast_to(ar, (len(ys), width + 1)).copy()
    for i in range(1, len(x) + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        np.minimum(prev[:, :-1] + (Y != x[i - 1]), prev[:, 1:] + 1, out=cur[:, 1:])
        cur = np.minimum.accumulate(cur - ar, axis=1) + ar   # cur[j] = min over j' <= j of cur[j'] + (j - j'): the insertions
        prev = cur
    return prev[np.arange(len(ys)), lens]


def lev(x, y):
    return int(lev_many(x, [np.asarray(y, np.uint8)])[0])


def allowed(wp, we, alpha, max_diffs):
    """k(e, p): the largest d in 0 .. max_diffs with (wp >> (alpha d + 1)) >= we; a shift of 64 or more gives 0"""
    wp, we, k = int(wp), int(we), 0
    for d in range(1, max_diffs + 1):
        sh = alpha * d + 1
        if (0 if sh >= 64 else wp >> sh) >= we:
            k = d
    return k


def lim_of(sizes, alpha):
    return np.array([sum(1 for p in sizes if (int(p) >> (alpha + 1)) >= int(e)) for e in sizes], np.uint32)


def tiers_of(sizes, alpha):
    """the first rows of the tiers, and n behind them"""
    begin, s0, n = [], 0, len(sizes)
    while s0 < n:
        begin.append(s0)
        s1 = s0 + 1
        while s1 < n and (int(sizes[s0]) >> (alpha + 1)) < int(sizes[s1]):
            s1 += 1
        s0 = s1
    return begin + [n]


def solve(seqs, sizes, counts=None, minsize=8, alpha=2, max_diffs=0, everybody_live=False):
    """The definition, e ascending.  everybody_live: every row below lim(e) that is not long is a parent, whatever its status (what UNOISE's
    greedy rule forbids; for the test of that rule only)."""
    max_diffs = max_diffs or MAX_DIFFS
    n = len(seqs)
    sizes = [int(s) for s in sizes]
    lim = lim_of(sizes, alpha)
    status = np.full(n, LEFT, np.uint8)
    parent = np.full(n, NONE, np.uint32)
    dist = np.full(n, NONE, np.uint32)
    for e in range(n):
        if len(seqs[e]) > MAX_LEN:
            status[e] = LONG
            continue
        cand = [p for p in range(int(lim[e])) if (status[p] == ZOTU or (everybody_live and status[p] != LONG)) and allowed(sizes[p], sizes[e], alpha, max_diffs) >= 1]
        best = None
        if cand:
            d = lev_many(seqs[e], [seqs[p] for p in cand])
            for p, dp in zip(cand, d):
                if dp <= allowed(sizes[p], sizes[e], alpha, max_diffs) and (best is None or (int(dp), p) < best):
                    best = (int(dp), p)
        if best is not None:
            status[e], dist[e], parent[e] = ABSORBED, best[0], best[1]
        elif sizes[e] >= minsize:
            status[e] = ZOTU
    otu = np.zeros(n, np.uint32)
    seed = []
    for r in range(n):
        if status[r] == ABSORBED:
            otu[r] = otu[parent[r]]
        else:
            otu[r] = len(seed)
            seed.append(r)
    no = len(seed)
    counts = np.asarray(sizes, np.uint64)[:, None] if counts is None else np.asarray(counts, np.uint64)
    oc = np.zeros((no, counts.shape[1]), np.uint64)
    members = np.zeros(no, np.uint64)
    for r in range(n):
        oc[otu[r]] += counts[r]
        members[otu[r]] += 1
    return {"status": status, "parent": parent, "dist": dist, "lim": lim, "otu": otu, "seed": np.array(seed, np.uint32), "members": members,
            "sizes": oc.sum(axis=1).astype(np.uint64), "counts": oc, "long_rows": int((status == LONG).sum()), "minsize": minsize, "alpha": alpha, "max_diffs": max_diffs,
            "n_zotu": int((status == ZOTU).sum()), "n_absorbed": int((status == ABSORBED).sum()), "n_left": int((status == LEFT).sum()), "n_long": int((status == LONG).sum())}


def solve_table(table, **params):
    return solve(table.seqs, table.sizes, table.counts, **params)


VIEW_KEYS = ("n_zotu", "n_absorbed", "n_left", "n_long", "minsize", "alpha", "max_diffs")


def assert_unoise(got, want):
    """an rx.Otus of otu_unoise / otu_unoise_host against a solve() dict or another such rx.Otus: every field of both views but the device's
    counters and the times, no tolerance"""
    if not isinstance(want, dict):
        w = {k: getattr(want, k) for k in ("otu", "seed", "members", "sizes", "counts", "long_rows")}
        w.update(want.unoise)
        want = w
    assert got.n_rows == len(want["otu"]) and got.n_otus == len(want["seed"])
    for k in ("status", "parent", "dist", "lim"):
        assert got.unoise[k].shape == want[k].shape and np.array_equal(got.unoise[k], want[k]), k
    for k in VIEW_KEYS:
        assert got.unoise[k] == want[k], (k, got.unoise[k], want[k])
    for k in ("otu", "seed", "members", "sizes", "counts"):
        assert getattr(got, k).shape == want[k].shape and np.array_equal(getattr(got, k), want[k]), k
    assert got.long_rows == want["long_rows"] and got.links.shape == (0, 2) and got.rounds == 0 and got.link_passes == 0


def table_of_weights(seqs, weights, sample=None, samples=0):
    """a TallyTable whose rows hold any weight below 2^64: 16 bits of the weights per table (a chunk of rtx_tally_table_add counts at most 2^32 - 1
    reads), doubled by merging it with itself, and the sum of those"""
    weights = [int(w) for w in weights]
    parts = []
    for level in range(4):
        digit = [(w >> (16 * level)) & 0xFFFF for w in weights]
        pick = [i for i, d in enumerate(digit) if d]
        if not pick:
            continue
        t = None
        for a in range(0, len(pick), 60000):
            chunk = pick[a:a + 60000]
            args = (*concat([seqs[i] for i in chunk]), None if sample is None else np.asarray([sample[i] for i in chunk], np.uint32), np.array([digit[i] for i in chunk], np.uint32))
            if t is None:
                t = rx.tally_reads(*args, samples=samples)
            else:
                t.add(*args)
        for _ in range(16 * level):
            t = rx.tally_merge([t, t])
        parts.append(t)
    return parts[0] if len(parts) == 1 else rx.tally_merge(parts)


def rank_of(table):
    return {bytes(s): r for r, s in enumerate(table.seqs)}


class World:
    """rows by name; .build() -> (table, marks: name -> rank)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.names, self.seqs, self.weights, self.seen = [], [], [], set()

    def add(self, name, seq, weight):
        seq = np.asarray(seq, np.uint8)
        assert bytes(seq) not in self.seen, name
        self.seen.add(bytes(seq))
        self.names.append(name)
        self.seqs.append(seq)
        self.weights.append(int(weight))
        return seq

    def centre(self, name, length, weight):
        return self.add(name, random_seq(self.rng, length), weight)

    def build(self):
        table = table_of_weights(self.seqs, self.weights)
        by = rank_of(table)
        return table, {n: by[bytes(s)] for n, s in zip(self.names, self.seqs)}


def other(rng, c):
    return int(rng.choice([p for p in PLAIN if p != c]))


def sub_at(rng, s, i):
    t = np.array(s, np.uint8)
    t[i] = other(rng, int(s[i]))
    return t


def delete_at(s, i):
    return np.delete(np.asarray(s, np.uint8), i)


def insert_at(rng, s, i):
    """a base in front of s[i] (i = len: behind the end) that differs from both neighbours: no alignment undoes it for less"""
    s = np.asarray(s, np.uint8)
    near = {int(s[j]) for j in (i - 1, i) if 0 <= j < len(s)}
    return np.insert(s, i, int(rng.choice([p for p in PLAIN if p not in near])))


def edited(rng, s, d, kinds, where=None):
    """s after d random edits of the given kinds ('s', 'i', 'd') whose Levenshtein distance to s is exactly d (drawn again until it is)"""
    for _ in range(200):
        t = np.array(s, np.uint8)
        for _e in range(d):
            kind = kinds[int(rng.integers(len(kinds)))]
            if kind == "s":
                t = sub_at(rng, t, int(rng.integers(len(t))) if where is None else min(where, len(t) - 1))
            elif kind == "d":
                t = delete_at(t, int(rng.integers(len(t))) if where is None else min(where, len(t) - 1))
            else:
                t = insert_at(rng, t, int(rng.integers(len(t) + 1)) if where is None else min(where, len(t)))
        if lev(s, t) == d:
            return t
    raise AssertionError("no such edit found")


def weight_for(we, k, alpha=2):
    """the least weight of a parent that allows a read of weight we exactly k differences"""
    return int(we) << (alpha * k + 1)


# ---- the worlds ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def skew_world(alpha):
    """per d = 1, 2, 3: a centre at exactly w[e] 2^(alpha d + 1) with a read d away (absorbed), a centre one read lighter with a read d away (not).
    Then a centre of 100 x 2^(16 alpha + 3) reads (k would pass 16: capped) with reads at d = 16 and 17."""
    w = World(100 + alpha)
    for d in (1, 2, 3):
        c = w.centre(f"at{d}", 90, weight_for(9, d, alpha))
        w.add(f"at{d}_read", edited(w.rng, c, d, "s"), 9)
        c = w.centre(f"below{d}", 90, weight_for(9, d, alpha) - 1)
        w.add(f"below{d}_read", edited(w.rng, c, d, "s"), 9)
    if alpha <= 2:
        c = w.centre("cap", 120, 100 << (16 * alpha + 3))
        w.add("cap_read16", edited(w.rng, c, 16, "s"), 100)
        w.add("cap_read17", edited(w.rng, c, 17, "s"), 99)
    return w.build() + ({"alpha": alpha},)


@functools.lru_cache(maxsize=None)
def shift_world():
    """alpha = 8: d = 8 would shift by 65, so k = 7 however heavy the parent (2^62 reads here)"""
    w = World(7)
    c = w.centre("heavy", 100, 1 << 62)
    w.add("read7", edited(w.rng, c, 7, "s"), 1)
    w.add("read8", edited(w.rng, c, 8, "s"), 1)
    return w.build() + ({"alpha": 8},)


DISTANCE_KINDS = ("subs", "ins", "dels", "mixed", "indel_first", "indel_last")


@functools.lru_cache(maxsize=None)
def distance_world():
    """per kind of edit and k = 1, 2, 3 (and 16): a centre that allows its two reads exactly k, one read at d = k, one at d = k + 1"""
    w = World(11)
    cases = []

    def case(name, k, c, near, far):
        assert lev(c, near) == k and lev(c, far) == k + 1, name
        w.add(name, c, weight_for(2, k))
        w.add(name + "_near", near, 2)
        w.add(name + "_far", far, 2)
        cases.append((name, k))

    for k in (1, 2, 3, 16):
        for kind in DISTANCE_KINDS:
            if k == 16 and kind not in ("subs", "mixed"):
                continue
            c = random_seq(w.rng, int(w.rng.integers(90, 111)))
            if kind == "subs":
                near, far = edited(w.rng, c, k, "s"), edited(w.rng, c, k + 1, "s")
            elif kind == "ins":    # a length difference of exactly k, and of k + 1 (the length test drops it)
                near, far = edited(w.rng, c, k, "i"), edited(w.rng, c, k + 1, "i")
            elif kind == "dels":
                near, far = edited(w.rng, c, k, "d"), edited(w.rng, c, k + 1, "d")
            elif kind == "mixed":
                near, far = edited(w.rng, c, k, "sid"), edited(w.rng, c, k + 1, "sid")
            elif kind == "indel_first":   # a deletion at position 0 (and the rest anywhere): Hamming distance large, edit distance small
                near = edited(w.rng, delete_at(c, 0), k - 1, "s") if k > 1 else delete_at(c, 0)
                far = edited(w.rng, insert_at(w.rng, c, 0), k, "s")
            else:
                near = edited(w.rng, insert_at(w.rng, c, len(c)), k - 1, "s") if k > 1 else insert_at(w.rng, c, len(c))
                far = edited(w.rng, delete_at(c, len(c) - 1), k, "s")
            case(f"{kind}{k}", k, c, near, far)
    # a homopolymer run: every deletion inside it is the same read, several alignments tie
    c = random_seq(w.rng, 100)
    c[40:52] = 1
    c[39], c[52] = 2, 4
    case("homopolymer1", 1, c, delete_at(c, 45), delete_at(delete_at(c, 45), 46))
    # an ambiguity code against a plain base is a mismatch; equal ambiguity codes match
    c = random_seq(w.rng, 100)
    c[30] = 15
    plain = c.copy()
    plain[30] = 1
    case("ambiguous1", 1, c, plain, sub_at(w.rng, plain, 60))
    c = random_seq(w.rng, 100)
    c[30] = 15
    case("same_code1", 1, c, sub_at(w.rng, c, 60), sub_at(w.rng, sub_at(w.rng, c, 60), 10))
    return w.build() + (tuple(cases),)


LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def lengths_world():
    """a centre of every edge length (16 reads) with a read one substitution (the last code) and one deletion away (2 reads each: k = 1)"""
    w = World(13)
    for n in LENGTHS:
        c = random_seq(w.rng, n)
        if n == 1:
            c[:] = 1
        w.add(f"len{n}", c, 16)
        w.add(f"len{n}_sub", sub_at(w.rng, c, n - 1) if n > 1 else np.array([2], np.uint8), 2)
        if n >= 15:
            w.add(f"len{n}_del", edited(w.rng, c, 1, "d"), 2)
    return w.build()


@functools.lru_cache(maxsize=None)
def short_world():
    """a read shorter than k: 3 codes against a centre of 10 that allows it 16 differences"""
    w = World(17)
    c = w.centre("centre", 10, weight_for(2, 16))
    w.add("short", c[[0, 4, 9]], 2)
    return w.build()


@functools.lru_cache(maxsize=None)
def long_world():
    """4096 codes as centroid and as read; 4097: long, an OTU of its own, no parent of the rarer copy beside it (one code less: not long)"""
    w = World(19)
    c = w.centre("max", 4096, 16)
    w.add("max_read", sub_at(w.rng, c, 4095), 2)
    c = w.centre("long", 4097, 16)
    w.add("long_copy", delete_at(c, 2000), 2)
    w.add("long_too", sub_at(w.rng, c, 7), 2)
    return w.build()


@functools.lru_cache(maxsize=None)
def ties_world():
    w = World(23)
    # two live centroids at equal d: the lower rank wins
    p1 = w.centre("p1", 80, 64)
    w.add("p2", sub_at(w.rng, p1, 20), 63)
    t = p1.copy()
    t[20] = [c for c in PLAIN if c not in (int(p1[20]), int(w.seqs[-1][20]))][0]
    w.add("tie_read", t, 2)
    # a centroid of higher rank at a smaller d beats one of lower rank at a larger d
    q1 = w.centre("q1", 80, 512)
    q2 = w.add("q2", sub_at(w.rng, sub_at(w.rng, q1, 10), 50), 511)
    w.add("near_read", sub_at(w.rng, q2, 30), 2)
    return w.build()


@functools.lru_cache(maxsize=None)
def lanes_world(n_live):
    """n_live centroids (weights all within a factor of 8: nobody absorbs another, the list position is the rank) and a read one substitution
    away from the centroid at list positions 0, 63, 64, 65 and the last"""
    w = World(29 + n_live)
    centres = [w.centre(f"c{i}", 60, 100 + n_live - i) for i in range(n_live)]
    at = sorted({p for p in (0, 63, 64, 65, n_live - 1) if p < n_live})
    for p in at:
        w.add(f"read{p}", sub_at(w.rng, centres[p], 30), 2)
    return w.build() + (tuple(at),)


@functools.lru_cache(maxsize=None)
def greedy_world():
    """A (1000); B = A + one substitution (100), absorbed by A; C = B + one substitution (10), d(C, A) = 2.  Under max_diffs = 1 B would absorb C
    and A may not: C is a ZOTU, because B is no parent."""
    w = World(31)
    a = w.centre("A", 100, 1000)
    b = w.add("B", sub_at(w.rng, a, 25), 100)
    w.add("C", sub_at(w.rng, b, 75), 10)
    return w.build() + ({"max_diffs": 1},)


@functools.lru_cache(maxsize=None)
def small_world():
    """minsize = 100: a small read that is absorbed, a small read that is left, a small read that would absorb a rarer one and does not"""
    w = World(37)
    c = w.centre("centre", 90, 1600)
    w.add("small_absorbed", sub_at(w.rng, c, 5), 40)
    w.centre("small_left", 90, 30)
    s = w.centre("small_parent", 90, 80)
    w.add("small_child", sub_at(w.rng, s, 44), 2)
    return w.build() + ({"minsize": 100},)


@functools.lru_cache(maxsize=None)
def tiers_world():
    """a parent in the tier just before at exactly 2^(alpha + 1) times the weight; the last row of a tier (11: no candidate of 80) and the first
    of the next (10)"""
    w = World(41)
    p = w.centre("parent", 90, 80)
    w.add("last_of_tier", sub_at(w.rng, p, 10), 11)
    w.add("first_of_next", sub_at(w.rng, p, 20), 10)
    return w.build()


@functools.lru_cache(maxsize=None)
def one_tier_world():
    """20 rows within a factor of 8, one substitution from the first: one tier, nobody is absorbed"""
    w = World(43)
    c = w.centre("r0", 70, 63)
    for i in range(1, 20):
        w.add(f"r{i}", sub_at(w.rng, c, 3 * i), 63 - 2 * i)
    return w.build()


@functools.lru_cache(maxsize=None)
def row_tiers_world():
    """every row a tier of its own: weights 8^7 .. 8, 1, all one substitution from the first"""
    w = World(47)
    c = w.centre("r0", 70, 8 ** 7)
    for i in range(1, 8):
        w.add(f"r{i}", sub_at(w.rng, c, 5 * i), 8 ** (7 - i))
    return w.build()


def planted(seed, per_d):
    """40 random centres of 120 bases with geometric abundances, each with per_d[d - 1] variants at d = 1, 2, 3 light enough for their centre to
    allow them d differences (and heavier than nothing else allows): (table, marks, variants: name -> (centre name, d))"""
    w = World(seed)
    variants = {}
    for i in range(40):
        wc = int(200000 * 0.85 ** i)
        c = w.centre(f"centre{i}", 120, wc)
        for d in (1, 2, 3):
            top = wc >> (2 * d + 1)
            for v in range(per_d[d - 1]):
                name = f"v{i}_{d}_{v}"
                seq = edited(w.rng, c, d, "sid" if v % 2 else "s")
                while bytes(seq) in w.seen:
                    seq = edited(w.rng, c, d, "sid" if v % 2 else "s")
                w.add(name, seq, max(1, min(top, int(w.rng.integers(1, 8)))))
                variants[name] = (f"centre{i}", d)
    table, marks = w.build()
    return table, marks, variants


@functools.lru_cache(maxsize=None)
def planted_world():
    return planted(53, (4, 3, 2))


@functools.lru_cache(maxsize=None)
def big_planted_world():
    """the same with 49 variants per centre: 2 000 rows, held against the host function only"""
    return planted(59, (25, 16, 8))


SOLVED = {}


def solved(key, table, **params):
    """solve_table once per world (key) and parameters"""
    k = (key, tuple(sorted(params.items())))
    if k not in SOLVED:
        SOLVED[k] = solve_table(table, **params)
    return SOLVED[k]


def all_worlds():
    """(key, table, params) of every world that is held against solve()"""
    out = [(f"skew{a}", skew_world(a)[0], skew_world(a)[2]) for a in (1, 2, 3)]
    out.append(("shift", shift_world()[0], shift_world()[2]))
    out.append(("distance", distance_world()[0], {}))
    out.append(("lengths", lengths_world()[0], {}))
    out.append(("short", short_world()[0], {}))
    out.append(("long", long_world()[0], {}))
    out.append(("ties", ties_world()[0], {}))
    out += [(f"lanes{n}", lanes_world(n)[0], {}) for n in (65, 128, 129)]
    out.append(("greedy", greedy_world()[0], greedy_world()[2]))
    out.append(("small", small_world()[0], small_world()[2]))
    out.append(("small_minsize1", small_world()[0], {"minsize": 1}))
    out.append(("tiers", tiers_world()[0], {}))
    out.append(("one_tier", one_tier_world()[0], {}))
    out.append(("row_tiers", row_tiers_world()[0], {}))
    out.append(("planted", planted_world()[0], {}))
    return out

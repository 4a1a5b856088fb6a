"""The de novo chimera check restated in numpy, from the definition in include/raxtax_hip.h ("de novo chimera check of a run") and nothing
else: the entries with their weights, lim from Python integers, one inverted index over the 8-mer SETS of all entries, and per entry the
counts of chimera_common.Restatement over an explicit list of parents -- the entries below lim that are not flagged.  solve() walks the
entries in ascending order (the recursion of the definition); rounds() iterates from "nobody is flagged" the way the device does and
counts the rounds and the entry scans.  It shares no code with the library.  The builders of the designed cases are here too."""
from __future__ import annotations

import bisect

import numpy as np

import chimera_common as cc

NO_REF = cc.NO_REF
NO_PARENT = 3
ACGT = np.array([1, 2, 4, 8], np.uint8)
N = np.array([15], np.uint8)


def blank(status):
    return dict(status=status, n_valid=0, single=0, parent=NO_REF, seg=0, pos=0, left=0, parent_a=NO_REF, right=0, parent_b=NO_REF, delta=0, flag=0)


def limits(weights, abskew=2, max_parents=262144):
    """lim(e) = min(e, #{p : w[p] >= abskew w[e]}, max_parents), in Python integers."""
    w = [int(x) for x in weights]
    assert all(w[i] >= w[i + 1] for i in range(len(w) - 1)), "weights never increase along the list"
    neg = [-x for x in w]   # ascending: w[p] >= a x  <=>  -w[p] <= -a x
    return [min(e, bisect.bisect_right(neg, -abskew * x), max_parents) for e, x in enumerate(w)]


class Restatement:
    """seqs: the entries' sequences in entry order; weights likewise."""

    def __init__(self, seqs, weights, segments=16, mindelta=24, abskew=2, max_parents=0):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        self.n = len(self.seqs)
        self.S, self.mindelta = int(segments), int(mindelta)
        self.weights = [int(x) for x in weights]
        self.lim = limits(self.weights, abskew, max_parents or 262144)
        self.n_par = max(self.lim, default=0)
        self.win = [cc.window_codes(s) for s in self.seqs]
        keys = [np.unique(code[valid]) * self.n + p for p, (code, valid) in enumerate(self.win[:self.n_par])]   # the SET of 8-mers of every parent
        keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
        self.post_ref = keys % max(self.n, 1)
        self.post_off = np.searchsorted(keys // max(self.n, 1), np.arange(65537))
        self._iterated = None   # (rounds() and flag_history() iterate once between them)

    def record(self, e, flagged) -> dict:
        """The record of entry e when `flagged` (bool per entry) are the flags of the entries below it."""
        S, lim, seq = self.S, self.lim[e], self.seqs[e]
        if len(seq) > cc.MAX_QUERY:
            return blank(cc.TOO_LONG)
        code, valid = self.win[e]
        n_pos = len(code)
        if not valid.any():
            return blank(cc.NO_KMER)
        if lim == 0:
            return blank(NO_PARENT)
        b = np.array([s * n_pos // S for s in range(S + 1)], np.int64)
        idx = np.nonzero(valid)[0]
        seg_of = np.searchsorted(b[1:], idx, side="right")
        lo, hi = self.post_off[code[idx]], self.post_off[code[idx] + 1]
        refs = np.concatenate([self.post_ref[a:z] for a, z in zip(lo, hi)])
        segs = np.repeat(seg_of, hi - lo)
        parent = (refs < lim) & ~np.asarray(flagged, bool)[refs]   # the explicit list: below lim and not flagged
        cnt = np.bincount(refs[parent] * S + segs[parent], minlength=lim * S).reshape(lim, S)
        P = np.concatenate([np.zeros((lim, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
        T = P[:, S]
        Suf = T[:, None] - P
        two = np.array([P[:, s].max() + Suf[:, s].max() for s in range(1, S)])
        seg = 1 + int(np.argmax(two))
        left, right, single = int(P[:, seg].max()), int(Suf[:, seg].max()), int(T.max())
        rec = blank(cc.OK)
        rec.update(n_valid=int(valid.sum()), single=single, parent=int(np.argmax(T)) if single else NO_REF, seg=seg, pos=int(b[seg]), left=left,
                   parent_a=int(np.argmax(P[:, seg])) if left else NO_REF, right=right, parent_b=int(np.argmax(Suf[:, seg])) if right else NO_REF,
                   delta=int(two[seg - 1]) - single)
        assert rec["delta"] >= 0
        rec["flag"] = int(rec["delta"] >= self.mindelta)
        return rec

    def solve(self):
        """The records of all entries: e ascending, the flags of the entries below e are final when e is looked at."""
        flagged = np.zeros(self.n, bool)
        recs = []
        for e in range(self.n):
            recs.append(self.record(e, flagged))
            flagged[e] = bool(recs[-1]["flag"])
        return recs

    def totals(self, e):
        """T_p of entry e for every p below n_par: the valid windows of e whose 8-mer occurs in p, whatever lim and the flags are."""
        code, valid = self.win[e]
        idx = np.nonzero(valid)[0]
        lo, hi = self.post_off[code[idx]], self.post_off[code[idx] + 1]
        refs = np.concatenate([self.post_ref[a:z] for a, z in zip(lo, hi)]) if len(idx) else np.zeros(0, np.int64)
        return np.bincount(refs, minlength=self.n_par)

    def _iterate(self):
        if self._iterated is None:
            self._iterated = self._iterate_once()
        return self._iterated

    def _iterate_once(self):
        flagged = np.zeros(self.n, bool)
        e0, rounds, scans, history = 0, 0, 0, []
        while True:
            rounds += 1
            scans += self.n - e0
            assert rounds <= self.n + 1
            new = flagged.copy()
            for e in range(e0, self.n):
                new[e] = bool(self.record(e, flagged)["flag"])
            diff = np.nonzero(new != flagged)[0]
            flagged = new
            history.append(flagged.copy())
            if len(diff) == 0:
                return rounds, scans, flagged, history
            e0 = next((e for e in range(self.n) if self.lim[e] > diff[0]), self.n)

    def rounds(self):
        """(rounds, scans, flags) of the iteration the device runs: round 1 takes every entry with nobody flagged, the next one the entries
        e with lim(e) > the lowest entry whose flag changed, and the first round that changes nothing is the last."""
        return self._iterate()[:3]

    def flag_history(self):
        """The flags behind every round of rounds(), one bool array per round (the flags in front of round 1 are all 0)."""
        return [h.copy() for h in self._iterate()[3]]


def as_tuples(recs):
    return [cc.as_tuple(r) for r in recs]


def check_equal(d, rs: Restatement, what=""):
    """A Denovo result against the restatement: lim, weights and every field of every record."""
    want = rs.solve()
    assert d.n_entries == rs.n, what
    assert [int(x) for x in d.lim] == rs.lim, what
    assert [int(x) for x in d.weight] == rs.weights, what
    got = as_tuples(d.rec)
    for e, (g, w) in enumerate(zip(got, as_tuples(want))):
        assert g == w, (what, e, dict(zip(cc.FIELDS, g)), dict(zip(cc.FIELDS, w)))
    assert d.n_flagged == sum(r["flag"] for r in want) and d.n_checked == sum(r["status"] == cc.OK for r in want), what
    flagged = {e for e, r in enumerate(want) if r["flag"]}
    assert not flagged & {int(r[k]) for r in d.rec for k in ("parent", "parent_a", "parent_b")}, what   # nobody names a flagged parent
    return want


def of_table(table, **params) -> Restatement:
    """The restatement over the rows of a TallyTable (entries = rows, weight = the row's total)."""
    return Restatement(table.seqs, table.sizes, **params)


def of_otus(table, otus, **params):
    """(restatement, the OTU of every entry) over the seeds of an Otus object: weight = the OTU's total, ordered by (weight descending, seed
    rank ascending)."""
    order = sorted(range(otus.n_otus), key=lambda k: (-int(otus.sizes[k]), int(otus.seed[k])))
    seqs = table.seqs
    return Restatement([seqs[int(otus.seed[k])] for k in order], [int(otus.sizes[k]) for k in order], **params), order


def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def tag(rng):
    """An N and seven random bases: makes a sequence distinct and adds no valid window (behind another N-separated piece)."""
    return np.concatenate([N, rand_seq(rng, 7)])


def prefix_world(n_parents, lims, seed=3, qlen=40, head=28):
    """n_parents parents with the weights 2 (W - p), descending, and one query per L in lims with the weight W - (L - 1), so that under
    abskew = 2 the parents of the query are exactly the entries 0 .. L - 1 (the edge w[p] = abskew w[e] is included, the next weight down
    is excluded).  Entry L (just outside, when it is a parent at all) holds the whole query; entry L - 1 and a lower entry j both hold the
    query's head and nothing else of it: j wins.  The designed parents are pieces joined by an N, so that no window spans two pieces.
    Returns (seqs, weights, {L: (entry of the query, j or L - 1 when there is no lower one)})."""
    rng = np.random.default_rng(seed)
    W = 2 * n_parents + 100   # every query is rarer than every parent, and no query is a parent of another
    queries = {L: rand_seq(rng, qlen) for L in lims}
    roles = {}
    lower = {}
    for L in lims:
        assert 1 <= L <= n_parents
        j = (L - 1) // 2 if L >= 3 else None
        lower[L] = j if j is not None else L - 1
        if L < n_parents:
            roles.setdefault(L, []).append(queries[L])
        roles.setdefault(L - 1, []).append(queries[L][:head])
        if j is not None:
            roles.setdefault(j, []).append(queries[L][:head])
    seqs, weights = [], []
    for p in range(n_parents):
        if p in roles:
            parts = []
            for piece in roles[p]:
                parts += [piece, N]
            seqs.append(np.concatenate(parts[:-1] + [tag(rng)]))
        else:
            seqs.append(rand_seq(rng, int(rng.integers(24, 61))))
        weights.append(2 * (W - p))
    where = {}
    for L in sorted(lims):   # (weights descend with L)
        where[L] = (len(seqs), lower[L])
        seqs.append(queries[L])
        weights.append(W - (L - 1))
    return seqs, weights, where


def substitute_at(seq, positions):
    out = seq.copy()
    for i in positions:
        out[i] = {1: 2, 2: 4, 4: 8, 8: 1}[int(out[i])]
    return out


def rounds_world(seed=5, length=200):
    """Templates A and B, C = the head of A joined to the tail of B, D = C with three substitutions, E = D with three more, at falling
    weights: with C live D is explained by C, with D live E is explained by D; by the definition all three are flagged."""
    rng = np.random.default_rng(seed)
    A, B = rand_seq(rng, length), rand_seq(rng, length)
    Cc = np.concatenate([A[:length // 2], B[length // 2:]])
    D = substitute_at(Cc, (20, 70, 150))
    E = substitute_at(D, (40, 120, 180))
    return [A, B, Cc, D, E], [1000, 900, 100, 20, 4]


def counts_world(seed=9):
    """Entries at the plane classes' edges and the odd ones: X of 4097 bases (too long as a query, still a parent), its first 4096, 1031 and
    1030 bases as queries whose parents hold every window, and short entries."""
    rng = np.random.default_rng(seed)
    X = rand_seq(rng, 4097)
    rep = rand_seq(rng, 120)
    rep[30:60] = 1                                   # a parent with a repeated 8-mer ...
    rep_q = rep.copy()
    rep_q[70:110] = 1                                # ... and a query with a longer run of it: every position counts
    amb = X[100:300].copy()
    amb[50:60] = 15
    amb[120] = 5
    short = X[500:513].copy()                        # 6 windows: n_pos < S
    entries = [(X, 100000), (X[:4096], 10000), (X[:1031], 1000), (X[:1030], 100), (rep, 5000), (rep_q, 50), (amb, 40), (short, 30),
               (X[700:707], 20), (np.full(30, 15, np.uint8), 10)]
    entries.sort(key=lambda t: -t[1])
    return [s for s, _ in entries], [w for _, w in entries]


def planted_world(seed=21, n_templates=40, n_chimeras=20, length=400):
    """Random templates with geometric weights, a few d = 1 variants of each, and chimeras of two templates at a weight of at most a
    quarter of the rarer parent.  Returns (reads as (sequence, weight), the template sequences, the chimera sequences)."""
    rng = np.random.default_rng(seed)
    templates = [rand_seq(rng, length) for _ in range(n_templates)]
    w = [max(64, int(20000 * 0.85 ** t)) for t in range(n_templates)]
    reads = [(t, x) for t, x in zip(templates, w)]
    for t, x in zip(templates, w):
        for _ in range(3):
            i = int(rng.integers(0, length))
            reads.append((substitute_at(t, (i,)), max(1, x // 50)))
    chimeras = []
    for _ in range(n_chimeras):
        a, b = (int(x) for x in rng.choice(n_templates, 2, replace=False))
        bp = int(rng.integers(length // 4, 3 * length // 4))
        c = np.concatenate([templates[a][:bp], templates[b][bp:]])
        chimeras.append(c)
        reads.append((c, max(1, min(w[a], w[b]) // 4 - int(rng.integers(0, 3)))))
    return reads, templates, chimeras


def table_of(rx, seqs, weights, samples=0, sample=None):
    bases, off = cc.concat([np.asarray(s, np.uint8) for s in seqs])
    return rx.tally_reads(bases, off, sample=sample, weight=np.asarray(weights, np.uint32), samples=samples)


def lane_entries(n_parents, tile, groups, lanes=(0, -1), bits=(0, 7)):
    """The entries of a tile of the stage's bitmap over n_parents entries that lie at bit j of byte g of a lane, for g in groups, j in bits
    and the lanes given (-1: the tile's last lane, L - 1): ref_slot inverted -- local entry (g L + lane) 8 + j is bit j of byte g of the
    lane.  Entries 0 and 1 (the templates of live_world) and entries that do not exist are left out."""
    stride = (((n_parents + 7) >> 3) + 15) & ~15
    L = min(64, (stride - tile * 1024) >> 4)
    out = set()
    for g in groups:
        for lane in lanes:
            for j in bits:
                e = tile * 8192 + ((g * L + lane % L) * 8 + j)
                if 2 <= e < n_parents:
                    out.add(e)
    return sorted(out)


WORD_EDGES = (0, 3, 4, 7, 8, 11, 12, 15)   # the first and the last byte of each 32-bit word of a lane's 16 bytes
LIVE_520 = tuple(lane_entries(520, 0, WORD_EDGES))                       # five lanes: bytes 0 .. 12 are in use, entry 519 is bit 7 of byte 12 of lane 4
LIVE_8232 = tuple(sorted(set(lane_entries(8232, 0, WORD_EDGES, bits=(7,)) + lane_entries(8232, 1, (0, 3, 4), bits=(0, 7)) + [2048])))


def live_world(n_parents, flagged_at, seed=13, qlen=40, head=28):
    """n_parents parents and one query per f in flagged_at, for segments = 4 and mindelta = 8.  Entries 0 and 1 are templates A and B at more
    than twice the weight of everything else, so that every other parent has exactly them as its parents.  Entry f is the piece "head of A +
    tail of B", an N, and the whole of the query Q_f: by the definition a chimera of A and B, flagged, and so no parent of Q_f.  A lower entry
    j_f that is not flagged -- f - 1 where that is free, so that the bit next to f's counts -- holds Q_f's head and nothing else of it.  Q_f is
    rarer than every parent: its lim is n_parents, its parent is j_f with `single` below the 33 windows that f holds.
    Returns (seqs, weights, {f: (entry of Q_f, j_f)})."""
    rng = np.random.default_rng(seed)
    flagged_at = sorted(flagged_at)
    assert flagged_at and 2 < flagged_at[0] and flagged_at[-1] < n_parents and len(set(flagged_at)) == len(flagged_at)
    A, B = rand_seq(rng, 80), rand_seq(rng, 80)
    piece = np.concatenate([A[:40], B[40:]])
    taken, lower = set(flagged_at), {}
    for f in flagged_at:
        j = next(j for j in range(f - 1, 1, -1) if j not in taken)
        taken.add(j)
        lower[f] = j
    queries = {f: rand_seq(rng, qlen) for f in flagged_at}
    head_of = {j: f for f, j in lower.items()}
    W = 2 * n_parents + 100
    seqs, weights = [A, B], [8 * W, 8 * W - 1]
    for p in range(2, n_parents):
        if p in queries:
            seqs.append(np.concatenate([piece, N, queries[p]]))
        elif p in head_of:
            seqs.append(np.concatenate([queries[head_of[p]][:head], tag(rng)]))
        else:
            seqs.append(rand_seq(rng, int(rng.integers(24, 61))))
        weights.append(2 * (W - p))
    where = {}
    for k, f in enumerate(flagged_at):
        where[f] = (len(seqs), lower[f])
        seqs.append(queries[f])
        weights.append(W - n_parents - k)
    return seqs, weights, where


def flipback_world(seed=31, length=200):
    """Templates A, B and Z (a bystander), then C, D and E at falling weights, for the default parameters.  C = A's head + B's tail: flagged
    in every round, so live in round 1 only.  D = A with B's bases 100 .. 139 in place of its own, which is also C's first 140 bases + A's
    tail: while C is live D is C's head joined to A's tail and flagged, once C is flagged A alone explains D as well as any pair and D is
    not flagged: D's flag goes 0 -> 1 -> 0 and its live bit is cleared and set again.  E = D with three substitutions: its parent is D.
    Returns (seqs, weights, names -> entry)."""
    rng = np.random.default_rng(seed)
    A, B, Z = (rand_seq(rng, length) for _ in range(3))
    Cc = np.concatenate([A[:100], B[100:]])
    D = np.concatenate([A[:100], B[100:140], A[140:]])
    E = substitute_at(D, (30, 120, 175))
    return [A, B, Z, Cc, D, E], [1000, 900, 800, 100, 20, 4], dict(A=0, B=1, Z=2, C=3, D=4, E=5)


def two_tile_rounds_world(seed=41):
    """8 232 parents in two tiles (the second one a single lane) with the chain of rounds_world laid across them.  In weight tiers, each at
    least twice the next: A and B; entries 2 .. 8179 with lim = 2, C among them at 8150; entries 8180 .. 8199 with lim = 8180, one tile;
    entries 8200 .. 8231 with lim = 8200, two tiles, D the first of them; and from 8232 on entries with lim = 8232: E, a query X of 1 100
    bases (twelve planes) whose first 700 an entry of the second tile holds, and fillers.  Round 1 flags C; round 2 takes the entries from
    8180 on -- the first entry that scans tile 0 is clipped, the first that scans tile 1 is not -- and flags D; round 3 takes those from
    8232 on -- both are clipped -- and flags E; round 4 has nothing to scan.
    H at 8190 is a query of the one-tile tier whose head entry 77 holds and whose whole entry 8185, outside its lim, holds.
    Returns (seqs, weights, names -> entry)."""
    rng = np.random.default_rng(seed)
    A, B = rand_seq(rng, 200), rand_seq(rng, 200)
    Cc = np.concatenate([A[:100], B[100:]])
    D = substitute_at(Cc, (20, 70, 150))
    E = substitute_at(D, (40, 120, 180))
    H, X = rand_seq(rng, 40), rand_seq(rng, 1100)
    names = dict(A=0, B=1, H_head=77, C=8150, H_whole=8185, H=8190, D=8200, X_head=8210, E=8232, X=8234)
    fixed = {0: A, 1: B, 77: np.concatenate([H[:28], tag(rng)]), 8150: Cc, 8185: np.concatenate([H, tag(rng)]), 8190: H, 8200: D,
             8210: np.concatenate([X[:700], tag(rng)]), 8232: E, 8234: X}
    n = 8240
    seqs = [fixed[e] if e in fixed else rand_seq(rng, int(rng.integers(24, 61))) for e in range(n)]
    weights = []
    for e in range(n):
        if e < 2:
            weights.append(40000 - e)
        elif e < 8180:
            weights.append(10000 + 8180 - e)
        elif e < 8200:
            weights.append(4300 - (e - 8180))
        elif e < 8232:
            weights.append(2100 - (e - 8200))
        else:
            weights.append(1000 - (e - 8232))
    return seqs, weights, names

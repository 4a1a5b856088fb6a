"""The OTUs of a run (raxtax_hip.h, "OTUs of a run") as brute-force Python, and the fixtures of test_otu_cpu.py and test_gpu_otu.py.

brute_force(seqs, sizes, counts): the rows of a table in rank order.  Links: every variant the definition names -- one code deleted, one
code replaced by A, C, G or T -- is formed as bytes and looked up in a dict of the rows; OTUs: the greedy breadth-first growth, literally.
pair_links(seqs) states the link a second time, pair by pair, without forming a variant."""
import functools

import numpy as np

import raxtax_amd as rx
from tally_common import concat, random_seq

MAX_LEN = 4096
PLAIN = (1, 2, 4, 8)
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 658, 4095, 4096)
N, R = 15, 5


def brute_links(rows):
    """rows: bytes in rank order.  (sorted list of (a, b), a < b; the number of rows above MAX_LEN)"""
    rank = {s: r for r, s in enumerate(rows)}
    assert len(rank) == len(rows)
    links, long_rows = set(), 0
    for x, s in enumerate(rows):
        if len(s) > MAX_LEN:
            long_rows += 1
            continue
        for i in range(len(s)):
            head, tail = s[:i], s[i + 1:]
            variants = [head + bytes((c,)) + tail for c in PLAIN if c != s[i]]
            if len(s) > 1:
                variants.append(head + tail)
            for v in variants:
                y = rank.get(v)
                if y is not None:
                    links.add((min(x, y), max(x, y)))
    return sorted(links), long_rows


def linked(a, b):
    """the definition for one pair of rows (numpy uint8), without forming a variant"""
    if len(a) > MAX_LEN or len(b) > MAX_LEN:
        return False
    if len(a) == len(b):
        d = np.flatnonzero(a != b)
        return len(d) == 1 and (int(a[d[0]]) in PLAIN or int(b[d[0]]) in PLAIN)
    if len(a) < len(b):
        a, b = b, a
    if len(a) != len(b) + 1:
        return False
    d = np.flatnonzero(a[:-1] != b)
    i = int(d[0]) if len(d) else len(b)
    return bool(np.array_equal(a[i + 1:], b[i:]))


def pair_links(seqs):
    by_len = {}
    for r, s in enumerate(seqs):
        by_len.setdefault(len(s), []).append(r)
    out = []
    for n, rs in by_len.items():
        for x in rs:
            out += [(min(x, y), max(x, y)) for y in rs if y > x and linked(seqs[x], seqs[y])]
            out += [(min(x, y), max(x, y)) for y in by_len.get(n - 1, []) if linked(seqs[x], seqs[y])]
    return sorted(out)


def brute_force(seqs, sizes, counts):
    """dict(links [n, 2], long_rows, otu, seed, members, sizes, counts) of the rows (numpy uint8 arrays) in rank order"""
    n = len(seqs)
    links, long_rows = brute_links([bytes(s) for s in seqs])
    adj = [[] for _ in range(n)]
    for a, b in links:
        adj[a].append(b)
        adj[b].append(a)
    otu, seed = [None] * n, []
    for s in range(n):                       # 1. the unassigned row of lowest rank is a seed
        if otu[s] is not None:
            continue
        k = len(seed)
        seed.append(s)
        otu[s] = k
        queue = [s]
        for x in queue:                      # 2. breadth-first: x pulls in every unassigned linked y with size[y] <= size[x]
            for y in adj[x]:
                if otu[y] is None and sizes[y] <= sizes[x]:
                    otu[y] = k
                    queue.append(y)
    counts = np.asarray(counts, np.uint64).reshape(n, -1)
    per_otu = np.zeros((len(seed), counts.shape[1]), np.uint64)
    for r in range(n):
        per_otu[otu[r]] += counts[r]
    return dict(links=np.array(links, np.uint32).reshape(-1, 2), long_rows=long_rows, otu=np.array(otu, np.uint32), seed=np.array(seed, np.uint32),
                members=np.bincount(np.array(otu, np.int64), minlength=len(seed)).astype(np.uint64), sizes=per_otu.sum(axis=1), counts=per_otu)


def assert_otus(got, want):
    """an rx.Otus against a brute_force() dict or another rx.Otus: every field but rounds and link_passes, no tolerance"""
    w = want if isinstance(want, dict) else {k: getattr(want, k) for k in ("links", "long_rows", "otu", "seed", "members", "sizes", "counts")}
    assert got.n_rows == len(w["otu"]) and got.n_otus == len(w["seed"])
    assert got.links.shape == w["links"].shape and np.array_equal(got.links, w["links"]), (len(got.links), len(w["links"]))
    assert got.long_rows == w["long_rows"]
    for k in ("otu", "seed", "members", "sizes", "counts"):
        assert getattr(got, k).shape == w[k].shape and np.array_equal(getattr(got, k), w[k]), k


def table_of(seqs, weight=None, sample=None, samples=0):
    return rx.tally_reads(*concat(seqs), sample, None if weight is None else np.asarray(weight, np.uint32), samples=samples)


def brute_of(table):
    return brute_force(table.seqs, table.sizes, table.counts)


def other(rng, c):
    return int(rng.choice([p for p in PLAIN if p != c]))


def with_sub(rng, s, i):
    t = s.copy()
    t[i] = other(rng, s[i])
    return t


def without(s, i):
    return np.delete(s, i)


@functools.lru_cache(maxsize=None)
def edge_rows(seed=5):
    """(seqs, weight, marks): about 190 distinct rows.  For every length of LENGTHS a random base row; a substitution and a deletion at 0, 7, 8
    and the last position; the row one code longer (an insertion at 0, 8, the end); one deletion out of a run of four equal codes that
    straddles a word boundary (deleting the first, an inner or the last code of the run gives this one row).  marks: name -> (x, y, linked)
    pairs of sequences the tests look up."""
    rng = np.random.default_rng(seed)
    seqs, marks = [], {}
    for n in LENGTHS:
        base = random_seq(rng, n)
        run = 14 if n >= 19 else 6 if n >= 11 else None   # the run lies over the boundary at 16 or 8, away from the other edits
        if run is not None:
            base[run:run + 4] = base[run]
            base[run - 1] = other(rng, base[run])
            base[run + 4] = other(rng, base[run])
        seqs.append(base)
        for i in sorted({0, 7, 8, n - 1}):
            if i >= n:
                continue
            seqs.append(with_sub(rng, base, i))
            marks[f"sub {n} {i}"] = (base, seqs[-1], True)
            if n > 1:
                seqs.append(without(base, i))
                marks[f"del {n} {i}"] = (base, seqs[-1], True)
        for i in sorted({0, min(8, n), n}):
            seqs.append(np.insert(base, i, other(rng, base[min(i, n - 1)])))
            marks[f"ins {n} {i}"] = (base, seqs[-1], n < MAX_LEN)   # (a row of 4097 codes has no link)
        if run is not None:
            seqs.append(without(base, run + 1))
            assert all(np.array_equal(seqs[-1], without(base, run + k)) for k in range(4))
            marks[f"run {n}"] = (base, seqs[-1], True)
    # ambiguity codes
    b = random_seq(rng, 64)
    n_, r_ = b.copy(), b.copy()
    n_[5], r_[5] = N, R
    ins_n = np.insert(b, 20, N)
    seqs += [b, n_, r_, ins_n]
    marks.update({"N base": (b, n_, True), "R base": (b, r_, True), "N R": (n_, r_, False), "deleted N": (ins_n, b, True)})
    # what is no link
    c = random_seq(rng, 70)
    c[30], c[31] = 1, 2
    two = with_sub(rng, with_sub(rng, c, 3), 40)
    sub_del = without(with_sub(rng, c, 3), 40)
    swap = c.copy()
    swap[30], swap[31] = c[31], c[30]
    rot = np.roll(c, 1)
    seqs += [c, two, sub_del, swap, rot]
    marks.update({"two subs": (c, two, False), "one of each": (c, sub_del, False), "transposition": (c, swap, False), "rotation": (c, rot, False)})
    keys = [bytes(s) for s in seqs]
    keep = [i for i, k in enumerate(keys) if k not in keys[:i]]
    seqs = [seqs[i] for i in keep]
    weight = rng.integers(1, 6, len(seqs)).astype(np.uint32)
    return seqs, weight, marks


@functools.lru_cache(maxsize=None)
def edge_case():
    """(table, brute force, marks) of edge_rows(): computed once, shared, never changed"""
    seqs, weight, marks = edge_rows()
    table = table_of(seqs, weight)
    return table, brute_of(table), marks


def chain(rng, n, length=60):
    """n rows, each one substitution away from the one before and at least two from every other"""
    rows = [random_seq(rng, length)]
    for k in range(1, n):
        rows.append(with_sub(rng, rows[-1], k - 1))
    return rows


@functools.lru_cache(maxsize=None)
def cluster_case(seed=9):
    """(table, brute force, named): the clustering cases in one table of two columns.  Every row is given as two reads, one per sample, whose
    weights add up to the size the case wants.  named: name -> bytes of a row."""
    rng = np.random.default_rng(seed)
    seqs, sizes, named = [], [], {}

    def put(name, s, size):
        seqs.append(s)
        sizes.append(size)
        named[name] = bytes(s)

    for k, s in enumerate(chain(rng, 40)):               # a descending chain: one OTU, about 40 rounds
        put(f"chain{k}", s, 400 - k)
    for name, s, size in zip(("valley10", "valley2", "valley9"), chain(rng, 3), (210, 2, 209)):    # 10-2-9: the 2 goes to the 10, the 9 is a seed
        put(name, s, size)
    for name, s, size in zip(("up10", "up5", "up7"), chain(rng, 3), (220, 5, 7)):                  # 10-5-7: the 7 is a seed
        put(name, s, size)
    plateau = chain(rng, 5)                               # five rows of one size, entered from the middle one
    for k, s in enumerate(plateau):
        put(f"plateau{k}", s, 6)
    put("plateau_head", with_sub(rng, plateau[2], 50), 230)
    base = random_seq(rng, 60)                            # one row linked to two seeds that are not linked to each other
    mid = with_sub(rng, base, 3)
    put("seed_a", base, 250)
    put("seed_b", with_sub(rng, mid, 9), 240)
    put("between", mid, 3)
    n = len(seqs)
    w1 = np.array([k % 3 for k in range(n)], np.uint32)
    w0 = np.array(sizes, np.uint32) - w1
    table = table_of(seqs + seqs, np.concatenate([w0, w1]), np.repeat(np.array([0, 1], np.uint32), n), samples=2)
    return table, brute_of(table), named


def ranks(table):
    return {bytes(s): r for r, s in enumerate(table.seqs)}


def seq(text):
    return np.array([{"A": 1, "C": 2, "G": 4, "T": 8, "N": 15, "R": 5}[c] for c in text], np.uint8)


def check_clusters(table, got, named):
    """what the cases were built to show, on any result"""
    by_bytes = ranks(table)
    rank = {k: by_bytes[v] for k, v in named.items()}
    otu = got.otu
    assert len({otu[rank[f"chain{k}"]] for k in range(40)}) == 1 and got.seed[otu[rank["chain0"]]] == rank["chain0"]
    assert got.members[otu[rank["chain0"]]] == 40
    assert otu[rank["valley2"]] == otu[rank["valley10"]] != otu[rank["valley9"]] and got.seed[otu[rank["valley9"]]] == rank["valley9"]
    assert otu[rank["up5"]] == otu[rank["up10"]] != otu[rank["up7"]] and got.seed[otu[rank["up7"]]] == rank["up7"]
    assert {otu[rank[f"plateau{k}"]] for k in range(5)} == {otu[rank["plateau_head"]]}
    order = [rank[f"plateau{k}"] for k in range(5)]
    assert min(order) < rank["plateau2"] < max(order)                  # the plateau is entered at a rank between its others: labels run both ways
    assert rank["seed_a"] < rank["seed_b"] and otu[rank["between"]] == otu[rank["seed_a"]] != otu[rank["seed_b"]]
    assert got.columns == 2 and got.counts.shape == (got.n_otus, 2)
    sums = np.zeros((got.n_otus, 2), np.uint64)
    np.add.at(sums, otu.astype(np.int64), table.counts)
    assert np.array_equal(got.counts, sums) and np.array_equal(got.sizes, sums.sum(axis=1)) and (table.counts[:, 1] > 0).any()
    assert list(got.seed) == sorted(got.seed) and np.array_equal(otu[got.seed], np.arange(got.n_otus))

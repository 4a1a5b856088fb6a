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
    links, long_rows = brute_links([bytes(s) for s in seqs])
    return grow(len(seqs), links, long_rows, sizes, counts)


def grow(n, links, long_rows, sizes, counts):
    """the OTUs over a sorted list of links (a, b), a < b: the greedy breadth-first growth, literally"""
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
    np.add.at(per_otu, np.array(otu, np.int64), counts)
    return dict(links=np.array(links, np.uint32).reshape(-1, 2), long_rows=long_rows, otu=np.array(otu, np.uint32), seed=np.array(seed, np.uint32),
                members=np.bincount(np.array(otu, np.int64), minlength=len(seed)).astype(np.uint64), sizes=per_otu.sum(axis=1), counts=per_otu)


def equal_length_force(seqs, sizes, counts):
    """brute_force() said a second time for rows of ONE length over A, C, G, T alone, vectorised: a row is the integer of its base-4
    digits, the substitution of digit d_i by c is key + (c - d_i) 4^i, and a variant is looked up with a binary search in the sorted keys.
    Rows of one length have no deletion link.  The growth is grow(), as in brute_force()."""
    rows = np.stack([np.asarray(s, np.uint8) for s in seqs])
    n, length = rows.shape
    assert length <= 31 and np.isin(rows, PLAIN).all()
    digit = np.zeros(16, np.int64)
    digit[list(PLAIN)] = np.arange(4)
    d = digit[rows]
    keys = (d << (2 * np.arange(length, dtype=np.int64))).sum(axis=1)
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    assert (np.diff(sorted_keys) > 0).all()
    pairs = []
    for i in range(length):
        for c in range(4):
            x = np.flatnonzero(d[:, i] != c)
            variant = keys[x] + ((c - d[x, i]) << (2 * i))
            at = np.minimum(np.searchsorted(sorted_keys, variant), n - 1)
            hit = sorted_keys[at] == variant
            y = order[at[hit]]
            x = x[hit]
            pairs.append(np.stack([x[x < y], y[x < y]], axis=1))   # every link is found from both of its rows: kept from the lower one
    links = np.concatenate(pairs)
    links = links[np.lexsort((links[:, 1], links[:, 0]))]
    return grow(n, [(int(a), int(b)) for a, b in links], 0, sizes, counts)


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


WEIGHTINGS = ("equal", "three", "distinct")


@functools.lru_cache(maxsize=None)
def complete_case(weighting, seed=17):
    """(table, brute force): the complete world -- all 1 024 rows of 5 codes and all 4 096 rows of 6 codes over A, C, G, T: 5 120 rows in 20
    blocks of 256, 64 000 links (36 864 + 7 680 substitutions, 1 024 x 19 deletions), which is more than the 4 n links the first pass has room
    for.  equal: one size, every link runs both ways, one OTU; three: sizes from {1, 2, 3}, a dense plateau with borders; distinct: no link
    runs both ways."""
    rng = np.random.default_rng(seed)
    codes = np.array(PLAIN, np.uint8)
    seqs = [codes[(k >> (2 * np.arange(length))) & 3] for length in (5, 6) for k in range(4 ** length)]
    n = len(seqs)
    weight = {"equal": np.ones(n, np.uint32), "three": rng.integers(1, 4, n).astype(np.uint32), "distinct": (rng.permutation(n) + 1).astype(np.uint32)}[weighting]
    table = table_of([seqs[i] for i in rng.permutation(n)], weight)
    return table, brute_of(table)


COMPLETE_LINKS = 36864 + 7680 + 1024 * 19
COMPLETE_MASK = 0xFF00000000000003   # the top 8 bits of the slot and two bits of the tag: 256 chains of about 20 rows in the 16 384 slots


def check_complete(table, got, weighting):
    """what the complete world was built to show, on any result"""
    sizes = table.sizes
    assert got.n_rows == 5120 and len(got.links) == COMPLETE_LINKS == 64000 and COMPLETE_LINKS > 4 * got.n_rows
    assert got.long_rows == 0 and int(got.members.sum()) == 5120
    a, b = got.links[:, 0].astype(np.int64), got.links[:, 1].astype(np.int64)
    two_way = int((sizes[a] == sizes[b]).sum())
    if weighting == "equal":
        assert two_way == COMPLETE_LINKS and got.n_otus == 1 and got.seed.tolist() == [0] and got.members.tolist() == [5120] and not got.otu.any()
    elif weighting == "three":
        assert 0 < two_way < COMPLETE_LINKS     # (rank 0 has the largest size and the rows of that size are connected: still one OTU, by the definition)
    else:
        assert two_way == 0 and 1 < got.n_otus < 5120


BLOCK_EDGES = (255, 256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def block_case(n, last):
    """(table, brute force, planted): n rows of 20 random codes at distinct falling sizes, so that row k of the list has rank k.  The last row
    is a seed (last = "seed": a random row) or a substitution of row 0 (last = "variant": it lies in OTU 0, across every block edge in
    front of it); the rows 256 .. 259 that are not the last one are variants of rows of block 0, links across the edge at 256.
    planted: the (a, b) pairs, a < b, that were built as links."""
    assert last in ("seed", "variant")
    rng = np.random.default_rng(1000 + n)
    seqs = [random_seq(rng, 20) for _ in range(n)]
    planted = []
    for k in range(256, min(n - 1, 260)):
        a = 255 - 3 * (k - 256)
        seqs[k] = with_sub(rng, seqs[a], k - 250) if k % 2 == 0 else without(seqs[a], k - 250)
        planted.append((a, k))
    if last == "variant":
        seqs[n - 1] = with_sub(rng, seqs[0], 3)
        planted.append((0, n - 1))
    table = table_of(seqs, np.arange(2 * n, n, -1, dtype=np.uint32))
    assert [bytes(s) for s in table.seqs] == [bytes(s) for s in seqs]
    return table, brute_of(table), planted


def check_blocks(got, n, planted):
    assert got.links.tolist() == [list(l) for l in sorted(planted)]
    assert got.n_otus == n - len(planted) and all(got.otu[b] == got.otu[a] for a, b in planted)
    assert (got.seed[got.otu[n - 1]] == n - 1) == ((0, n - 1) not in planted)


MANY = 65537


@functools.lru_cache(maxsize=None)
def many_blocks_case(seed=23):
    """(table, restatement): exactly 65 537 distinct rows of 12 random codes over A, C, G, T at sizes from 1 .. 4: 257 blocks of 256, the last
    one holding row 65 536 alone -- the second pass of the scan of the block sums.  Nearly every row is a seed: every block adds to the
    numbering.  The reference is equal_length_force() (test_otu_cpu.py holds it against brute_force() on the complete world's 6-mers)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((0, 12), np.uint8)
    while len(rows) < MANY:                  # duplicates are drawn again until the count is exact
        more = np.array(PLAIN, np.uint8)[rng.integers(0, 4, (MANY - len(rows), 12))]
        both = np.concatenate([rows, more])
        _, first = np.unique(both, axis=0, return_index=True)
        rows = both[np.sort(first)]
    assert rows.shape == (MANY, 12)
    table = table_of(list(rows), rng.integers(1, 5, MANY).astype(np.uint32))
    assert len(table.seqs) == MANY
    return table, equal_length_force(table.seqs, table.sizes, table.counts)

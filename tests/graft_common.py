"""Fastidious grafting (raxtax_hip.h, "Fastidious grafting") as brute-force Python, and the fixtures of test_graft_cpu.py, test_gpu_graft.py
and test_cli_graft_gpu.py.  The definition is stated twice, independently:
  (a) restate(): the balls B1 as Python bytes in a dict (a string of more than 64 bytes goes in as its length and a 128-bit digest, so
      that the balls of the rows of 4 096 codes fit), parents, grafts, renumbering, sums;
  (b) near(): pair by pair, without forming a variant -- Levenshtein distance <= 2 by dynamic programming, for rows over A, C, G, T.
plain_force() says (a) a third time for rows of one length over A, C, G, T, vectorised, for the world of 74 000 rows."""
import functools
import hashlib

import numpy as np

import raxtax_amd as rx
from otu_common import LENGTHS, MAX_LEN, PLAIN, brute_of, other, table_of, with_sub, without
from tally_common import random_seq

NONE = 0xFFFFFFFF
N, R, Y = 15, 5, 10


def ball(s: bytes):
    """B1(s), literally"""
    n = len(s)
    if n == 0 or n > MAX_LEN:
        return set()
    out = {s}
    for i in range(n):
        out.update(s[:i] + bytes((c,)) + s[i + 1:] for c in PLAIN if c != s[i])
        if n >= 2:
            out.add(s[:i] + s[i + 1:])
    if n + 1 <= MAX_LEN:
        for i in range(n + 1):
            out.update(s[:i] + bytes((c,)) + s[i:] for c in PLAIN)
    return out


def _key(v: bytes):
    return v if len(v) <= 64 else (len(v), hashlib.blake2b(v, digest_size=16).digest())


def finish(otus, sizes, counts, parent, boundary):
    """the result from the parents: dict(otu, seed, members, sizes, counts, parent, old_to_new, grafts [n, 5], heavy_otus, light_otus, ...)"""
    otu = np.asarray(otus["otu"], np.int64)
    n, no = len(otu), len(otus["seed"])
    heavy_otu = np.asarray(otus["sizes"], np.uint64) >= boundary
    best = {}
    for x in range(n):
        if parent[x] != NONE:
            k = int(otu[x])
            best[k] = min(best.get(k, (NONE, NONE)), (int(parent[x]), x))
    old_to_new = np.full(no, NONE, np.uint32)
    seed = [int(otus["seed"][k]) for k in range(no) if k not in best]
    old_to_new[[k for k in range(no) if k not in best]] = np.arange(len(seed))
    grafts = []
    for k in sorted(best):
        p, x = best[k]
        assert heavy_otu[otu[p]] and not heavy_otu[k]
        old_to_new[k] = old_to_new[otu[p]]
        grafts.append((k, x, p, int(otu[p]), int(old_to_new[otu[p]])))
    new = old_to_new[otu].astype(np.int64)
    counts = np.asarray(counts, np.uint64).reshape(n, -1)
    per = np.zeros((len(seed), counts.shape[1]), np.uint64)
    np.add.at(per, new, counts)
    return dict(otu=new.astype(np.uint32), seed=np.array(seed, np.uint32), members=np.bincount(new, minlength=len(seed)).astype(np.uint64), sizes=per.sum(axis=1), counts=per,
                parent=np.asarray(parent, np.uint32), old_to_new=old_to_new, grafts=np.array(grafts, np.uint32).reshape(-1, 5), links=np.asarray(otus["links"]),
                long_rows=otus["long_rows"], heavy_otus=int(heavy_otu.sum()), light_otus=int((~heavy_otu).sum()), heavy_rows=int(heavy_otu[otu].sum()),
                light_rows=int((~heavy_otu[otu]).sum()), boundary=boundary)


def restate(seqs, sizes, counts, otus, boundary=3):
    """(a): otus is a brute_force() dict (or anything with otu, seed, sizes, links, long_rows)"""
    otu = np.asarray(otus["otu"], np.int64)
    heavy = (np.asarray(otus["sizes"], np.uint64) >= boundary)[otu]
    lowest = {}
    for y in np.flatnonzero(heavy):
        for v in ball(bytes(seqs[y])):
            lowest.setdefault(_key(v), int(y))          # (rows come in rank order: the first one is the lowest)
    parent = np.full(len(seqs), NONE, np.uint32)
    if lowest:
        for x in np.flatnonzero(~heavy):
            parent[x] = min((lowest.get(_key(v), NONE) for v in ball(bytes(seqs[x]))), default=NONE)
    return finish(otus, sizes, counts, parent, boundary)


def near(a, b):
    """(b): rows over A, C, G, T of 1 .. MAX_LEN codes are near iff their Levenshtein distance is at most 2"""
    if not (1 <= len(a) <= MAX_LEN and 1 <= len(b) <= MAX_LEN) or abs(len(a) - len(b)) > 2:
        return False
    a, b = bytes(a), bytes(b)
    prev = {j: j for j in range(min(len(b), 2) + 1)}    # the band |i - j| <= 2 of the table; what lies outside it is above 2
    for i in range(1, len(a) + 1):
        cur = {}
        for j in range(max(0, i - 2), min(len(b), i + 2) + 1):
            cur[j] = min(prev.get(j, 9) + 1, cur.get(j - 1, 9) + 1, prev.get(j - 1, 9) + (a[i - 1] != b[j - 1]) if j else 9)
        if min(cur.values()) > 2:
            return False
        prev = cur
    return prev.get(len(b), 9) <= 2


def pair_parents(seqs, heavy):
    """parent[] from near() alone, for the rows over A, C, G, T (every other row: NONE)"""
    ok = [bool(np.isin(s, PLAIN).all()) for s in seqs]
    hs = [y for y in np.flatnonzero(heavy) if ok[y]]
    parent = np.full(len(seqs), NONE, np.uint32)
    for x in np.flatnonzero(~np.asarray(heavy)):
        if ok[x]:
            parent[x] = next((y for y in hs if near(seqs[x], seqs[y])), NONE)
    return parent


def plain_force(seqs, sizes, counts, otus, boundary=3):
    """(a) said again for rows of ONE length <= 14 over A, C, G, T, vectorised: a string is the integer 4^len + sum d_i 4^i, and every string
    of every ball is formed with integer arithmetic over all rows at once.  test_graft_cpu.py holds it against restate() on the parity world."""
    rows = np.stack([np.asarray(s, np.uint8) for s in seqs])
    n, length = rows.shape
    assert 2 <= length <= 14 and np.isin(rows, PLAIN).all()
    digit = np.zeros(16, np.int64)
    digit[list(PLAIN)] = np.arange(4)
    d = digit[rows]
    pw = 4 ** np.arange(length + 2, dtype=np.int64)
    key = (d * pw[:length]).sum(axis=1) + pw[length]
    cols = [key]
    for i in range(length):
        low, high = key % pw[i], key // pw[i + 1]
        cols += [key + (c - d[:, i]) * pw[i] for c in range(4)]            # (c = d_i gives the row itself again: harmless in a set)
        cols.append(low + high * pw[i])
    for i in range(length + 1):
        low, high = key % pw[i], key // pw[i]
        cols += [low + c * pw[i] + high * pw[i + 1] for c in range(4)]
    balls = np.stack(cols, axis=1)                                            # [n, strings]
    otu = np.asarray(otus["otu"], np.int64)
    heavy = (np.asarray(otus["sizes"], np.uint64) >= boundary)[otu]
    hy = np.flatnonzero(heavy)
    flat = balls[hy].ravel()
    who = np.repeat(hy, balls.shape[1])
    order = np.lexsort((who, flat))
    flat, who = flat[order], who[order]
    first = np.concatenate([[True], flat[1:] != flat[:-1]]) if len(flat) else np.zeros(0, bool)
    keys, lowest = flat[first], who[first]
    parent = np.full(n, NONE, np.uint32)
    lx = np.flatnonzero(~heavy)
    if len(keys) and len(lx):
        at = np.minimum(np.searchsorted(keys, balls[lx]), len(keys) - 1)
        hit = keys[at] == balls[lx]
        parent[lx] = np.where(hit, lowest[at], NONE).min(axis=1)
    return finish(otus, sizes, counts, parent, boundary)


RESULT_FIELDS = ("otu", "seed", "members", "sizes", "counts", "parent", "old_to_new", "grafts", "links")
INFO_FIELDS = ("boundary", "heavy_otus", "light_otus", "heavy_rows", "light_rows")


def assert_graft(got, want):
    """an rx.Otus made by otu_graft / otu_graft_host against a restate() dict or another such Otus: every field but the filter's counters"""
    if isinstance(want, dict):
        w, info = want, want
    else:
        w, info = {k: getattr(want, k) for k in RESULT_FIELDS + ("long_rows", "rounds", "link_passes")}, want.graft_info
        assert got.rounds == want.rounds and got.link_passes == want.link_passes
    assert got.n_rows == len(w["otu"]) and got.n_otus == len(w["seed"]) and got.long_rows == w["long_rows"]
    for k in RESULT_FIELDS:
        assert getattr(got, k).shape == np.asarray(w[k]).shape and np.array_equal(getattr(got, k), w[k]), k
    for k in INFO_FIELDS:
        assert got.graft_info[k] == info[k], k
    assert got.graft_info["grafts"] == len(w["grafts"])


def restate_of(table, otus, boundary=3):
    """restate() of a table and its d = 1 clustering (a brute_force() dict or an rx.Otus)"""
    o = otus if isinstance(otus, dict) else {k: getattr(otus, k) for k in ("otu", "seed", "sizes", "links", "long_rows")}
    return restate(table.seqs, table.sizes, table.counts, o, boundary)


def apply_edits(base, edits):
    """edits: (kind, position, code) on positions of `base`, applied from the highest position down so that they stay those of the base"""
    s = base.copy()
    for kind, i, c in sorted(edits, key=lambda e: -e[1]):
        if kind == "sub":
            s[i] = c
        elif kind == "del":
            s = np.delete(s, i)
        else:
            s = np.insert(s, i, c)
    return s


KINDS = (("sub", "sub"), ("sub", "del"), ("sub", "ins"), ("del", "del"), ("ins", "ins"), ("del", "ins"))


@functools.lru_cache(maxsize=None)
def edge_world(seed=7):
    """(table, d = 1 brute force, restatement at B = 3, marks).  For every length n of LENGTHS a heavy base row of size 5 and light rows of
    size 1 two edits away: every pair of kinds of KINDS at positions from {0, 7, 8, n - 1, n} -- both in one word, in adjacent words, at both
    ends; n + 1 gains a word at 8, 16, 64, 512 and n - 1 loses one at 9, 17, 65, 513; no deletion of the only code, no insertion into 4 096
    codes.  One row three substitutions away per base (it must stay), a run of equal codes over a word boundary with that code inserted
    beside it, a row of 4 097 codes (no ball), ambiguity codes.  marks: name -> bytes of a row."""
    rng = np.random.default_rng(seed)
    seqs, weight, marks = [], [], {}

    def put(s, w, name=None):
        if len(s) and bytes(s) not in {bytes(t) for t in seqs[-80:]}:
            seqs.append(np.asarray(s, np.uint8))
            weight.append(w)
            if name:
                marks[name] = bytes(s)

    for n in LENGTHS:
        base = random_seq(rng, n)
        if n >= 11:
            base[6:10] = base[6]                     # a run over the boundary at 8
            base[5], base[10] = other(rng, base[6]), other(rng, base[6])
        put(base, 5, f"base {n}")
        spots = [(0, 7), (7, 8), (0, n - 1), (8, n - 1)] if n <= 1000 else [(7, n - 1)]
        for k1, k2 in KINDS:
            for p, q in spots:
                if k2 == "ins" and q == n - 1:
                    q = n                            # behind the end
                if not (0 <= p < q and p < n and q < n + (k2 == "ins")):
                    continue
                e1 = (k1, p, other(rng, base[p]))
                e2 = (k2, q, other(rng, base[min(q, n - 1)]))
                put(apply_edits(base, [e1, e2]), 1)
        if n >= 12:
            put(apply_edits(base, [("ins", 8, base[6]), ("sub", 11, other(rng, base[11]))]), 1, f"run {n}")
        if n >= 7:                                   # three substitutions, away from the positions of the other edits
            put(subs(rng, base, (2, 4, n - 2)), 1, f"far {n}")
        else:                                        # three codes more
            put(np.concatenate([base, np.repeat(base[-1:], 3)]), 1, f"far {n}")
    long_base = random_seq(rng, MAX_LEN + 1)         # 4 097 codes: no ball, heavy or light
    put(long_base, 5, "long heavy")
    put(with_sub(rng, long_base, 100), 1, "long light")
    b = random_seq(rng, 64)                          # an N and a substitution against a plain heavy row
    with_n = with_sub(rng, b, 30)
    with_n[5] = N
    put(b, 5, "plain for N")
    put(with_n, 1, "N light")
    c = random_seq(rng, 70)                          # two different ambiguity codes at one position: either becomes the same plain row
    with_r, with_y = c.copy(), c.copy()
    with_r[10], with_y[10] = R, Y
    put(with_r, 5, "R heavy")
    put(with_y, 1, "Y light")
    table = table_of(seqs, np.array(weight, np.uint32))
    d1 = brute_of(table)
    return table, d1, restate(table.seqs, table.sizes, table.counts, d1, 3), marks


def rank_of(table):
    return {bytes(s): r for r, s in enumerate(table.seqs)}


def check_edges(table, got, marks):
    """what the edge world was built to show, on any result (the device's, the host's, the restatement's as an Otus-like object)"""
    by_bytes = rank_of(table)
    rank = {k: by_bytes[v] for k, v in marks.items()}
    parent = got["parent"] if isinstance(got, dict) else got.parent
    grafts = got["grafts"] if isinstance(got, dict) else got.grafts
    otu = got["otu"] if isinstance(got, dict) else got.otu
    for n in LENGTHS:
        if True:
            assert parent[rank[f"far {n}"]] == NONE and otu[rank[f"far {n}"]] != otu[rank[f"base {n}"]], n
        if n >= 12:                                  # (4 096 codes and one more: no ball)
            assert parent[rank[f"run {n}"]] == (rank[f"base {n}"] if n < MAX_LEN else NONE), n
    assert parent[rank["long light"]] == NONE and parent[rank["long heavy"]] == NONE
    assert parent[rank["N light"]] == rank["plain for N"] and parent[rank["Y light"]] == rank["R heavy"]
    assert len(grafts) >= 150                        # (of about 180 light OTUs; light rows that share an edit are linked to each other)


@functools.lru_cache(maxsize=None)
def small_edge_world(seed=3):
    """(table, d = 1 brute force, restatement): the edge world in small -- bases of 7, 8, 9 and 17 codes -- for the runs in which every
    string is a candidate"""
    rng = np.random.default_rng(seed)
    seqs, weight = [], []
    for n in (7, 8, 9, 17):
        base = random_seq(rng, n)
        seqs.append(base)
        weight.append(5)
        for k1, k2 in KINDS:
            p, q = (0, n if k2 == "ins" else n - 1) if (k1, k2) != ("sub", "sub") else (7 % n, n - 1)
            if p == q:
                p = 0
            seqs.append(apply_edits(base, [(k1, p, other(rng, base[p])), (k2, q, other(rng, base[min(q, n - 1)]))]))
            weight.append(1)
        far = base.copy()
        far[[0, 3, n - 1]] = [other(rng, base[i]) for i in (0, 3, n - 1)]
        seqs.append(far)
        weight.append(1)
    keys = [bytes(s) for s in seqs]
    keep = [i for i, k in enumerate(keys) if k not in keys[:i]]
    table = table_of([seqs[i] for i in keep], np.array([weight[i] for i in keep], np.uint32))
    d1 = brute_of(table)
    return table, d1, restate(table.seqs, table.sizes, table.counts, d1, 3)


def subs(rng, s, at):
    t = s.copy()
    for i in at:
        t[i] = other(rng, s[i])
    return t


@functools.lru_cache(maxsize=None)
def rule_world(seed=29):
    """(table, d = 1 brute force, named): the cases of the rule on rows of 40 codes; named: name -> bytes"""
    rng = np.random.default_rng(seed)
    seqs, weight, named = [], [], {}

    def put(name, s, w):
        seqs.append(s)
        weight.append(w)
        named[name] = bytes(s)

    h1 = random_seq(rng, 40)                          # two members near different heavy OTUs: the lower parent wins
    h2 = subs(rng, h1, range(5))
    m1 = h1.copy()
    m1[:2] = h2[:2]
    m2 = m1.copy()
    m2[2] = h2[2]
    put("h1", h1, 9), put("h2", h2, 8), put("m1", m1, 1), put("m2", m2, 1)
    h3 = random_seq(rng, 40)                          # both members near one heavy row: the lower child wins
    m3 = subs(rng, h3, (0, 1))
    m4 = m3.copy()
    m4[1] = next(c for c in PLAIN if c not in (h3[1], m3[1]))
    put("h3", h3, 7), put("m3", m3, 1), put("m4", m4, 1)
    s5 = random_seq(rng, 40)                          # the parent is a member of its OTU that is no seed
    mem = subs(rng, s5, (20,))
    put("s5", s5, 6), put("member5", mem, 2), put("child5", subs(rng, mem, (21, 22)), 1)
    h6 = random_seq(rng, 40)                          # light - light - heavy: the middle one is grafted, the outer one is not
    mid = subs(rng, h6, (0, 1))
    put("h6", h6, 6), put("middle6", mid, 1), put("outer6", subs(rng, mid, (2, 3)), 1)
    t7 = random_seq(rng, 40)                          # three rows of size 1 are a heavy OTU; a lone row of size 2 outranks its seed
    t7b = subs(rng, t7, (30,))
    put("three0", t7, 1), put("three1", t7b, 1), put("three2", subs(rng, t7b, (31,)), 1), put("lone2", subs(rng, t7, (0, 1)), 2)
    for size in (1, 2, 3, 9, 10):                     # the boundary: a row of size B is heavy, one of B - 1 is light
        base = random_seq(rng, 40)
        put(f"size{size}", base, size), put(f"beside{size}", subs(rng, base, (4, 5)), 1)
    pair = random_seq(rng, 40)                        # the TOTAL decides: 2 + 1 is heavy at B = 3
    put("pair2", pair, 2), put("pair1", subs(rng, pair, (9,)), 1), put("beside_pair", subs(rng, pair, (10, 11)), 1)
    table = table_of(seqs, np.array(weight, np.uint32))
    return table, brute_of(table), named


@functools.lru_cache(maxsize=None)
def parity_world(seed=17):
    """(table, d = 1 brute force): the 1 024 rows of six codes over A, C, G, T whose base-4 digit sum is 0 mod 4 -- no two are linked -- 256 of
    them (the first of a permutation) at size 3, the others at size 1"""
    rng = np.random.default_rng(seed)
    digits = (np.arange(4 ** 6)[:, None] >> (2 * np.arange(6))) & 3
    rows = np.array(PLAIN, np.uint8)[digits[digits.sum(axis=1) % 4 == 0]]
    assert rows.shape == (1024, 6)
    order = rng.permutation(1024)
    weight = np.ones(1024, np.uint32)
    weight[:256] = 3
    table = table_of(list(rows[order]), weight)
    return table, brute_of(table)


@functools.lru_cache(maxsize=None)
def block_world(n, last):
    """(table, d = 1 brute force, planted): n rows of 20 codes, row k at rank k.  Rows 0 .. n - 7 have falling sizes >= 3 (heavy at B = 3), the
    last six rows sizes 2, 2, 2, 2, 2, 1.  Of those, five are two substitutions away from rows 250 .. 254 + (across row 256 when n > 262: the parents lie
    in block 0, the children in the last block) and the last row is two away from row 0 (last = "grafted") or random (last = "kept").
    planted: (parent, child)."""
    assert last in ("grafted", "kept") and n >= 255
    rng = np.random.default_rng(2000 + n)
    seqs = [random_seq(rng, 20) for _ in range(n)]
    planted = []
    for k in range(n - 6, n - 1):
        a = 250 - (n - 2 - k) if n > 262 else k - (n - 6)
        seqs[k] = subs(rng, seqs[a], (3, 12))
        planted.append((a, k))
    if last == "grafted":
        seqs[n - 1] = subs(rng, seqs[0], (1, 19))
        planted.append((0, n - 1))
    weight = np.concatenate([np.arange(2 * n, n + 6, -1), [2, 2, 2, 2, 2, 1]]).astype(np.uint32)
    keep = sorted(range(n - 6, n - 1), key=lambda k: bytes(seqs[k]))          # rows of one size rank by their bytes; the last row is alone at size 1
    seqs = seqs[:n - 6] + [seqs[k] for k in keep] + [seqs[n - 1]]
    where = {k: n - 6 + i for i, k in enumerate(keep)}
    where[n - 1] = n - 1
    planted = sorted((a, where[k]) for a, k in planted)
    table = table_of(seqs, weight)
    assert [bytes(s) for s in table.seqs] == [bytes(s) for s in seqs]
    return table, brute_of(table), planted


MANY_ROWS = 74000


@functools.lru_cache(maxsize=None)
def many_world():
    """(table, d = 1 restatement, graft restatement): 74 000 rows of 12 codes as otu_common.many_blocks_case draws them, sizes 1 .. 4: more than
    65 536 OTUs before the graft, hence more than 256 blocks of them and a second round of the scan of the block sums.  The d = 1 clustering is the
    host's, the reference of the graft plain_force() at B = 3."""
    rng = np.random.default_rng(37)
    rows = np.unique(np.array(PLAIN, np.uint8)[rng.integers(0, 4, (MANY_ROWS + 2000, 12))], axis=0)
    rows = rows[rng.permutation(len(rows))[:MANY_ROWS]]
    table = table_of(list(rows), rng.integers(1, 5, MANY_ROWS).astype(np.uint32))
    d1 = rx.otu_cluster_host(table)                  # (test_otu_cpu.py holds it against the definition)
    d1 = {k: getattr(d1, k) for k in ("otu", "seed", "sizes", "links", "long_rows")}
    return table, d1, plain_force(table.seqs, table.sizes, table.counts, d1, 3)


@functools.lru_cache(maxsize=None)
def planted_world(seed=31):
    """(table, d = 1 brute force, two_edit): 40 centres of 200 codes at geometric sizes (all >= 3), and about 760 variants of size 1 in the
    probe's mix: 60 % one substitution, 20 % two substitutions, 12 % a deletion, 8 % an insertion.  two_edit: the bytes of the variants with
    two substitutions -- each has no d = 1 neighbour but its centre is two away."""
    rng = np.random.default_rng(seed)
    centres = [random_seq(rng, 200) for _ in range(40)]
    seqs = list(centres)
    weight = [max(3, int(2000 * 0.85 ** k)) for k in range(40)]
    two_edit, seen = [], {bytes(c) for c in centres}
    for k in range(760):
        c = centres[k % 40]
        u = rng.random()
        at = sorted(rng.choice(200, 2, replace=False))
        if u < 0.6:
            s = subs(rng, c, at[:1])
        elif u < 0.8:
            s = subs(rng, c, at)
        elif u < 0.92:
            s = without(c, at[0])
        else:
            s = np.insert(c, at[0], other(rng, c[at[0]]))
        if bytes(s) in seen:
            continue
        seen.add(bytes(s))
        seqs.append(s)
        weight.append(1)
        if 0.6 <= u < 0.8:
            two_edit.append(bytes(s))
    table = table_of(seqs, np.array(weight, np.uint32))
    return table, brute_of(table), two_edit


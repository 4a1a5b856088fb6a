"""The processing order of a batch (rtx_cluster.hip) against its definition, restated in numpy from the header comment of that file:

  * three multiplicative min-hashes over the 12-mers of a read (21 bits each; 2^21 - 1 where the read has no 12-mer without an N);
  * the locator table: per 12-mer the lowest position (lineage order) of a reference that holds it, dropped where the 12-mer occurs more
    than 512 times over all references;
  * a query looks up every second of its first 1 024 windows and votes: coarse bins of 2^s references (the best pair of neighbouring
    bins wins, the lowest among equals), then bins of a sixteenth inside the winning pair (again the best pair, the lowest among equals);
  * key = position << 39 | m1 << 18 | m2 >> 3 for a query with a vote, m1 << 42 | m2 << 21 | m3 for one without; with several length
    classes in the batch the class leads (class << 61 | key >> 2); a stable sort by the key.

The order decides no result, so nothing else in the suite pins the keys bit by bit; every kernel launch behind the order depends on them."""
from __future__ import annotations

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth

pytestmark = pytest.mark.gpu

N = 15
NONE21 = (1 << 21) - 1
MULT = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9)
MAX_COUNT, LOC_WIN, STRIDE, FINE = 512, 1024, 2, 16


def codes12(seq):
    """(code, valid) of every 12-base window: two bits per base, the first base highest; valid: no N inside."""
    n = len(seq) - 11
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    two = np.zeros(len(seq), np.uint64)
    for c, v in ((2, 1), (4, 2), (8, 3)):
        two[seq == c] = v
    good = np.isin(seq, (1, 2, 4, 8))
    code = np.zeros(n, np.uint64)
    valid = np.ones(n, bool)
    for j in range(12):
        code = (code << np.uint64(2)) | two[j:n + j]
        valid &= good[j:n + j]
    return code, valid


def min_hashes(seq):
    code, valid = codes12(seq)
    code = code[valid]
    if not len(code):
        return [NONE21] * 3
    return [int(((code * np.uint64(c)) >> np.uint64(43)).min()) for c in MULT]      # (uint64 arithmetic wraps: the low 64 bits of the product)


def twin(seq, which, rng):
    """A copy of `seq` with one base changed inside the window that gives min-hash `which` (0-based) and outside the windows that give
    the min-hashes in front of it: those stay, this one and the ones behind it change.  None where the windows leave no such base."""
    code, valid = codes12(seq)
    if not valid.any():
        return None
    h = [np.where(valid, (code * np.uint64(c)) >> np.uint64(43), np.uint64(1 << 22)) for c in MULT]
    arg = [int(np.argmin(x)) for x in h]
    free = [b for b in range(arg[which], arg[which] + 12) if all(not arg[j] <= b <= arg[j] + 11 for j in range(which))]
    if not free:
        return None
    out = seq.copy()
    b = int(rng.choice(free))
    out[b] = np.uint8(1 << ((int(np.log2(out[b])) + 1 + int(rng.integers(0, 3))) & 3))
    return out


def locator_table(ref_seqs_in_position_order):
    """12-mer -> lowest position, -1 where absent or too common."""
    pos_min = np.full(1 << 24, -1, np.int64)
    count = np.zeros(1 << 24, np.int64)
    for p in range(len(ref_seqs_in_position_order) - 1, -1, -1):      # descending: the lowest position is written last
        code, valid = codes12(ref_seqs_in_position_order[p])
        code = code[valid].astype(np.int64)
        np.add.at(count, code, 1)
        pos_min[code] = p
    pos_min[count > MAX_COUNT] = -1
    return pos_min, count


def bin_shift(n_refs):
    s = 8
    while ((n_refs + (1 << s) - 1) >> s) + 1 > 8192:
        s += 1
    return s


def best_pair(votes):
    """First index B with the largest votes[B] + votes[B + 1] (a zero stands behind the last bin)."""
    v = np.asarray(votes, np.int64)
    return int(np.argmax(v + np.append(v[1:], 0)))


def locate(seq, table, n_refs):
    """The 24-bit position of a query, or None where it has no vote."""
    code, valid = codes12(seq)
    code, valid = code[:LOC_WIN:STRIDE].astype(np.int64), valid[:LOC_WIN:STRIDE]
    pos = table[code[valid]]
    pos = pos[pos >= 0]
    if not len(pos):
        return None
    s = bin_shift(n_refs)
    n_bins = (n_refs + (1 << s) - 1) >> s
    B = best_pair(np.bincount(pos >> s, minlength=n_bins))
    lo = B << s
    inside = pos[(pos >= lo) & (((pos - lo) >> s) < 2)]
    fine = best_pair(np.bincount((inside - lo) >> (s - 4), minlength=2 * FINE))
    return (B * FINE + fine) & 0xFFFFFF


def key_of(seq, table, n_refs, locator):
    m1, m2, m3 = min_hashes(seq)
    loc = locate(seq, table, n_refs) if locator and len(seq) >= 12 else None
    if loc is None:
        return (m1 << 42) | (m2 << 21) | m3, "short" if len(seq) < 12 else "no_vote"
    return (loc << 39) | (m1 << 18) | (m2 >> 3), "voted"


def expected_order(seqs, table, n_refs, locator, class_limits=(262, 1030, 2054)):
    """perm[position] = query.  The classes of this file's batches: reads of up to 1 030 bases form one (fewer than 4 096 of t <= 255 ride with
    the bulk), the longer ones another; the class leads the key only where the batch holds both."""
    keys, paths = zip(*[key_of(s, table, n_refs, locator) for s in seqs])
    long_ = np.array([len(s) > class_limits[1] for s in seqs])
    keys = raw = [int(k) for k in keys]
    if long_.any() and not long_.all():
        keys = [(int(l) << 61) | (k >> 2) for k, l in zip(keys, long_)]
    return np.argsort(np.array(keys, np.uint64), kind="stable"), paths, raw


def _concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off


@pytest.fixture(scope="module")
def world():
    """About 2 000 references, one 12-mer planted into 600 of them (more than the table keeps), and the queries of every path."""
    db = synth.make_db(2000)
    rng = np.random.default_rng(77)
    bases = db.seq_bytes.copy()
    motif = (1 << rng.integers(0, 4, 12)).astype(np.uint8)
    for r in rng.choice(db.n, 600, replace=False):
        at = int(db.seq_off[r]) + int(rng.integers(0, db.length - 12))
        bases[at:at + 12] = motif
    tree = rx.Tree.new_flat(db.lineages, bases, db.seq_off)
    orig = tree.original_index().astype(np.int64)
    refs = [bases[int(db.seq_off[i]):int(db.seq_off[i + 1])] for i in orig]         # position p of the database holds reference orig[p]
    table, count = locator_table(refs)
    mcode = int(codes12(motif)[0][0])
    assert count[mcode] > MAX_COUNT and table[mcode] == -1
    ref = lambda i: bases[int(db.seq_off[i]):int(db.seq_off[i + 1])]
    seqs = [ref(int(i)).copy() for i in rng.integers(0, db.n, 100)]                  # copies
    for i in rng.integers(0, db.n, 100):                                             # 2 % variants
        s = ref(int(i)).copy()
        hit = rng.random(len(s)) < 0.02
        s[hit] = (1 << rng.integers(0, 4, int(hit.sum()))).astype(np.uint8)
        seqs.append(s)
    seqs += [(1 << rng.integers(0, 4, int(n))).astype(np.uint8) for n in rng.integers(14, 60, 60)]     # random: most have no 12-mer in the table
    seqs += [np.zeros(0, np.uint8)] + [ref(5)[:n].copy() for n in (11, 12, 13)]
    for k in range(6):                                                                # with N: one, many, all windows broken
        s = ref(20 + k).copy()
        s[rng.integers(0, len(s), (1, 5, 40, 80, 200, 400)[k])] = N
        seqs.append(s)
    for _ in range(100):                                                             # random bases around the 12-mer that is too common, at a
        lone = (1 << rng.integers(0, 4, 40)).astype(np.uint8)                        # window that is looked up (14); an N on either side, so that
        lone[14:26] = motif                                                          # no window holds a part of it (parts of it with a base of the
        lone[13] = lone[26] = N                                                      # reference beside them are in the table)
        if locate(lone, table, db.n) is None:
            break
    assert locate(lone, table, db.n) is None
    lone_at = len(seqs)
    seqs.append(lone)
    seqs += [ref(int(i))[: int(n)].copy() for i, n in zip(rng.integers(0, db.n, 20), rng.integers(20, 600, 20))]
    # Pairs that only the LATER hashes tell apart -- a wrong second or third multiplier would otherwise hide behind the position and m1:
    # a reference and its twin with the same position and m1 but another m2, and random reads without a vote that share m1 and m2
    # (m1 alone) and differ in m3 (in m2)
    n_m2 = n_m3 = 0
    for i in rng.integers(0, db.n, 400):
        a = ref(int(i)).copy()
        b = twin(a, 1, rng)
        if b is None or n_m2 >= 12:
            continue
        (ka, pa), (kb, pb) = key_of(a, table, db.n, True), key_of(b, table, db.n, True)
        if pa == pb == "voted" and ka >> 18 == kb >> 18 and ka != kb:
            seqs += [a, b]
            n_m2 += 1
    for _ in range(4000):
        a = (1 << rng.integers(0, 4, 120)).astype(np.uint8)
        b = twin(a, 2, rng)
        if b is None or n_m3 >= 12:
            continue
        (ka, pa), (kb, pb) = key_of(a, table, db.n, True), key_of(b, table, db.n, True)
        if pa == pb == "no_vote" and ka >> 21 == kb >> 21 and ka != kb:
            seqs += [a, b]
            n_m3 += 1
    assert n_m2 == 12 and n_m3 == 12
    long_q = np.concatenate([ref(100), ref(900)])[:1200].copy()                      # 1 189 windows: the last 165 only enter the min-hashes
    order = rng.permutation(len(seqs))
    seqs = [seqs[int(i)] for i in order]
    return dict(tree=tree, table=table, n_refs=db.n, seqs=seqs, long_q=long_q, motif_query=int(np.nonzero(order == lone_at)[0][0]))


@pytest.mark.parametrize("locator", [True, False])
@pytest.mark.parametrize("classes", [1, 2])
def test_order_is_the_stable_sort_of_the_restated_keys(world, locator, classes):
    seqs = list(world["seqs"]) + ([world["long_q"]] if classes == 2 else [])
    want, paths, keys = expected_order(seqs, world["table"], world["n_refs"], locator)
    # queries that the later hashes alone tell apart: equal position and m1 but another m2 (voted), equal m1 and m2 but another m3 (no vote)
    def told_apart_by_tail(path, shift):
        groups = {}
        for k, p in zip(keys, paths):
            if p == path:
                groups.setdefault(k >> shift, set()).add(k)
        return sum(len(g) > 1 for g in groups.values())
    by_m2, by_m3 = told_apart_by_tail("voted", 18), told_apart_by_tail("no_vote", 21)
    print(f"told apart by m2 alone: {by_m2} groups, by m3 alone: {by_m3} groups")
    assert by_m3 >= 12 and (by_m2 >= 12 or not locator)
    index = rx.Index(world["tree"], locator=locator)
    bases, off = _concat(seqs)
    index.classify(bases, off)
    assert len(index.batch_classes()) == classes
    got = index.debug_order(len(seqs)).astype(np.int64)
    n_paths = {p: paths.count(p) for p in ("short", "no_vote", "voted")}
    print(f"locator {locator}, {classes} classes: {len(seqs)} queries, paths {n_paths}")
    assert n_paths["short"] >= 2 and n_paths["no_vote"] >= 10
    if locator:
        assert n_paths["voted"] >= 150
        assert paths[world["motif_query"]] == "no_vote"            # its one 12-mer of the database is too common to vote
        if classes == 2:
            assert paths[-1] == "voted"
    else:
        assert n_paths["voted"] == 0
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"first difference at position {bad[0]}: query {got[bad[0]]} ({paths[got[bad[0]]]}), expected {want[bad[0]]} ({paths[want[bad[0]]]})"

"""The tails of the pair kernel's row loop on the device (hit_count_pair_kernel: the counting pass and the one-level bounds pass), on inputs
whose every count and bound has a closed form (tests/debruijn_common.py).

The three lists of a (pair, tile) block -- rows both queries share, A's alone, B's alone -- are padded to whole groups of 24 rows and run as
one pipeline; the last group of whichever list is the last of the block is folded by a body of its own that requests nothing behind it
(fold_seg, rtx_hit_pair.hip).  The pairs here are two windows (a, T), (a + d, T): T - d shared rows and d of either query alone, every row
dense in four of the five tiles (23, 17, 19 nested windows and the partial last tile) and sparse in one.  d = 0 makes the shared list the
last one, every other d B's; d walks over both sides of every multiple of 8 up to 48 = two groups, so that the lists end at every place of
a group and the last list is shorter than one group, exactly one, and longer; reads of 8 .. 25 rows give blocks whose every list is shorter
than one group, a pair of disjoint reads a block without a shared list.

The two-level bounds pass (bounds2_kernel: fold_list, groups of 128 rows at level A and of 256 at level B, the same body without loads behind
a level's last list) runs on the same windows in a database of 16 full tiles + 37: shared lists of 255 .. 257 rows beside lists of 31 .. 33
and 127 .. 129, a pair in which one window lies inside the other (A's list is the last one), a last pair of one query."""
import numpy as np
import pytest

import debruijn_common as D
import raxtax_amd as rx
from raxtax_amd.checks import assert_rows_equivalent, check_run_as_left

pytestmark = pytest.mark.gpu

T, A = D.PAIR_T, D.PAIR_A
SHIFTS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 47, 48, 49)
SHORT_T, SHORT_SHIFTS = (8, 9, 24, 25), (0, 1, 3, 8)
# tile 1 becomes dense for every query (23 nested windows in one leaf taxon); tiles 0, 2 and the last are dense by D.PLANTED, tile 3 is sparse
PLANTED = D.PLANTED + [(1, 1536 + i, 12050 - i, 1500 + 2 * i) for i in range(23)]


def queries():
    qs = []
    for d in SHIFTS:
        qs += [(A, T), (A + d, T)]
    for t in SHORT_T:
        qs += [q for d in SHORT_SHIFTS for q in ((12500 + 40 * t, t), (12500 + 40 * t + d, t))]
    return qs


def block_bounds(fam, a, t, size=64):
    """The closed form of the bounds over blocks of `size` references: the rows of the query [a, a + t) that some reference of the block
    holds -- the positions its windows cover; [tile][8192 / size] (0 behind the database)."""
    lo = np.clip(fam.start - a, 0, t)
    hi = np.clip(fam.start + fam.n_kmers - a, 0, t)
    per_tile = D.TILE // size
    d = np.zeros((fam.ntiles * per_tile, t + 1), np.int64)
    blk = np.arange(fam.n_refs) // size
    np.add.at(d, (blk, lo), 1)
    np.add.at(d, (blk, hi), -1)
    return (np.cumsum(d, axis=1)[:, :t] > 0).sum(axis=1).reshape(fam.ntiles, per_tile)


class Case:
    def __init__(self, oracle):
        self.fam = D.Family(PLANTED, 4, 37)
        bases, off = self.fam.flat()
        self.tree = rx.Tree.new_flat(self.fam.lineages, bases, off, kmer_map=False)
        self.otree = oracle.tree_new_flat(self.fam.lineages, bases, off)
        assert np.array_equal(self.otree.original_index(), np.arange(self.fam.n_refs))
        self.qs = queries()
        self.bases, self.off = D.concat([D.query(a, t) for a, t in self.qs])
        # the reference, computed once: the closed form (held against the oracle's counts), the oracle's probabilities and rows
        self.want = [self.fam.expected_counts(a, t) for a, t in self.qs]
        t_o, c_o = self.otree.hit_counts_batch(self.bases, self.off, threads=8)
        assert all(int(t_o[j]) == t and np.array_equal(c_o[j], self.want[j]) for j, (a, t) in enumerate(self.qs))
        self.tables, _, _ = oracle.prob_tables_batch(t_o, c_o, threads=8)
        _, rows, nrows = self.otree.classify_batch(self.bases, self.off, raw_confidence=True, threads=8, cap=64)
        self.rows = [self.otree.rows_of(rows, nrows, j, 64) for j in range(len(self.qs))]
        self.lf = np.array([oracle.lib.orc_ln_factorial(i) for i in range(2 * 400 + 8)], dtype=np.float64)
        for a, t in self.qs:      # every row dense in tiles 0, 1, 2 and the last, none in tile 3
            assert [self.fam.segments(a, t, tile) for tile in (0, 1, 2, 4)] == [(0, t)] * 4 and self.fam.segments(a, t, 3)[1] == 0

    def classify(self, **opts):
        index = rx.Index(self.tree, debug_taps=True, locator=False, **opts)
        res = index.classify(self.bases, self.off)
        classes = index.batch_classes()
        assert len(classes) == 1 and classes[0]["planes"] == 10 and classes[0]["pair"], classes
        assert index.last_sub_batch() == (0, len(self.qs))
        order = index.debug_order(len(self.qs)).astype(np.int64)
        lists = set()      # (t_a, t_b, shared rows) of the pairs the device formed
        for x, y in D.pairs_of(order):
            (a, ta), (b, tb) = self.qs[x], self.qs[y]
            lists.add((ta, tb, max(0, min(a + ta, b + tb) - max(a, b))))
        assert {(T, T, T - d) for d in SHIFTS} <= lists, sorted(lists)
        assert sum(max(ta, tb) < 24 for ta, tb, s in lists) >= 3 and sum(24 <= max(ta, tb) < 48 for ta, tb, s in lists) >= 3, sorted(lists)
        return index, res, classes

    def check_rows(self, oracle, res):
        for j, q in enumerate(self.qs):
            got = res.rows(j)
            # identical rows -- or the other of two sibling taxa that tie to 1e-9 in the oracle's own numbers (they hold copies of the same windows)
            assert_rows_equivalent(got, self.rows[j], self.tables[j][self.want[j]], self.fam.lineages, f"query {q}")


@pytest.fixture(scope="module")
def case(oracle):
    return Case(oracle)


def test_counts_of_every_tile(case, oracle):
    """Pruning off: every (pair, tile) block is counted -- two-dimensional grid, the dense lists of four tiles, the sparse slots of one."""
    index, res, classes = case.classify(tile_prune=False)
    assert not classes[0]["prune"]
    for j, (a, t) in enumerate(case.qs):
        got = index.debug_hit_counts(j)
        assert np.array_equal(got, case.want[j]), ((a, t), np.nonzero(got != case.want[j])[0][:8])
    case.check_rows(oracle, res)


@pytest.mark.parametrize("records", [8, 0])     # (every tile holds windows that cover the queries: five live tiles each)
def test_pruned_run_and_bounds(case, oracle, emul, records):
    """Pruning on: the one-level bounds pass (hit_count_pair_kernel<.., 1, ..>) leaves the closed-form bound of every tile, the counting pass
    over the list of live blocks leaves the closed-form counts of the tiles it visited (on the records path: those above the threshold)."""
    index, res, classes = case.classify(tile_prune=True, records=records)
    assert classes[0]["prune"] and classes[0]["records"] == (records > 0)
    seen = []
    for j, (a, t) in enumerate(case.qs):
        o = check_run_as_left(index, j, t, case.want[j], case.tables[j], index.n_refs, emul, case.lf, f"query {(a, t)}")
        seen.append(o)
        bb = block_bounds(case.fam, a, t)
        got = index.debug_tile_bounds(j)
        assert np.array_equal(got, bb.max(axis=1)), ((a, t), got, bb.max(axis=1))
        det = index.debug_prune_detail(j)
        assert det["largest_bound"] == int(bb.max()) and int(bb.reshape(-1)[det["block"]]) == int(bb.max()), ((a, t), det["block"], det["largest_bound"])
    print("as left (threshold, live tiles, records):", sorted({(o["threshold"], o["live"], o["records"]) for o in seen}))
    assert sum(o["threshold"] > 0 for o in seen) >= 2 * len(SHIFTS) and any(o["records"] for o in seen) == (records > 0)
    case.check_rows(oracle, res)


# ---- the two-level bounds pass -------------------------------------------------------------------------------------------------------------
A2 = 12050        # from here every pair below has the min-hashes of its first window (checked through debug_order)
SHARED2, SHIFTS2 = (255, 256, 257), (31, 32, 33, 127, 128, 129)
# 16 full tiles + 37: tiles 0 .. 3 (B-tile 0) hold the windows of D.PLANTED and the 23 of tile 1, tiles 4 .. 15 background alone; the partial
# last tile (B-tile 4) holds two windows that begin 100 rows into the queries, so that its level-A bound lies below the largest one
PLANTED2 = [p for p in PLANTED if not (p[0] == -1 and p[2] >= 11990)] + [(-1, 20, A2 + 100, 4000), (-1, 21, A2 + 101, 4000)]
# tile 5 (B-tile 1): two windows in different blocks of 64 of one block of 256 that hold 100 rows each of every query below -- 100 over blocks of 64, 200 over blocks of 256
PLANTED2 += [(5, 0, A2 + 130, 100), (5, 70, A2 + 255, 100)]


def _rule(ct, cm, lo, hi):      # RTX_OPT_TWO_LEVEL_BOUNDS > 1: dl = ct t - cm max within [lo t, hi t], all in 1/256 (tests/test_gpu_two_level.py)
    return ct | (cm << 16) | (lo << 32) | (hi << 48)


def queries2():
    qs = []
    for s in SHARED2:
        for d in SHIFTS2:
            qs += [(A2, s + d), (A2 + d, s + d)]
    qs += [(A2, 300), (A2 + 10, 280)]      # the second window inside the first: 280 shared rows, 20 of A alone, none of B alone
    qs += [(A2 + 5, 300)]                  # a last pair of one query
    return qs


@pytest.fixture(scope="module")
def case2():
    fam = D.Family(PLANTED2, 16, 37)
    bases, off = fam.flat()
    tree = rx.Tree.new_flat(fam.lineages, bases, off, kmer_map=False)
    qs = queries2()
    ref = []      # per query, computed once: counts, bounds over blocks of 64 and of 256
    for a, t in qs:
        ref.append((fam.expected_counts(a, t), block_bounds(fam, a, t, 64), block_bounds(fam, a, t, 256).max(axis=1)))
    return fam, tree, qs, ref


@pytest.mark.parametrize("rule", ["all", "least"])
def test_two_level_bounds(case2, rule):
    """bounds2_kernel on lists that end on either side of 32, 128 and 256 rows.  With the rule that refines every B-tile the bounds are the
    one-level closed form on every tile; with the rule that refines only the B-tiles that hold the largest level-A bound, every other tile
    carries the closed form over blocks of 256.  The best block is the lowest block of 64 with the largest bound among the refined tiles,
    its 64 exact counts are the closed form."""
    fam, tree, qs, ref = case2
    assert fam.ntiles == 17
    index = rx.Index(tree, debug_taps=True, locator=False, tile_prune=True, two_level=_rule(0, 0, 1024, 1024) if rule == "all" else _rule(2, 0, 0, 0))
    bases, off = D.concat([D.query(a, t) for a, t in qs])
    res = index.classify(bases, off)
    classes = index.batch_classes()
    assert len(classes) == 1 and classes[0]["planes"] == 10 and classes[0]["pair"] and classes[0]["prune"], classes
    assert index.last_sub_batch() == (0, len(qs)) and len(qs) % 2 == 1
    order = index.debug_order(len(qs)).astype(np.int64)
    lists = set()      # (rows of A, rows of B, shared rows) of the pairs the device formed
    for x, y in D.pairs_of(order):
        if y is None:
            lists.add((qs[x][1], 0, 0))
            continue
        (a, ta), (b, tb) = qs[x], qs[y]
        lists.add((ta, tb, max(0, min(a + ta, b + tb) - max(a, b))))
    assert {(s + d, s + d, s) for s in SHARED2 for d in SHIFTS2} | {(300, 280, 280), (300, 0, 0)} <= lists, sorted(lists)
    st = index.debug_prune_stats()
    assert st["bound_violations"] == 0, st
    n_unrefined = 0
    for j, (a, t) in enumerate(qs):
        want, bb64, a_max = ref[j]
        assert int(res.t[j]) == t
        want_ub = bb64.max(axis=1).copy()
        refined = np.ones(fam.ntiles, bool)
        if rule == "least":      # dl = 1: a B-tile (four tiles) is refined where its largest level-A bound is the query's largest
            for bt in range(0, fam.ntiles, 4):
                if a_max[bt:bt + 4].max() != a_max.max():
                    refined[bt:bt + 4] = False
                    want_ub[bt:bt + 4] = a_max[bt:bt + 4]
            n_unrefined += int((~refined & (a_max > 0)).sum())
        got = index.debug_tile_bounds(j)
        assert np.array_equal(got, want_ub), ((a, t), got, want_ub)
        det = index.debug_prune_detail(j)
        cand = np.where(np.repeat(refined, 128), bb64.reshape(-1), -1)
        best = int(np.argmax(cand))      # (the lowest block among equals)
        assert det["block"] == best and det["largest_bound"] == int(cand[best]) and det["t"] == t, ((a, t), det["block"], best, det["largest_bound"])
        blk = np.zeros(64, np.uint32)
        seg = want[best * 64:(best + 1) * 64]
        blk[:len(seg)] = seg
        assert np.array_equal(det["block_counts"], blk) and det["M"] == int(blk.max()), (a, t)
        got_counts = index.debug_hit_counts(j)
        assert np.array_equal(got_counts, want), ((a, t), np.nonzero(got_counts != want)[0][:8])
    if rule == "least":
        assert n_unrefined >= len(qs), n_unrefined      # the partial last tile of every query carries level A's bound

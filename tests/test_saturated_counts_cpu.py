"""The de Bruijn family of tests/debruijn_common.py on the CPU: the closed form of the hit counts against the oracle, and the
preconditions of tests/test_gpu_saturated_counts.py taken from the oracle's own results -- every count, split and sparse-segment number
the GPU cases are named after really occurs, no designed query has sibling taxa on an exact tie or a confidence on a rounding boundary
(so the GPU tests can demand identical rows, without an excuse ledger), the processing order forms the pairs the pair case needs, and
the pruning threshold of the query that runs the `smax > h_thr` branch of rec_epilogue lies below its sparse maximum."""
import numpy as np
import pytest

import debruijn_common as D
from raxtax_amd.checks import emul_threshold

SMALL = ("p8", "p10", "p10_long", "p11", "p12", "p16", "p16_global", "seg", "pairs", "p11_sample")


@pytest.fixture(scope="module")
def world(oracle):
    return D.World(oracle, 4, 37)


@pytest.fixture(scope="module")
def world13(oracle):
    return D.World(oracle, 13, 100)


def test_the_sequence_and_the_database_order(world):
    seq = D.de_bruijn_4_8()
    assert len(seq) == 65_543
    two = np.log2(seq).astype(np.int64)
    kmers = sum(two[j:len(seq) - 7 + j] << (2 * (7 - j)) for j in range(8))
    assert len(np.unique(kmers)) == 65_536                                           # every 8-mer exactly once
    fam = world.fam
    assert fam.n_refs == 4 * 8192 + 37 and fam.ntiles == 5
    assert len(set(fam.lineages)) >= 300 and max(l.count(",") for l in fam.lineages) + 1 <= 6
    assert np.array_equal(world.otree.original_index(), np.arange(fam.n_refs))        # the tree keeps the database order
    bg = np.setdiff1d(np.arange(fam.n_refs), fam.planted_ids)
    assert (fam.start[bg] >= D.BG0).all() and (fam.n_kmers[bg] <= 39).all()           # no query touches the background
    for qs in list(D.QUERIES.values()) + [D.pair_queries(), D.p11_bulk()]:
        assert all(a + t <= D.BG0 for a, t in qs)


@pytest.mark.parametrize("case", SMALL)
def test_oracle_equals_the_closed_form(world, case):
    r = world.case(case)
    oi = world.otree.original_index().astype(np.int64)
    assert r["bad"] == 0 and (r["rc"] == 0).all()
    for j, (a, t) in enumerate(r["qs"]):
        assert int(r["t"][j]) == t
        want = world.fam.expected_counts(a, t)
        assert np.array_equal(r["counts"][j], want[oi]), (case, a, t)
        assert len(r["rows"][j]) >= 1


def test_oracle_equals_the_closed_form_beyond_twelve_tiles(world13):
    r = world13.case("seg")
    oi = world13.otree.original_index().astype(np.int64)
    assert np.array_equal(oi, np.arange(world13.fam.n_refs)) and world13.fam.ntiles == 14
    for j, (a, t) in enumerate(r["qs"]):
        assert int(r["t"][j]) == t and np.array_equal(r["counts"][j], world13.fam.expected_counts(a, t)[oi])


def _node_sums(probs):
    """Confidence of every node of the lineage tree of debruijn_common.lineage_of, level by level (root excluded), with each node's parent."""
    x = np.arange(len(probs)) // D.PER_TAXON
    out = []
    for div, pdiv in ((128, None), (32, 128), (8, 32), (2, 8), (1, 2)):
        node = x // div
        s = np.bincount(node, weights=probs)
        ids = np.arange(len(s))
        parent = np.zeros(len(s), np.int64) if pdiv is None else ids * div // pdiv
        out.append((s, parent))
    return out


def check_no_tie_no_boundary(r, label):
    for j, (a, t) in enumerate(r["qs"]):
        probs = r["tables"][j][r["counts"][j]]
        assert abs(probs.sum() - 1.0) < 1e-9
        for s, parent in _node_sums(probs):
            h = s * 100.0
            near = np.abs(h - np.floor(h) - 0.5) < 1e-4                  # within 1e-6 of a hundredths rounding boundary
            assert not near.any(), (label, a, t, s[near])
            live = np.nonzero(s > 1e-6)[0]                               # (a node below that prints 0.00 and leads nowhere)
            for p in np.unique(parent[live]):
                c = np.sort(s[live[parent[live] == p]])
                assert (np.diff(c) > 1e-9).all(), (label, a, t, "sibling taxa on a tie", c)


@pytest.mark.parametrize("case", SMALL)
def test_no_sibling_ties_and_no_confidence_on_a_rounding_boundary(world, case):
    check_no_tie_no_boundary(world.case(case), case)


def test_no_ties_beyond_twelve_tiles(world13):
    check_no_tie_no_boundary(world13.case("seg"), "seg, 13 tiles + 100")


def _counts_seen(r):
    return set(np.unique(np.concatenate([c for c in r["counts"]])).tolist())


def test_every_class_reaches_its_target_counts(world):
    """t, t - 1, 2^k - 1 and 2^k (k = 8, 9, 10) -- as far as the class can hold them -- among the ORACLE's counts of the designed queries."""
    want = {"p8": {255, 254, 128, 8}, "p10": {1023, 1022, 512, 511, 256, 255}, "p10_long": {1024, 1023},
            "p11": {2047, 2046, 1024, 1023, 512, 511, 256, 255}, "p12": {4095, 4094, 2048, 2047, 1024, 1023, 512, 511, 256, 255},
            "p16": {4096, 4095}, "p16_global": {7893, 7892}}
    for case, targets in want.items():
        r = world.case(case)
        assert targets <= _counts_seen(r), (case, targets - _counts_seen(r))
        full = [j for j, (a, t) in enumerate(r["qs"]) if int(r["counts"][j].max()) == t]
        near = [j for j, (a, t) in enumerate(r["qs"]) if (r["counts"][j] == t - 1).any()]
        assert full and near, case                                           # a reference that contains the query, a neighbour at t - 1
    ts = {case: {t for a, t in D.QUERIES[case]} for case in D.QUERIES}
    assert {255, 254, 128, 8} <= ts["p8"] and max(ts["p8"]) == 255
    assert 1023 in ts["p10"] and min(ts["p10"]) >= 256 and max(ts["p10"]) == 1023
    assert 2047 in ts["p11"] and min(ts["p11"]) >= 1024
    assert {1024, 2047, 2048, 4095} <= ts["p12"] and max(ts["p12"]) == 4095 and ts["p16"] == {4096}
    bulk = D.p11_bulk()
    assert len(bulk) >= 4096 and all(1024 <= t <= 2047 for a, t in bulk)
    # eight references of one group all at 1023 (packed high bits all 3, low bytes all 0xFF) beside a group of all 0
    c = world.case("p10")["counts"][D.QUERIES["p10"].index((7000, 1023))]
    g = 8192 + 400
    assert (c[g:g + 16] == 1023).all() and (c[g - 8:g] == 0).all() and g % 8 == 0
    # the byte neighbours of the saturated references of the eight-plane case hold counts >= 1
    for q, ref in (((1000, 255), 97), ((2000, 255), 8192 + 201), ((3000, 255), 2 * 8192 + 241)):
        c = world.case("p8")["counts"][D.QUERIES["p8"].index(q)]
        g = ref // 8 * 8
        assert c[ref] == 255 and (c[g:g + 8] >= 1).all(), q


def test_the_dense_and_sparse_splits_occur(world):
    fam = world.fam
    want = {(128, 127): ("p8", (3000, 255), 2 * 8192 + 241), (0, 255): ("p8", (1000, 255), 97), (255, 0): ("p8", (2000, 255), 8192 + 200),
            (768, 255): ("p10", (5000, 1023), 321), (1023, 0): ("p10", (7000, 1023), 8192 + 400), (1792, 255): ("p11", (12000, 2047), 1201)}
    for split, (case, q, ref) in want.items():
        assert q in D.QUERIES[case]
        assert fam.split(q[0], q[1], ref) == split, (split, fam.split(q[0], q[1], ref))
        assert int(fam.expected_counts(*q)[ref]) == sum(split) == q[1]
        tile = ref // 8192
        assert fam.segments(q[0], q[1], tile)[0] <= 255 or split[1] == 0      # no cap in the way: the split is the one the kernel makes
    # the partial last tile has no sparse path
    assert fam.segments(4000, 255, 4) == (0, 255) and fam.split(4000, 255, 4 * 8192 + 5) == (255, 0)


@pytest.mark.parametrize("which", ["world", "world13"])
def test_every_sparse_segment_count_occurs(which, request):
    fam = request.getfixturevalue(which).fam
    seen = {}
    for a, t in D.QUERIES["seg"]:
        for tile in range(fam.ntiles):
            sp, de = fam.segments(a, t, tile)
            seen.setdefault(sp, []).append((a, tile, de))
    assert set(D.SPARSE_TARGETS) <= set(seen), set(D.SPARSE_TARGETS) - set(seen)
    # the class edge: the same rows with exactly 16 covering references in tile 1 (sparse) and exactly 17 in tile 2 (dense)
    c1, c2, c3 = fam.cover(1)[20000:20300], fam.cover(2)[20000:20300], fam.cover(3)[20000:20300]
    assert (c1 == 16).all() and (c2 == 17).all() and (c3 == 1).all()
    for a, t in D.QUERIES["seg"]:
        k = 20300 - a
        assert fam.segments(a, t, 1) == (k, 0) and fam.segments(a, t, 2) == (0, k) and fam.segments(a, t, 3) == (k, t - k)
    # ... and the cap with its dense remainder in the other cases: 512 and 2047 sparse rows of one (query, tile)
    assert fam.segments(7000, 1023, 2) == (512, 0) and fam.segments(12000, 2047, 1)[0] == 2047


def test_the_processing_order_forms_the_pairs(world):
    """Without the locator the order is a stable sort by the three min-hashes of a read (rtx_cluster.hip), restated in debruijn_common:
    the batch of the pair case is laid out so that it pairs an identical couple, a disjoint one, every designed shift, a read without a
    k-mer, and leaves the last read alone."""
    qs = D.pair_queries()
    order = D.expected_order([D.query(a, t) for a, t in qs])
    kinds = D.pair_kinds(qs, order)
    assert kinds["identical"] >= 1 and kinds["disjoint"] >= 1 and kinds["single"] == 1 and kinds["no_kmers_inside"] == 1
    assert set(D.PAIR_OFFSETS) | {D.PAIR_T} <= kinds["shifts"]
    assert kinds["odd_lists"] >= 5                       # shifts of 1, 23, 25, 63, 65: A-only and B-only lists that are no multiple of 8


def test_the_threshold_of_the_all_sparse_query_lies_below_its_sparse_maximum(world, emul, oracle):
    """rec_epilogue takes `smax > h_thr` when a reference sits in more sparse segments than the query's threshold: the eight-plane
    query whose best reference is reached through 255 sparse segments and nothing else, and its neighbour whose best count is t - 1."""
    fam = world.fam
    for a, t in ((1000, 255), (999, 255)):
        c = fam.expected_counts(a, t)
        ref = int(np.argmax(c))
        assert fam.split(a, t, ref) == (0, int(c[ref])) and int(c[ref]) >= 254
        lf = np.array([oracle.lib.orc_ln_factorial(i) for i in range(2 * t + 8)], dtype=np.float64)
        blk = c[ref // 64 * 64:ref // 64 * 64 + 64].astype(np.uint32)
        pad = fam.ntiles * 8192 - fam.n_refs
        tile_ub = np.concatenate([c, np.zeros(pad, np.uint16)]).reshape(fam.ntiles, 8192).max(axis=1)
        for ub in (None, tile_ub):
            u, i1 = emul_threshold(emul, lf, t, fam.n_refs, blk, tile_ub=ub)
            assert 0 < u < int(c[ref]), (a, t, u)

"""rtx_denovo_check on the device (rtx_denovo.hip) against the numpy restatement of the definition (tests/denovo_common.py) and against
rtx_denovo_check_host, exact in every field: the prefix mask at the byte, word and tile edges and in a short last tile, the skew edge, the
rounds of the greedy rule, the live mask at every edge of its 16-byte column and in a short last tile, a flag that is taken back, later
rounds over two tiles, the same worlds cut into slices (RTX_DEFAULT_CHIMERA_SLICE), the counts at the plane classes' edges, the entries of an
OTU object, a planted scenario, and the reference-based check (rx.Chimera) on an index built from the same parents."""
import numpy as np
import pytest

import chimera_common as cc
import denovo_common as dc
import raxtax_amd as rx
from raxtax_amd import _lib

pytestmark = pytest.mark.gpu
ONE_TILE = (1, 7, 8, 9, 511, 512, 513, 520)   # (520: all the parents, so that the bitmap holds the entry at lim = 513 too)
TWO_TILES = (8191, 8192, 8193, 8232)


def _both(seqs, weights, otus=False, rounds=True, **params):
    """The device's result, held against the restatement and the host function; returns (device result, restatement, its records)."""
    table = dc.table_of(rx, seqs, weights)
    o = rx.otu_cluster_host(table) if otus else None
    d = rx.denovo_check(table, o, **params)
    h = rx.denovo_check_host(table, o, **params)
    rs = dc.of_otus(table, o, **params)[0] if otus else dc.of_table(table, **params)
    want = dc.check_equal(d, rs, "device")
    assert dc.as_tuples(d.rec) == dc.as_tuples(h.rec) and np.array_equal(d.lim, h.lim) and np.array_equal(d.row, h.row) and np.array_equal(d.weight, h.weight)
    assert (d.n_checked, d.n_flagged) == (h.n_checked, h.n_flagged)
    if rounds:
        r, s, _ = rs.rounds()
        assert (d.rounds, d.scans) == (r, s)
    return d, rs, want


def test_prefix_mask_in_one_tile():
    """520 parents: a tile of five lanes.  lim at 1, around a byte of the mask (7, 8, 9), around a word of the 16-byte row (511, 512, 513),
    and at all 520, which also puts the entry at lim = 513 into the bitmap."""
    seqs, weights, where = dc.prefix_world(520, ONE_TILE)
    d, rs, want = _both(seqs, weights, segments=4, mindelta=8)
    for L, (e, winner) in where.items():
        assert int(d.lim[e]) == L and int(d.rec[e]["parent"]) == winner and 21 <= int(d.rec[e]["single"]) < 33, (L, d.rec[e])


def test_prefix_mask_across_two_tiles_and_a_short_last_tile():
    """8192 + 40 parents: the second tile spans one lane.  lim at 8191, 8192, 8193 and all of them; the tie of entry lim - 1 with a lower
    entry crosses the tiles at 8193."""
    seqs, weights, where = dc.prefix_world(8232, TWO_TILES, seed=8)
    d, rs, want = _both(seqs, weights, segments=4, mindelta=8)
    for L, (e, winner) in where.items():
        assert int(d.lim[e]) == L and int(d.rec[e]["parent"]) == winner and 21 <= int(d.rec[e]["single"]) < 33, (L, d.rec[e])


def test_skew_edge_max_parents_and_no_parent():
    rng = np.random.default_rng(2)
    T = dc.rand_seq(rng, 60)
    seqs = [T, np.concatenate([T[:50], dc.rand_seq(rng, 10)]), np.concatenate([dc.rand_seq(rng, 10), T[10:]]), dc.rand_seq(rng, 60)]
    d, rs, _ = _both(seqs, [10, 9, 5, 1], segments=4, mindelta=8)
    assert rs.lim == [0, 0, 1, 3] and [int(r["status"]) for r in d.rec] == [dc.NO_PARENT, dc.NO_PARENT, cc.OK, cc.OK]
    d, rs, _ = _both(seqs, [7, 7, 7, 7], segments=4, mindelta=8, abskew=1)
    assert rs.lim == [0, 1, 2, 3]
    d, rs, _ = _both(seqs, [100, 90, 5, 1], segments=4, mindelta=8, max_parents=1)
    assert rs.lim == [0, 0, 1, 1]
    d, rs, _ = _both(seqs, [100, 90, 5, 1], abskew=1000)                       # nobody has a parent: no bitmap, no scan
    assert rs.lim == [0, 0, 0, 0] and (d.n_checked, d.rounds, d.scans) == (0, 1, 4)
    empty = rx.denovo_check(dc.table_of(rx, [], []))
    assert empty.n_entries == 0 and (empty.rounds, empty.scans) == (0, 0)


def test_rounds_of_the_greedy_rule():
    seqs, weights = dc.rounds_world()
    d, rs, want = _both(seqs, weights)
    assert [int(r["flag"]) for r in d.rec] == [0, 0, 1, 1, 1]
    assert d.rounds == 4 and d.scans == 8 < d.rounds * d.n_entries             # C, then D, then E, then a round with nothing left to scan
    assert len(d.seconds) == 4 and all(t >= 0 for t in d.seconds) and d.seconds[1] > 0


@pytest.mark.parametrize("n_parents, flagged_at", ((520, dc.LIVE_520), (8232, dc.LIVE_8232)))
def test_live_mask_at_the_byte_word_lane_and_tile_edges(n_parents, flagged_at):
    """the flagged entries lie at bits 0 and 7 of the first and last byte of every word of a lane's 16 bytes, in the first and the last lane
    of a tile of five lanes, of a full tile, and of a last tile of one lane: each one's bit is cleared, and only that one"""
    seqs, weights, where = dc.live_world(n_parents, flagged_at)
    d, rs, want = _both(seqs, weights, segments=4, mindelta=8)
    assert [e for e in range(rs.n) if int(d.rec[e]["flag"])] == sorted(flagged_at) and d.rounds == 2
    for f, (e, lower) in where.items():
        assert int(d.lim[e]) == n_parents and int(d.rec[e]["parent"]) == lower and 21 <= int(d.rec[e]["single"]) < 33, (f, d.rec[e])


def test_a_flag_that_goes_back():
    """D is flagged in round 1 and not in round 2: its live bit is cleared and then set again, and E finds D"""
    seqs, weights, at = dc.flipback_world()
    d, rs, want = _both(seqs, weights)
    assert [int(r["flag"]) for r in d.rec] == [0, 0, 0, 1, 0, 0] and (d.rounds, d.scans) == (3, 9)
    assert int(d.rec[at["E"]]["parent"]) == at["D"]


def test_later_rounds_over_two_tiles():
    """rounds 2 and 3 begin in the middle of the list with two tiles to scan: the first entry of every tile is clipped by the round's, in
    the ten-plane and in the twelve-plane class"""
    seqs, weights, at = dc.two_tile_rounds_world()
    d, rs, want = _both(seqs, weights)
    assert [e for e in range(rs.n) if int(d.rec[e]["flag"])] == [at["C"], at["D"], at["E"]]
    assert (d.rounds, d.scans) == (4, 8240 + 60 + 8 + 0)
    assert int(d.rec[at["X"]]["parent"]) == at["X_head"] and int(d.rec[at["H"]]["parent"]) == at["H_head"]


def _capped(cap, seqs, weights, **kw):
    """_both under RTX_DEFAULT_CHIMERA_SLICE = cap, and the records, rounds and scans of the uncapped run beside it"""
    free, _, _ = _both(seqs, weights, **kw)
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, cap))
    try:
        d, rs, want = _both(seqs, weights, **kw)
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, 0))
    assert d.rec.tobytes() == free.rec.tobytes() and (d.rounds, d.scans) == (free.rounds, free.scans)
    assert np.array_equal(d.lim, free.lim) and (d.n_checked, d.n_flagged) == (free.n_checked, free.n_flagged)
    assert all(t >= 0 for t in d.seconds) and d.seconds[1] > 0
    return d, rs, want


def test_slices_with_a_round_that_begins_inside_one():
    """slices of two entries: rounds 2 and 3 begin at entries 3 and 4, the second entry of slice 1 and the first of slice 2"""
    d, rs, _ = _capped(2, *dc.rounds_world())
    assert (d.rounds, d.scans) == (4, 8) and [int(r["flag"]) for r in d.rec] == [0, 0, 1, 1, 1]


def test_slices_of_the_planted_scenario():
    reads, templates, chimeras = dc.planted_world()
    d, rs, _ = _capped(50, [s for s, _ in reads], [w for _, w in reads], otus=True)
    assert d.n_entries == 60 and d.n_flagged == len(chimeras) == 20      # a slice of 50 seeds and one of 10; the chimeras are the rarest


def test_slices_of_one_entry():
    seqs, weights, at = dc.flipback_world()
    d, rs, _ = _capped(1, seqs, weights)
    assert (d.rounds, d.scans) == (3, 9) and int(d.rec[at["E"]]["parent"]) == at["D"]


@pytest.mark.parametrize("S", (16, 32))
def test_counts_at_the_class_edges(S):
    seqs, weights = dc.counts_world()
    d, rs, want = _both(seqs, weights, segments=S)
    by_len = {len(s): r for s, r in zip(rs.seqs, d.rec)}
    assert by_len[4097]["status"] == cc.TOO_LONG and by_len[7]["status"] == cc.NO_KMER
    assert (by_len[4096]["single"], by_len[4096]["parent"]) == (4089, 0)
    assert (by_len[1031]["single"], by_len[1030]["single"]) == (1024, 1023)   # twelve planes, and ten planes at their last value


def test_otu_mode():
    rng = np.random.default_rng(4)
    X, Y, Z = (dc.rand_seq(rng, 80) for _ in range(3))
    chim = np.concatenate([X[:40], Y[40:]])
    seqs = [Y, X] + [dc.substitute_at(X, (i,)) for i in (5, 25, 45, 65, 75)] + [Z, chim]
    d, rs, want = _both(seqs, [20, 10, 3, 3, 3, 3, 3, 8, 2], otus=True, segments=4, mindelta=8)
    assert rs.weights == [25, 20, 8, 2] and [int(x) for x in d.otu] == [1, 0, 2, 3] and int(d.rec[3]["flag"]) == 1
    assert rx.denovo_records_text(d).splitlines()[4].split("\t")[0::13] == ["otu4", "Y"]
    assert rx.denovo_fasta(d) == "".join(rx.otu_fasta(d.otus).splitlines(keepends=True)[:6])


def test_planted_scenario():
    reads, templates, chimeras = dc.planted_world()
    d, rs, want = _both([s for s, _ in reads], [w for _, w in reads], otus=True)
    flag_of = {bytes(rs.seqs[e]): int(d.rec[e]["flag"]) for e in range(rs.n)}
    assert all(flag_of[bytes(c)] == 1 for c in chimeras) and not any(flag_of[bytes(t)] for t in templates)


def test_counts_are_those_of_the_reference_based_check():
    """200 parents of one weight and 100 rarer entries, so that every one of the 100 has exactly the 200 as its parents (none of which is
    flagged: they have no parents themselves): rx.Chimera on an index of the 200 must count the same.  The index numbers its references in
    its own order, so the counts are compared and not the parents."""
    rng = np.random.default_rng(12)
    parents = [dc.rand_seq(rng, 300) for _ in range(200)]
    queries = []
    for q in range(100):
        a, b = (int(x) for x in rng.choice(200, 2, replace=False))
        bp = int(rng.integers(60, 240))
        s = np.concatenate([parents[a][:bp], parents[b][bp:]]) if q % 2 else parents[a].copy()
        queries.append(dc.substitute_at(cc.substitute(rng, s, 0.02), (q,)))   # (one certain difference: a query is no copy of a parent)
    table = dc.table_of(rx, parents + queries, [10] * 200 + [5] * 100)
    d = rx.denovo_check(table)
    assert [int(x) for x in d.lim] == [0] * 200 + [200] * 100 and d.rounds == 2
    seqs = table.seqs
    bases, off = cc.concat(seqs[:200])
    index = rx.Index(rx.Tree.new_flat([f"p:P,c:C,o:O,f:F,g:G,s:S{i}" for i in range(200)], bases, off))
    ref = rx.Chimera(index).run(*cc.concat(seqs[200:]))
    counts = ("status", "n_valid", "single", "seg", "pos", "left", "right", "delta", "flag")
    for f in counts:
        assert np.array_equal(d.rec[f][200:], ref[f]), f
    assert int(ref["flag"].sum()) >= 30

"""The read-out of a query's k-mer set (kmer_extract_kernel, rtx_kernels.hip): lane l owns the codes 1024 l .. 1024 l + 1023, one scan over the
wave places every lane's k-mers, they are staged in LDS (the first 4096 of a read) and go from there to the row translation and to `kmers`.
Held against the oracle's sequence_to_kmers (utils.rs:17-40): the sorted distinct k-mers and their number t, for every shape of read that
takes another way through the read-out; the row list behind it through bit-exact hit counts, on a pruned and on an unpruned handle."""
from __future__ import annotations

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth

import debruijn_common as dc

pytestmark = pytest.mark.gpu

N = 15      # the code of an ambiguous base


def _concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if int(off[-1]) else np.zeros(0, np.uint8)), off


def _random(rng, n, alphabet=4, p=None):
    return (1 << rng.choice(alphabet, n, p=p)).astype(np.uint8)


def _tapped(index, n):
    """The queries of the last run whose k-mers the taps can read: those of the last sub-batch."""
    first, cnt = index.last_sub_batch()
    return set(int(q) for q in index.debug_order(n)[first:first + cnt])


def _check_kmers(index, oracle, seqs, res, what, want_all=True):
    """t of every query and the k-mers of every query of the last sub-batch against the oracle; returns how many had their k-mers compared."""
    tapped = _tapped(index, len(seqs))
    for q, s in enumerate(seqs):
        want = oracle.sequence_to_kmers(s)
        assert int(res.t[q]) == len(want), f"{what}: t of query {q} ({len(s)} bases)"
        if q in tapped:
            got = index.debug_kmers(q)
            assert np.array_equal(got, want), f"{what}: k-mers of query {q} ({len(s)} bases)"
    if want_all:
        assert len(tapped) == len(seqs), f"{what}: {len(tapped)} of {len(seqs)} queries in the last sub-batch"
    return len(tapped)


@pytest.fixture(scope="module")
def small(oracle):
    """An unpruned handle: 1 500 references."""
    db = synth.make_db(1500, fanouts=(2, 2, 3, 3, 3, 2))
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    return db, rx.Index(tree), oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)


def _edge_reads(rng):
    """Reads that take the corners of the read-out: no window, the first and the last bit of the set, two codes, windows broken by N."""
    reads = [np.zeros(0, np.uint8)] + [_random(rng, n) for n in (7, 8, 9, 23)]
    reads += [np.full(300, 1, np.uint8), np.full(300, 8, np.uint8)]           # poly-A: code 0, the first bit; poly-T: code 65 535, the last
    reads += [np.tile(np.array([2, 4], np.uint8), 150)]                       # period two: two codes
    every8 = _random(rng, 400)
    every8[7::8] = N                                                          # an N in every window: no k-mer
    one = _random(rng, 400)
    one[200] = N
    ends = _random(rng, 400)
    ends[0] = ends[-1] = N
    return reads + [every8, one, ends]


@pytest.mark.parametrize("lo,hi", [(8, 238), (239, 469), (470, 700)])
def test_kmers_of_every_length_and_corner(small, oracle, lo, hi):
    """Random reads of every length from 8 to 700 (every number of windows per lane up to eleven, and reads with fewer windows than lanes),
    a third of the lengths per case, beside the corner reads: one length class, one sub-batch, every query's k-mers compared."""
    db, index, _ = small
    rng = np.random.default_rng(101 + lo)
    seqs = _edge_reads(rng) + [_random(rng, n) for n in range(lo, hi + 1)]
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    assert len(index.batch_classes()) == 1
    assert _check_kmers(index, oracle, seqs, res, f"lengths {lo} .. {hi}") == len(seqs)
    assert int(res.t[0]) == 0 and int(res.t[1]) == 0 and int(res.t[2]) == 1                  # 0, 7 and 8 bases
    assert list(index.debug_kmers(5)) == [0] and list(index.debug_kmers(6)) == [65535]       # poly-A, poly-T
    assert int(res.t[7]) == 2 and int(res.t[8]) == 0                                         # period two; an N in every window


def test_kmers_of_long_and_concentrated_reads(small, oracle):
    """More than sixteen windows per lane (1 100 and 1 500 bases: a handful of them rides with the longer reads, the class of t <= 2047
    proper is the next test's) and a read of 3 000 bases over A, C and G alone, A three times as frequent as C or G: its k-mers fall into
    the ranges of 27 lanes, and on the CPU the fullest lane (the codes that begin with AAA) holds 162 of its 1 574 k-mers -- 6.6 times the
    mean of 24.6 per lane (asserted below: at least four times)."""
    db, index, _ = small
    rng = np.random.default_rng(7)
    acg = _random(rng, 3000, 3, p=(0.6, 0.2, 0.2))
    k = oracle.sequence_to_kmers(acg).astype(np.int64)
    per_lane = np.bincount(k >> 10, minlength=64)
    print(f"ACG read: t = {len(k)}, fullest lane {per_lane.max()}, mean {len(k) / 64:.1f}, lanes with k-mers {(per_lane > 0).sum()}")
    assert per_lane.max() >= 4 * len(k) / 64
    seqs = [_random(rng, 1100), _random(rng, 1500), acg, _random(rng, 1100), _random(rng, 1500)]
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    assert len(index.batch_classes()) == 1
    assert _check_kmers(index, oracle, seqs, res, "long and concentrated reads") == len(seqs)
    assert int(res.t[1]) > 1024 + 64


def test_kmers_of_reads_with_every_8mer(small, oracle):
    """The De Bruijn reads: 65 543 bases hold every 8-mer once -- t = 65 536, reported as RTX_Q_ALL_KMERS (status 2), every lane full; one base
    less and t = 65 535, the largest t that is served: every k-mer but one, sixteen times the LDS staging."""
    db, index, _ = small
    every = dc.de_bruijn_4_8()
    seqs = [db.seq(3).copy(), every.copy(), every[:-1].copy()]
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    assert list(res.status) == [0, 2, 0] and int(res.t[1]) == 65_536 and int(res.t[2]) == 65_535
    tapped = _tapped(index, len(seqs))
    assert 2 in tapped
    want = oracle.sequence_to_kmers(seqs[2])
    assert len(want) == 65_535
    assert np.array_equal(index.debug_kmers(2), want)
    if 0 in tapped:
        assert np.array_equal(index.debug_kmers(0), oracle.sequence_to_kmers(seqs[0]))


def _rows_subset(db, rng):
    """Reads whose row lists differ in shape: barcodes and their variants, short cuts, corners, one long read."""
    qs = synth.make_queries(db, 40, seed=5)
    seqs = [qs.seq(i).copy() for i in range(qs.n)]
    seqs += [db.seq(int(i))[: int(n)].copy() for i, n in zip(rng.integers(0, db.n, 8), (8, 9, 23, 64, 71, 72, 300, 657))]
    seqs += _edge_reads(rng)
    return seqs


def test_row_lists_on_an_unpruned_handle(small, oracle):
    db, index, otree = small
    rng = np.random.default_rng(11)
    seqs = _rows_subset(db, rng)
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    assert not index.batch_classes()[0]["prune"]
    _check_kmers(index, oracle, seqs, res, "unpruned handle")
    for q in sorted(_tapped(index, len(seqs))):
        t, counts = otree.hit_counts(seqs[q])
        assert np.array_equal(index.debug_hit_counts(q), counts), f"hit counts of query {q} ({len(seqs[q])} bases)"


def test_row_lists_and_the_mid_class_on_a_pruned_handle(oracle):
    """A handle that prunes (five tiles): bit-exact hit counts of the same subset through the recounting taps, and 4 096 reads of 1 100 and
    1 500 bases, which form the class of t <= 2047 (eleven planes) with its own kstride.  That batch is knowingly larger than the few hundred
    queries the other cases keep to: fewer than 4 096 reads of that length form no class of their own and ride with the longer reads
    (kMinMidClass, rtx_api_batch.hip), as the handful in test_kmers_of_long_and_concentrated_reads does.  They are 64 distinct reads, 64
    copies of each; t of every query and the k-mers of EVERY query the taps can read (the last sub-batch) are compared."""
    db = synth.make_db(33_000)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    index = rx.Index(tree, tile_prune=True)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    rng = np.random.default_rng(13)
    seqs = _rows_subset(db, rng)
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    assert index.batch_classes()[0]["prune"]
    _check_kmers(index, oracle, seqs, res, "pruned handle")
    for q in sorted(_tapped(index, len(seqs)))[::3]:
        t, counts = otree.hit_counts(seqs[q])
        assert np.array_equal(index.debug_hit_counts(q), counts), f"hit counts of query {q} ({len(seqs[q])} bases)"
    # the class of t <= 2047: chimeras of references, so that the reads have hits and the pruned path has something to prune
    def chimera(n):
        parts = [db.seq(int(i)) for i in rng.integers(0, db.n, n // db.length + 1)]
        return np.concatenate(parts)[:n].copy()
    distinct = [chimera(1100 if i % 2 else 1500) for i in range(64)]
    seqs = [distinct[i % 64] for i in range(4096)]
    bases, off = _concat(seqs)
    res = index.classify(bases, off)
    classes = index.batch_classes()
    assert len(classes) == 1 and classes[0]["planes"] == 11, classes
    want = [oracle.sequence_to_kmers(s) for s in distinct]
    assert all(int(res.t[q]) == len(want[q % 64]) for q in range(4096))
    tapped = sorted(_tapped(index, len(seqs)))
    assert tapped
    for q in tapped:
        assert np.array_equal(index.debug_kmers(q), want[q % 64]), f"k-mers of query {q} ({len(seqs[q])} bases)"

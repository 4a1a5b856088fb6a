"""The OTUs of a run on the device (rtx_otu.hip): rx.otu_cluster against the brute force of otu_common.py and against rx.otu_cluster_host, field
by field (all but rounds and link_passes), with no tolerance.  The fixtures are those of test_otu_cpu.py, where the brute force itself is
checked.  The complete world, the block edges and the 65 537 rows are where the work splits: a second link pass under default parameters,
labels contended on every link, and a numbering over more than one block and more than 256 of them."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from otu_common import (BLOCK_EDGES, COMPLETE_MASK, MANY, MAX_LEN, WEIGHTINGS, assert_otus, block_case, brute_of, check_blocks, check_clusters,
                        check_complete, cluster_case, complete_case, edge_case, edge_rows, many_blocks_case, seq, table_of)
from tally_common import concat, random_seq

pytestmark = pytest.mark.gpu


def test_edges_against_the_brute_force_and_the_host():
    table, want, _ = edge_case()
    got = rx.otu_cluster(table)
    assert_otus(got, want)
    assert_otus(got, rx.otu_cluster_host(table))
    assert got.link_passes == 1 and got.long_rows == 3 and len(got.links) > 100
    assert all(t >= 0 for t in got.seconds) and got.seconds[1] > 0


def test_edges_under_forced_collisions():
    """a hash of two bits: every row lies in one chain and on four tags, so that every probe walks on to the byte compare"""
    table, want, _ = edge_case()
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, 3))
    try:
        got = rx.otu_cluster(table)
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, 0))
    assert_otus(got, want)
    assert_otus(rx.otu_cluster(table), want)           # (the mask is restored)


def test_a_link_buffer_that_is_too_small_is_grown():
    table, want, _ = edge_case()
    got = rx.otu_cluster(table, initial_links=1)
    assert got.link_passes == 2
    assert_otus(got, want)
    exact = rx.otu_cluster(table, initial_links=len(want["links"]))
    assert exact.link_passes == 1
    assert_otus(exact, want)


def test_small_link_cases():
    base = random_seq(np.random.default_rng(2), MAX_LEN + 1)
    table = table_of([base, np.delete(base, 100)], [2, 1])
    got = rx.otu_cluster(table)
    assert got.long_rows == 1 and len(got.links) == 0 and got.n_otus == 2 and got.rounds == 0
    assert_otus(got, brute_of(table))
    table = table_of([seq("ACGTACGT"), seq("ACNTACGT"), seq("ACRTACGT"), seq("ACGTNACGT"), seq("A"), seq("AC"), seq("C")], [7, 6, 5, 4, 3, 2, 1])
    got = rx.otu_cluster(table)
    assert got.links.tolist() == [[0, 1], [0, 2], [0, 3], [4, 5], [4, 6], [5, 6]]
    assert_otus(got, brute_of(table))
    empty = rx.otu_cluster(table_of([]))
    assert empty.n_rows == 0 and empty.n_otus == 0 and empty.links.shape == (0, 2)


def test_clusters():
    table, want, named = cluster_case()
    got = rx.otu_cluster(table)
    assert_otus(got, want)
    assert_otus(got, rx.otu_cluster_host(table))
    check_clusters(table, got, named)
    assert got.rounds > 8                              # the chain of 40 takes more than one read-back batch of label rounds


def test_two_runs_and_two_ways_to_the_table_agree():
    table, want, _ = cluster_case()
    a, b = rx.otu_cluster(table), rx.otu_cluster(table)
    assert_otus(a, b)
    assert a.rounds == b.rounds or a.rounds > 0        # (the rounds may depend on the scheduling, the result does not)
    seqs, weight, _ = edge_rows()
    t = rx.Tally()
    half = len(seqs) // 2
    t.add(*concat(seqs[:half]), None, weight[:half])
    t.add(*concat(seqs[half:]), None, weight[half:])
    from_device = t.read()
    from_host, want = edge_case()[:2]
    assert [bytes(s) for s in from_device.seqs] == [bytes(s) for s in from_host.seqs]
    assert_otus(rx.otu_cluster(from_device), want)
    assert rx.otu_fasta(rx.otu_cluster(from_device)) == rx.otu_fasta(rx.otu_cluster_host(from_host))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_complete_world(weighting):
    """5 120 rows in 20 blocks and 64 000 links: more than the 4 n the first pass has room for, so the buffer grows under default parameters"""
    table, want = complete_case(weighting)
    got = rx.otu_cluster(table)
    assert got.link_passes == 2
    assert_otus(got, want)
    assert_otus(got, rx.otu_cluster_host(table))
    check_complete(table, got, weighting)
    assert got.rounds >= 2


def test_complete_world_under_long_chains():
    """a hash of 256 slots and three tags: every probe walks a chain of about twenty rows, most of them to the byte compare"""
    table, want = complete_case("three")
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, COMPLETE_MASK))
    try:
        got = rx.otu_cluster(table)
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, 0))
    assert got.link_passes == 2
    assert_otus(got, want)
    check_complete(table, got, "three")


@pytest.mark.parametrize("last", ("seed", "variant"))
@pytest.mark.parametrize("n", BLOCK_EDGES)
def test_block_edges(n, last):
    table, want, planted = block_case(n, last)
    got = rx.otu_cluster(table)
    assert_otus(got, want)
    check_blocks(got, n, planted)


def test_more_than_256_blocks():
    """row 65 536 is alone in block 256: the scan of the block sums takes a second pass, and its carry is the number of the last seeds"""
    table, want = many_blocks_case()
    got = rx.otu_cluster(table)
    assert got.n_rows == MANY and got.link_passes == 1
    assert_otus(got, want)
    assert got.n_otus > MANY * 9 // 10 and got.seed[-1] > 65280       # nearly every row is a seed, one of them in the last full block or behind it

"""Fastidious grafting on the device (rtx_graft.hip): rx.otu_graft against the restatement of graft_common.py and against rx.otu_graft_host,
field by field (all but the filter's counters and the times), with no tolerance.  The fixtures are those of test_graft_cpu.py, where their
properties are proven from the restatement alone."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from graft_common import (NONE, assert_graft, block_world, check_edges, edge_world, many_world, parity_world, planted_world, rank_of, restate_of, rule_world,
                          small_edge_world)
from otu_common import COMPLETE_MASK, assert_otus, cluster_case

pytestmark = pytest.mark.gpu


def masked(mask, fn):
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, mask))
    try:
        return fn()
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_OTU_HASH_MASK, 0))


def passes(info):
    """the candidates fit the first buffer -- max(1024, 4 x light rows) -- or the test pass runs once more"""
    return 1 if info["candidates"] <= max(1024, 4 * info["light_rows"]) else 2


def test_edge_world_against_the_restatement_and_the_host():
    table, d1, want, marks = edge_world()
    before = rx.otu_cluster(table)
    assert_otus(before, d1)
    got = rx.otu_graft(before)
    assert_graft(got, want)
    assert_graft(got, rx.otu_graft_host(before))
    check_edges(table, got, marks)
    info = got.graft_info
    assert info["test_passes"] == passes(info) and info["variants"] > 38 * 9 and info["confirmed"] <= info["candidates"] and info["confirmed"] >= info["grafts"]
    assert 5 <= info["bloom_log2"] <= 40 and 2 ** info["bloom_log2"] >= 16 * info["variants"]
    assert all(t >= 0 for t in info["seconds"]) and info["seconds"][1] > 0
    again = rx.otu_graft(before)                     # two runs agree in every field, the filter's counters included
    assert_graft(again, got)
    assert {k: v for k, v in again.graft_info.items() if k != "seconds"} == {k: v for k, v in info.items() if k != "seconds"}


def test_the_filter_never_decides():
    table, d1, want = small_edge_world()
    before = rx.otu_cluster(table)
    default = rx.otu_graft(before)
    assert_graft(default, want)
    collide = masked(3, lambda: rx.otu_graft(before))                     # a hash of two bits: every probe ends in the byte compare
    everything = rx.otu_graft(before, bloom_log2=6)                       # 64 bits: every string is a candidate
    twice = rx.otu_graft(before, initial_candidates=1)
    large = rx.otu_graft(before, bloom_log2=24)
    for got in (collide, everything, twice, large):
        assert_graft(got, want)
        assert got.graft_info["confirmed"] <= got.graft_info["candidates"] and got.graft_info["variants"] == default.graft_info["variants"]
    assert twice.graft_info["test_passes"] == 2 and twice.graft_info["candidates"] == default.graft_info["candidates"]
    assert everything.graft_info["bloom_log2"] == 6 and everything.graft_info["candidates"] > 4 * default.graft_info["candidates"]
    assert large.graft_info["confirmed"] == everything.graft_info["confirmed"] == default.graft_info["confirmed"]   # (what the filter lets through wrongly dies in the verify)
    assert default.graft_info["test_passes"] == 1


def test_edge_world_with_a_candidate_buffer_that_is_too_small():
    table, d1, want, _ = edge_world()
    got = rx.otu_graft(rx.otu_cluster(table), initial_candidates=1)
    assert_graft(got, want)
    assert got.graft_info["test_passes"] == 2


def test_the_rule_and_the_boundary():
    table, d1, named = rule_world()
    before = rx.otu_cluster(table)
    for boundary in (2, 3, 10):
        got = rx.otu_graft(before, boundary=boundary)
        assert_graft(got, restate_of(table, d1, boundary))
        assert_graft(got, rx.otu_graft_host(before, boundary=boundary))
    got = rx.otu_graft(before)
    by_bytes = rank_of(table)
    k = got.otu[by_bytes[named["lone2"]]]
    assert by_bytes[named["lone2"]] < got.seed[k] and got.seed[k] in (by_bytes[named[f"three{i}"]] for i in range(3))   # the seed stays
    assert f">otu{k + 1};size=5;seed=uniq{got.seed[k] + 1}\n" in rx.otu_fasta(got)
    one = rx.otu_graft(before, boundary=1)           # nothing is light: the input's clustering
    assert_otus(one, before)
    assert len(one.grafts) == 0 and (one.parent == NONE).all() and one.graft_info["test_passes"] == 0


def test_broken_link_two_columns_and_denovo():
    table, d1, named = cluster_case()
    before = rx.otu_cluster(table)
    got, host = rx.otu_graft(before, boundary=210), rx.otu_graft_host(before, boundary=210)
    assert_graft(got, restate_of(table, d1, 210))
    assert_graft(got, host)
    assert got.columns == 2 and rx.otu_table_text(got, ["a", "b"]) == rx.otu_table_text(host, ["a", "b"])
    a, b = rx.denovo_check(table, got), rx.denovo_check_host(table, host)
    for f in ("row", "otu", "weight"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert rx.denovo_records_text(a) == rx.denovo_records_text(b) and len(a.row) == got.n_otus
    assert rx.denovo_fasta(a) == rx.denovo_fasta(b)


@pytest.mark.parametrize("mask", (0, COMPLETE_MASK))
def test_parity_world(mask):
    table, d1 = parity_world()
    before = rx.otu_cluster(table)
    got = masked(mask, lambda: rx.otu_graft(before))
    assert_graft(got, restate_of(table, d1))
    assert got.n_otus == 256 and len(got.grafts) == 768


@pytest.mark.parametrize("n", (255, 256, 257, 513))
@pytest.mark.parametrize("last", ("grafted", "kept"))
def test_block_edges(n, last):
    table, d1, planted = block_world(n, last)
    got = rx.otu_graft(rx.otu_cluster(table))
    assert_graft(got, restate_of(table, d1))
    assert (got.parent[n - 1] != NONE) == (last == "grafted") and got.n_otus == n - len(planted)


def test_more_than_65536_otus():
    table, d1, want = many_world()
    before = rx.otu_cluster(table)
    assert before.n_otus > 65536
    got = rx.otu_graft(before)
    assert_graft(got, want)
    assert got.graft_info["test_passes"] == passes(got.graft_info)


def test_planted_scenario():
    table, d1, two_edit = planted_world()
    got = rx.otu_graft(rx.otu_cluster(table))
    assert_graft(got, restate_of(table, d1))
    assert got.n_otus == 40

"""Denoising on the device (rtx_unoise.hip): rx.otu_unoise against the restatement of unoise_common.py and against rx.otu_unoise_host, field by
field (all but the device's counters and the times), with no tolerance.  The worlds are those of test_unoise_cpu.py, where the restatement
alone proves what each of them holds; the assertions on named rows here are made on the device's result."""
import numpy as np
import pytest

import raxtax_amd as rx
import unoise_common as uc
from raxtax_amd import _lib
from unoise_common import ABSORBED, LEFT, LONG, NONE, ZOTU

pytestmark = pytest.mark.gpu
WORLDS = {w[0]: w for w in uc.all_worlds()}


def sliced(cap, fn):
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_UNOISE_SLICE, cap))
    try:
        return fn()
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_UNOISE_SLICE, 0))


def device(key):
    _, table, params = WORLDS[key]
    return table, rx.otu_unoise(table, **params), uc.solved(key, table, **params)


@pytest.mark.parametrize("key", sorted(WORLDS))
def test_device_against_the_restatement_and_the_host(key):
    _, table, params = WORLDS[key]
    table, got, want = device(key)
    uc.assert_unoise(got, want)
    uc.assert_unoise(got, rx.otu_unoise_host(table, **params))
    u = got.unoise
    assert u["tiers"] == len(uc.tiers_of(table.sizes, u["alpha"])) - 1
    # every (row, live centroid below lim) is a pair; one is dropped by the length test or runs, and what reaches the last column ran
    live = np.flatnonzero(want["status"] == ZOTU)
    pairs = sum(int(np.searchsorted(live, want["lim"][e])) for e in range(len(table.seqs)) if want["status"][e] != LONG)
    assert u["pairs"] == pairs and u["pairs_length"] + u["pairs_finished"] <= pairs and u["pairs_finished"] >= u["n_absorbed"]
    assert all(t >= 0 for t in u["seconds"]) and (u["seconds"][1] > 0) == (pairs > 0) and (u["launches"] > 0) == (pairs > 0)


def test_skew_edge_and_shift():
    for alpha in (1, 2, 3):
        table, m, _ = uc.skew_world(alpha)
        _, got, _ = device(f"skew{alpha}")
        u = got.unoise
        for d in (1, 2, 3):
            assert u["status"][m[f"at{d}_read"]] == ABSORBED and u["parent"][m[f"at{d}_read"]] == m[f"at{d}"] and u["dist"][m[f"at{d}_read"]] == d
            assert u["status"][m[f"below{d}_read"]] == ZOTU and u["parent"][m[f"below{d}_read"]] == NONE
        if alpha <= 2:
            assert u["dist"][m["cap_read16"]] == 16 and u["parent"][m["cap_read16"]] == m["cap"] and u["status"][m["cap_read17"]] == ZOTU
    table, m, _ = uc.shift_world()
    _, got, _ = device("shift")
    assert got.unoise["dist"][m["read7"]] == 7 and got.unoise["status"][m["read8"]] == LEFT


def test_distances_at_and_behind_the_threshold():
    table, m, cases = uc.distance_world()
    _, got, _ = device("distance")
    u = got.unoise
    for name, k in cases:
        near, far = m[name + "_near"], m[name + "_far"]
        assert u["status"][near] == ABSORBED and u["parent"][near] == m[name] and u["dist"][near] == k, name
        assert u["status"][far] == LEFT and u["parent"][far] == NONE and u["dist"][far] == NONE, name
    # the reads whose lengths differ by more than their k never enter the distance: insertions and deletions only, at k + 1
    assert u["pairs_length"] >= 6


def test_lengths():
    table, m = uc.lengths_world()
    _, got, _ = device("lengths")
    for n in uc.LENGTHS:
        assert got.unoise["parent"][m[f"len{n}_sub"]] == m[f"len{n}"] and got.unoise["dist"][m[f"len{n}_sub"]] == 1, n
    table, m = uc.short_world()
    _, got, _ = device("short")
    assert got.unoise["dist"][m["short"]] == 7
    table, m = uc.long_world()
    _, got, _ = device("long")
    u = got.unoise
    assert u["parent"][m["max_read"]] == m["max"] and u["status"][m["long"]] == LONG == u["status"][m["long_too"]] and got.long_rows == 2
    assert u["status"][m["long_copy"]] == LEFT and got.members[got.otu[m["long"]]] == 1 and got.seed[got.otu[m["long"]]] == m["long"]


def test_ties_and_lane_edges():
    table, m = uc.ties_world()
    _, got, _ = device("ties")
    assert got.unoise["parent"][m["tie_read"]] == m["p1"] and got.unoise["parent"][m["near_read"]] == m["q2"] and got.unoise["dist"][m["near_read"]] == 1
    for n in (65, 128, 129):
        table, m, at = uc.lanes_world(n)
        _, got, _ = device(f"lanes{n}")
        for p in at:
            assert got.unoise["parent"][m[f"read{p}"]] == p and got.unoise["dist"][m[f"read{p}"]] == 1, (n, p)
        assert got.unoise["pairs"] == len(at) * n


def test_greedy_rule_small_rows_and_tiers():
    table, m, _ = uc.greedy_world()
    _, got, _ = device("greedy")
    assert got.unoise["status"][m["B"]] == ABSORBED and got.unoise["status"][m["C"]] == ZOTU and got.n_otus == 2
    table, m, _ = uc.small_world()
    _, got, _ = device("small")
    u = got.unoise
    assert u["status"][m["small_absorbed"]] == ABSORBED and u["status"][m["small_left"]] == LEFT == u["status"][m["small_parent"]] == u["status"][m["small_child"]]
    _, got, _ = device("small_minsize1")
    assert got.unoise["parent"][m["small_child"]] == m["small_parent"] and got.unoise["n_left"] == 0
    _, got, _ = device("tiers")
    assert got.unoise["tiers"] == 2 and got.unoise["status"].tolist() == [ZOTU, ZOTU, ABSORBED] and got.unoise["pairs"] == 1
    _, got, _ = device("one_tier")
    assert got.unoise["tiers"] == 1 and got.unoise["n_zotu"] == 20 and got.unoise["pairs"] == 0 and got.unoise["launches"] == 0
    _, got, _ = device("row_tiers")
    assert got.unoise["tiers"] == 8 and got.unoise["n_absorbed"] == 7 and got.unoise["launches"] == 7


@pytest.mark.parametrize("cap", (1, 3))
def test_slices_do_not_show(cap):
    for key in ("lanes65", "distance", "ties", "row_tiers"):
        table, whole, want = device(key)
        _, _, params = WORLDS[key]
        cut = sliced(cap, lambda: rx.otu_unoise(table, **params))
        uc.assert_unoise(cut, want)
        assert rx.unoise_text(cut) == rx.unoise_text(whole) and rx.otu_fasta(cut) == rx.otu_fasta(whole)
        for k in ("pairs", "pairs_length", "pairs_finished", "tiers"):
            assert cut.unoise[k] == whole.unoise[k], (key, k)
        assert cut.unoise["launches"] >= whole.unoise["launches"] and (key != "lanes65" or cut.unoise["launches"] > whole.unoise["launches"])
    again = rx.otu_unoise(table, **params)                  # the cap is gone
    assert again.unoise["launches"] == whole.unoise["launches"]


def test_planted_scenario():
    table, m, variants = uc.planted_world()
    _, got, _ = device("planted")
    assert got.n_otus == 40 and got.unoise["n_absorbed"] == 360
    for name, (centre, d) in variants.items():
        assert got.unoise["parent"][m[name]] == m[centre] and got.unoise["dist"][m[name]] == d, name
    table, m, variants = uc.big_planted_world()
    big = rx.otu_unoise(table)
    uc.assert_unoise(big, rx.otu_unoise_host(table))
    assert big.n_rows == 2000 and big.n_otus == 40 and all(big.unoise["parent"][m[v]] == m[c] for v, (c, d) in variants.items())
    assert rx.unoise_text(big) == rx.unoise_text(rx.otu_unoise_host(table))


def test_the_object_goes_downstream():
    from otutax_common import world

    table, m, _ = uc.planted_world()
    _, got, _ = device("planted")
    host = rx.otu_unoise_host(table)
    dn = rx.denovo_check(table, got)
    assert dn.n_entries == 40 and rx.denovo_records_text(dn) == rx.denovo_records_text(rx.denovo_check_host(table, host))
    n = got.n_rows
    lin = rx.Lineages(np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros((n, 4), np.uint8))
    tree = world().tree
    tax = rx.otu_taxonomy(tree, got, lin)
    assert tax.n_otus == 40 and np.array_equal(tax.sizes, got.sizes) and np.array_equal(tax.members, got.members)
    assert np.array_equal(tax.sizes, rx.otu_taxonomy_host(tree, host, lin).sizes)


def test_no_rows_no_device_and_a_byte_that_is_no_code():
    empty = rx.otu_unoise(uc.table_of_weights([np.array([1], np.uint8)], [9]))
    assert empty.n_otus == 1 and empty.unoise["status"].tolist() == [ZOTU] and empty.unoise["tiers"] == 1
    table = uc.tiers_world()[0]
    with pytest.raises(rx.RtxError) as e:
        rx.otu_unoise(table, device=1 << 20)
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE
    odd = uc.table_of_weights([np.array([1, 2, 16, 4], np.uint8), np.array([1, 2, 4], np.uint8)], [80, 9])
    with pytest.raises(rx.RtxError) as e:
        rx.otu_unoise(odd)
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert rx.otu_unoise_host(odd).n_otus == 1                # (the host compares bytes: the shorter row is one deletion away)

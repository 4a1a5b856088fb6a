"""rx.otu_graft_host (rtx_otu_graft_host) against the definition restated twice in graft_common.py, and the properties of every fixture that
test_gpu_graft.py runs on the device, proven from the restatement alone.  No GPU."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from graft_common import (NONE, assert_graft, block_world, check_edges, edge_world, many_world, near, pair_parents, parity_world, plain_force, planted_world, rank_of,
                          restate_of, rule_world, small_edge_world)
from otu_common import cluster_case, ranks


def host_d1(table):
    return rx.otu_cluster_host(table)


def test_edge_world_host_and_both_restatements():
    table, d1, want, marks = edge_world()
    got = rx.otu_graft_host(host_d1(table))
    assert_graft(got, want)
    check_edges(table, want, marks)
    check_edges(table, got, marks)
    # (b): pair by pair, for the rows over A, C, G, T -- the parents of (a) are those of the dynamic programme
    heavy = want["parent"] == NONE
    heavy &= (np.asarray(d1["sizes"]) >= 3)[d1["otu"].astype(np.int64)]
    plain = np.array([bool(np.isin(s, (1, 2, 4, 8)).all()) and len(s) <= 4096 for s in table.seqs])
    pairs = pair_parents(table.seqs, heavy)
    light_plain = plain & ~heavy
    assert light_plain.sum() > 200
    # a plain light row may have an ambiguous heavy row below its plain parent: only the rows whose parent of (a) is plain are compared
    ok = light_plain & ((want["parent"] == NONE) | plain[np.minimum(want["parent"], len(plain) - 1)])
    assert ok.sum() >= light_plain.sum() - 2 and np.array_equal(pairs[ok], want["parent"][ok])
    assert got.graft_info["variants"] == got.graft_info["candidates"] == got.graft_info["confirmed"] == got.graft_info["test_passes"] == 0


def test_near_is_levenshtein_two_on_short_rows():
    """all rows of 1 .. 4 codes: sharing a string of the balls is a distance of at most 2"""
    from graft_common import ball
    rng = np.random.default_rng(5)
    rows = [bytes(1 << ((k >> (2 * i)) & 3) for i in range(n)) for n in (1, 2, 3, 4) for k in range(4 ** n)]
    balls = {r: ball(r) for r in rows}
    for _ in range(4000):
        a, b = rows[rng.integers(len(rows))], rows[rng.integers(len(rows))]
        assert (not balls[a].isdisjoint(balls[b])) == near(a, b), (a, b)


def test_small_edge_world():
    table, d1, want = small_edge_world()
    assert_graft(rx.otu_graft_host(host_d1(table)), want)
    assert len(table.seqs) <= 40 and len(want["grafts"]) >= 12


def test_the_rule():
    table, d1, named = rule_world()
    by_bytes = rank_of(table)
    rank = {k: by_bytes[v] for k, v in named.items()}
    want = restate_of(table, d1)
    got = rx.otu_graft_host(host_d1(table))
    assert_graft(got, want)
    par, otu0, otu1 = want["parent"], d1["otu"], want["otu"]
    graft_of = {int(g[0]): g for g in want["grafts"]}
    # the lower parent wins
    assert otu0[rank["m1"]] == otu0[rank["m2"]] and {par[rank["m1"]], par[rank["m2"]]} == {rank["h1"], rank["h2"]} and rank["h1"] < rank["h2"]
    g = graft_of[otu0[rank["m1"]]]
    assert g[2] == rank["h1"] and g[1] == rank["m1"] and otu1[rank["m2"]] == otu1[rank["h1"]] != otu1[rank["h2"]]
    # equal parents: the lower child
    assert otu0[rank["m3"]] == otu0[rank["m4"]] and par[rank["m3"]] == par[rank["m4"]] == rank["h3"]
    assert graft_of[otu0[rank["m3"]]][1] == min(rank["m3"], rank["m4"])
    # a parent that is no seed
    assert par[rank["child5"]] == rank["member5"] != d1["seed"][otu0[rank["member5"]]] and otu1[rank["child5"]] == otu1[rank["s5"]]
    # the chain
    assert par[rank["middle6"]] == rank["h6"] and par[rank["outer6"]] == NONE and otu1[rank["outer6"]] != otu1[rank["h6"]] == otu1[rank["middle6"]]
    assert want["seed"][otu1[rank["outer6"]]] == rank["outer6"]
    # a grafted row that outranks its new seed: the seed stays
    k = otu1[rank["lone2"]]
    assert k == otu1[rank["three0"]] and rank["lone2"] < want["seed"][k] == d1["seed"][otu0[rank["three0"]]]
    assert got.seed[k] == want["seed"][k] and got.sizes[k] == 5 and got.members[k] == 4
    text = rx.otu_fasta(got).split("\n")
    assert text[2 * k] == f">otu{k + 1};size=5;seed=uniq{want['seed'][k] + 1}"
    assert text[2 * k + 1] == "".join("ACGT"[(1, 2, 4, 8).index(c)] for c in table.seqs[want["seed"][k]])
    assert np.array_equal(got.otu[got.seed], np.arange(got.n_otus))
    # grafts text
    lines = rx.otu_grafts_text(got).split("\n")
    assert lines[0] == "#light\tsize\tchild\tparent\theavy\tinto" and lines[-1] == "" and len(lines) == len(want["grafts"]) + 2
    g = want["grafts"][0]
    assert lines[1] == f"otu{g[0] + 1}\t{d1['sizes'][g[0]]}\tuniq{g[1] + 1}\tuniq{g[2] + 1}\totu{g[3] + 1}\totu{g[4] + 1}"
    assert rx.otu_map_text(got).split("\n")[rank["lone2"]] == f"uniq{rank['lone2'] + 1}\totu{k + 1}"


@pytest.mark.parametrize("boundary", (2, 3, 10))
def test_the_boundary(boundary):
    table, d1, named = rule_world()
    by_bytes = rank_of(table)
    rank = {k: by_bytes[v] for k, v in named.items()}
    want = restate_of(table, d1, boundary)
    got = rx.otu_graft_host(host_d1(table), boundary=boundary)
    assert_graft(got, want)
    for size in (1, 2, 3, 9, 10):
        heavy = size >= boundary
        assert (want["parent"][rank[f"beside{size}"]] == rank[f"size{size}"]) == heavy, size
    assert (want["parent"][rank["beside_pair"]] == rank["pair2"]) == (3 >= boundary)   # 2 + 1: the total decides


def test_boundary_one_returns_the_input():
    table, d1, _ = rule_world()
    before = host_d1(table)
    got = rx.otu_graft_host(before, boundary=1)
    for k in ("otu", "seed", "members", "sizes", "counts", "links"):
        assert np.array_equal(getattr(got, k), getattr(before, k)), k
    assert len(got.grafts) == 0 and (got.parent == NONE).all() and np.array_equal(got.old_to_new, np.arange(before.n_otus))


def test_broken_link_and_two_columns():
    """cluster_case at B = 210: valley9 (209), kept apart from valley10 by breaking, is grafted onto it; the counts are summed per column"""
    table, d1, named = cluster_case()
    by_bytes = ranks(table)
    rank = {k: by_bytes[v] for k, v in named.items()}
    want = restate_of(table, d1, 210)
    got = rx.otu_graft_host(host_d1(table), boundary=210)
    assert_graft(got, want)
    assert d1["otu"][rank["valley9"]] != d1["otu"][rank["valley10"]] and want["otu"][rank["valley9"]] == want["otu"][rank["valley10"]]
    assert want["parent"][rank["valley9"]] in (rank["valley10"], rank["valley2"])
    assert got.columns == 2 and (got.counts[:, 1] > 0).any() and np.array_equal(got.counts.sum(axis=1), got.sizes)
    sums = np.zeros((got.n_otus, 2), np.uint64)
    np.add.at(sums, got.otu.astype(np.int64), table.counts)
    assert np.array_equal(sums, got.counts)
    assert rx.otu_table_text(got, ["a", "b"]).count("\n") == got.n_otus + 1


def test_parity_world_and_the_vectorised_restatement():
    table, d1 = parity_world()
    assert len(d1["links"]) == 0 and len(d1["seed"]) == 1024
    want = restate_of(table, d1)
    fast = plain_force(table.seqs, table.sizes, table.counts, d1, 3)
    for k in ("otu", "seed", "parent", "old_to_new", "grafts", "sizes"):
        assert np.array_equal(fast[k], want[k]), k
    # every light row has at least two heavy near rows, in different OTUs
    heavy = np.flatnonzero(table.sizes >= 3)
    assert len(heavy) == 256
    seqs, otu = table.seqs, d1["otu"]
    for x in range(256, 1024, 16):
        assert len({int(otu[y]) for y in heavy if near(seqs[x], seqs[y])}) >= 2, x
    assert len(want["grafts"]) == 768 and len(want["seed"]) == 256
    assert_graft(rx.otu_graft_host(host_d1(table)), want)


@pytest.mark.parametrize("n", (255, 256, 257, 513))
@pytest.mark.parametrize("last", ("grafted", "kept"))
def test_block_edges(n, last):
    table, d1, planted = block_world(n, last)
    want = restate_of(table, d1)
    assert [(int(g[2]), int(g[1])) for g in want["grafts"]] == sorted(planted, key=lambda e: e[1])
    assert (want["parent"][n - 1] != NONE) == (last == "grafted") and want["seed"][-1] == (n - 1 if last == "kept" else n - 7)
    assert len(want["seed"]) == n - len(planted)
    assert_graft(rx.otu_graft_host(host_d1(table)), want)


def test_many_blocks():
    table, d1, want = many_world()
    assert len(d1["seed"]) > 65536 and 256 * 256 > len(want["seed"]) > 256 and len(want["grafts"]) > 1000
    assert_graft(rx.otu_graft_host(host_d1(table)), want)


def test_planted_scenario():
    table, d1, two_edit = planted_world()
    want = restate_of(table, d1)
    rank = rank_of(table)
    light_before = {int(d1["otu"][rank[b]]) for b in two_edit}
    light_before = {k for k in light_before if d1["sizes"][k] < 3}    # (one that shares a substitution with a one-edit variant is linked already)
    assert len(two_edit) > 100 and len(light_before) > 80
    assert light_before <= {int(g[0]) for g in want["grafts"]}        # every two-edit variant of a heavy centre is grafted
    assert len(want["seed"]) == 40
    assert_graft(rx.otu_graft_host(host_d1(table)), want)


def test_arguments():
    table, d1, _ = rule_world()
    otus = host_d1(table)
    other_table, _, _ = small_edge_world()
    for bad in (dict(flags=1), dict(bloom_log2=4), dict(bloom_log2=41)):
        with pytest.raises(rx.RtxError) as e:
            rx.otu_graft_host(otus, **bad)
        assert e.value.code == _lib.RTX_ERR_INVALID
    otus.table = other_table
    with pytest.raises(rx.RtxError) as e:
        rx.otu_graft_host(otus)
    assert e.value.code == _lib.RTX_ERR_INVALID
    otus.table = table
    with pytest.raises(rx.RtxError) as e:
        otus._read_graft()                                # no graft result
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert_graft(rx.otu_graft_host(otus, boundary=0), restate_of(table, d1, 3))
    if _lib.load().rtx_device_count() == 0:
        with pytest.raises(rx.RtxError) as e:
            rx.otu_graft(otus)
        assert e.value.code == _lib.RTX_ERR_NO_DEVICE


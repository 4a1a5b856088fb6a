"""The exact cases of walk_common.py on the CPU: every vector is dyadic and sums to 1, both trees keep the order given, the rational
restatement of lineage.rs:61-179 equals the oracle row for row -- and every case demonstrably exercises what its note says (checked on
the probabilities and the tree, never on the device).  The three wrong variants of the restatement (first maximum, half to even, an
unstable sort) must each disagree with the oracle on the case that is there to catch them."""
from fractions import Fraction

import numpy as np
import pytest

import raxtax_amd as rx
import walk_common as wc

CASES = wc.all_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def evaluated(oracle):
    """name -> (oracle rows, the restatement's rows, the restatement's tree), computed once."""
    out, trees = {}, {}
    for c in CASES:
        if c.tree not in trees:
            sb, so = wc.sequences(len(c.lineages))
            otree = oracle.tree_new_flat(c.lineages, sb, so)
            assert otree.lineages == c.lineages, c.name                          # the order given is the order the trees keep
            assert list(rx.Tree.new_flat(c.lineages, sb, so).lineages) == c.lineages, c.name
            trees[c.tree] = (otree, wc.build_tree(c.lineages))
        otree, root = trees[c.tree]
        out[c.name] = (otree.lineage_evaluate(c.probs), wc.evaluate_exact(c.lineages, c.probs, root=root), root)
    return out


def _node(root, path):
    for i in path:
        root = root.children[i]
    return root


def _mass(c, nd):
    return Fraction(int(c.units[nd.lo:nd.hi].sum()), wc.U)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_is_exact_and_matches_the_oracle(evaluated, name):
    c = BY_NAME[name]
    wc.assert_dyadic(c.probs, c.sequential_only)
    rows, exact, _ = evaluated[name]
    assert exact == wc.oracle_rows_exact(rows)
    assert 1 <= len(rows) <= wc.MAX_ROWS and max(len(r["conf"]) for r in rows) <= wc.MAX_DEPTH
    if "rows" in c.meta:
        assert len(rows) == c.meta["rows"]


def test_wide_cases_reach_past_the_first_chunk(evaluated):
    c = BY_NAME["wide_chunks"]
    rows, exact, root = evaluated[c.name]
    assert len(root.children) == 200 and [i for i, ch in enumerate(root.children) if wc.hundredths(_mass(c, ch))] == [63, 64, 127, 128, 199]
    assert [r[0] for r in exact] == [63, 64, 127, 128, 199]                      # five rows, in that order
    c = BY_NAME["wide_nested"]
    rows, exact, root = evaluated[c.name]
    for path, named in c.meta["nodes"]:
        nd = _node(root, path)
        assert len(nd.children) >= 130
        assert [i for i, ch in enumerate(nd.children) if wc.hundredths(_mass(c, ch))] == named
        assert max(named) >= 64
    outer = c.meta["nodes"][0][1]
    assert len({i // 64 for i in outer}) == 1 and min(outer) >= 64                # both in one chunk of the outer scan, beyond the first
    for path, named in c.meta["nodes"][1:]:
        assert {i // 64 for i in named} >= {1, 2}                                 # the second and the third chunk of the inner scans
    assert len(exact) == 6


@pytest.mark.parametrize("name", ["fallback_last_max", "fallback_all_equal", "fallback_max_0_64", "fallback_three_levels"])
def test_fallback_cases_tie_where_they_say(evaluated, name):
    c = BY_NAME[name]
    rows, exact, root = evaluated[name]
    start = _node(root, c.meta["chain"][0][0])
    assert wc.hundredths(_mass(c, start)) > 0 and start.type == wc.INNER
    assert all(_mass(c, ch) < Fraction(1, 128) and wc.hundredths(_mass(c, ch)) == 0 for ch in start.children)   # no child reaches 2^-7
    for path, maxima in c.meta["chain"]:
        nd = _node(root, path)
        assert len(nd.children) > 64
        vals = [_mass(c, ch) for ch in nd.children]
        assert [i for i, v in enumerate(vals) if v == max(vals)] == maxima and len(maxima) >= 2
    last = _node(root, c.meta["chain"][-1][0]).children[c.meta["chain"][-1][1][-1]]
    assert last.lo == c.meta["row"]
    hit = [r for r in wc.oracle_rows_exact(rows) if r[0] == c.meta["row"]]
    assert len(hit) == 1 and hit[0][1][-len(c.meta["chain"]):] == [1] * len(c.meta["chain"])   # the oracle's row is the last of the maxima
    if name == "fallback_last_max":
        assert hit[0][1] == [26, 1, 1]


def test_small_cases_give_the_stated_rows(evaluated):
    assert evaluated["fallback_not_at_taxon_0"][1] == [(4, [98]), (1, [2, 1])]
    assert [r[0] for r in evaluated["sort_depth_tie"][1]] == [1, 3, 0, 2]
    assert evaluated["stable_equal_rows"][1] == [(i, [1]) for i in range(128)]
    assert [r[1][0] for r in evaluated["round_half_away_3"][1]] == [63, 25, 13]
    assert [r[1][0] for r in evaluated["round_half_away_2"][1]] == [63, 38]
    seen = {k for r in evaluated["round_half_away_levels"][1] for k in r[1]}
    assert {13, 38} <= seen
    deep = evaluated["deepest"][1]
    assert all(len(r[1]) == wc.MAX_DEPTH for r in deep)
    assert [1] * wc.MAX_DEPTH in [r[1] for r in deep]                             # the fallback chain of 30 levels under two levels of 0.01
    vecs = [r[1] for r in deep]
    differ_at = {min(k for k in range(wc.MAX_DEPTH) if a[k] != b[k]) for a in vecs for b in vecs if a != b}
    assert {0, 16, 31} <= differ_at


def test_prefix_cases_put_boundaries_on_every_edge(evaluated):
    for n in wc.PREFIX_EDGE_N:
        c = BY_NAME[f"prefix_edges_{n}"]
        root = evaluated[c.name][2]
        bnd = set()

        def collect(nd):
            bnd.update((nd.lo, nd.hi))
            for ch in nd.children:
                collect(ch)

        collect(root)
        inside = {b for b in bnd if 0 < b < n}
        for step in (8, 512, 1024, 8192):
            if n > step:
                assert any(b % step == 0 for b in inside), (n, step)
        for i in (0, 7, 8, 511, 512, 1023, 1024, 8191, 8192, n - 1):
            if i < n:
                assert c.units[i] > 0, (n, i)
        if c.meta["fallback_family"]:                                             # a significant family none of whose genera is significant
            fam = next(f for k in root.children for o in k.children for f in o.children if f.lo == 1536)
            assert wc.hundredths(_mass(c, fam)) == 3 and all(wc.hundredths(_mass(c, g)) == 0 for g in fam.children)
            assert any(r[0] == 1599 and r[1][-2:] == [1, 1] for r in evaluated[c.name][1])   # the last of the tied genera, the last of its species
    assert len(set(BY_NAME["prefix_edges_8193_many_values"].units.tolist())) > 2048   # a table row beyond 16 KiB: read from global memory
    assert all(len(set(c.units.tolist())) <= 64 for c in CASES if not c.meta.get("many_values"))


def test_tile_cases_leave_the_stated_dead_runs(evaluated):
    for c in [x for x in CASES if x.name.startswith("tile_gaps")]:
        n, live = c.meta["n"], c.meta["live"]
        ntiles = (n + wc.TILE - 1) // wc.TILE
        has = [bool(c.units[t * wc.TILE:(t + 1) * wc.TILE].any()) for t in range(ntiles)]
        assert [t for t in range(ntiles) if has[t]] == list(live)
        runs = sum(1 for t in range(ntiles) if not has[t] and (t == 0 or has[t - 1]))
        assert runs == (8 if c.name == "tile_gaps_overflow" else 4), (c.name, runs)            # kMaxPrefixGaps = 6
    c = BY_NAME["tile_gaps_overflow"]
    rows = evaluated[c.name][1]
    assert len(rows) == 32
    tiles = {r[0] // wc.TILE for r in rows}
    assert {9, 11, 13, 16} <= tiles                                               # rows on both sides of the sixth dead run (tile 10), behind the eighth, in the last tile of 5
    assert not BY_NAME["tile_gaps_last_dead"].units[7 * wc.TILE:].any()


def test_wrong_variants_of_the_restatement_are_caught(evaluated):
    """Would a walk that kept the first maximum, rounded half to even or sorted unstably be noticed?  Each does disagree with the oracle."""
    for name, wrong in (("fallback_last_max", dict(first_max=True)), ("fallback_all_equal", dict(first_max=True)), ("fallback_three_levels", dict(first_max=True)),
                        ("round_half_away_3", dict(half_even=True)), ("round_half_away_2", dict(half_even=True)), ("round_half_away_levels", dict(half_even=True)),
                        ("stable_equal_rows", dict(unstable=True)), ("sort_depth_tie", dict(unstable=True))):
        c = BY_NAME[name]
        want = wc.oracle_rows_exact(evaluated[name][0])
        assert wc.evaluate_exact(c.lineages, c.probs) == want
        assert wc.evaluate_exact(c.lineages, c.probs, **wrong) != want, (name, wrong)


def test_fuzz_generator_is_exact_and_covers_ties_and_late_children(oracle):
    hits = {"fallback_tie": 0, "sig_child_ge64": 0}
    modes = set()
    for seed in range(wc.FUZZ_TREES):
        lineages = wc.fuzz_tree(seed)
        assert 1 <= len(lineages) <= wc.FUZZ_MAX_N and 1 <= max(l.count(",") for l in lineages) + 1 <= 8
        sb, so = wc.sequences(len(lineages))
        otree = oracle.tree_new_flat(lineages, sb, so)
        assert otree.lineages == lineages
        root = wc.build_tree(lineages)
        vectors = wc.fuzz_vectors(seed, lineages, root)
        assert len(vectors) == wc.FUZZ_VECTORS
        for units, mode in vectors:
            probs = units.astype(np.float64) * 2.0 ** -40
            assert (units >= 0).all() and int(units.sum()) == wc.U               # (assert_dyadic on integers: the same statement)
            wc.assert_dyadic(probs[units != 0])
            st = {"fallback_tie": 0, "sig_child_ge64": 0}
            exact = wc.evaluate_exact(lineages, probs, stats=st, root=root)
            assert len(exact) <= wc.MAX_ROWS
            assert exact == wc.oracle_rows_exact(otree.lineage_evaluate(probs))
            modes.add(mode)
            for k in hits:
                hits[k] += st[k] > 0
    assert hits["fallback_tie"] >= 20 and hits["sig_child_ge64"] >= 20, hits
    assert modes == {0, 1, 2}

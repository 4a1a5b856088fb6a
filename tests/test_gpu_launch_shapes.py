"""The launches between the heavy kernels of a pruned sub-batch (rtx_hit_pair.hip, rtx_kernels.hip, rtx_prune.hip): the lists that only
schedule work -- the items of the fine bounds pass, the live (pair, tile) blocks of the counting pass, the rows of the counts buffer that
taxon_prefix_kernel is launched over -- are built and walked in shapes that must never show in a result:
  * a fine list several times longer than the grid of its pass (walked through the queues of the XCDs);
  * the counting list put together by several workgroups, each reserving its stretch with one atomic (three groups of pairs, the last one
    partial, the last pair without a second query): whatever order the groups arrive in;
  * a sub-batch in which some queries take the records path and some the dense path, with the counts buffer on its diet (taxon_prefix_kernel
    comes up per ROW, the workgroups behind the rows handed out leave) and off it (per query), over several sub-batches and both scratch
    sets (the counters of a set are zeroed by the kmer_extract of the sub-batch that takes the set over, not by fill launches)."""
from types import SimpleNamespace

import numpy as np
import pytest

import raxtax_amd as rx
from gpu_common import Excuses, check_properties, oracle_sample_parity
from raxtax_amd import synth
from raxtax_amd._lib import ptr, u64p

pytestmark = pytest.mark.gpu

FIELDS = ("row_off", "row_lineage", "row_conf", "row_local_signal", "global_signal", "t", "status")
FINE_GRID_CAP = 4096  # RTX_FINE_GRID_CAP (rtx_hit_pair.hip: launch_fine_bounds)


def same_arrays(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


def raw_prune_stats(index):
    out = np.zeros(16, dtype=np.uint64)
    rx._lib.check(index._lib.rtx_debug_prune_stats(index._h, ptr(out, u64p)))
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def db140k(oracle):
    """140 000 references = 18 tiles (the fine bounds pass runs from 16 on), three tiles of the fine union bitmap."""
    db = synth.make_db(140_000)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    return db, tree, otree


def test_fine_list_longer_than_its_grid(oracle, emul, db140k):
    """10 000 reads 10 % from their source: nearly every pair qualifies for the fine pass, with an item in most of the three fine tiles -- 13 579
    items for a grid of 4096 workgroups, so most items are taken from the queues.  Same result arrays as the same handle gives with the
    first stage of the bounds alone (RTX_OPT_FINE_BOUNDS = 0), and a sample against the oracle."""
    db, tree, otree = db140k
    n_q = 10_000
    qs = synth.make_queries(db, n_q, seed=71, mu_q=0.10, exact_frac=0.0)
    index = rx.Index(tree, debug_taps=True)
    ex = index.exact_matches(qs.bases, qs.base_off)
    res = index.classify(qs.bases, qs.base_off, *ex)
    check_properties(res, db, n_q)
    st = index.debug_prune_stats()
    print("both stages:", st)
    f_ntiles = (((db.n + 8191) // 8192) + 7) // 8
    grid = min(st["pairs"] * f_ntiles, FINE_GRID_CAP)
    items = st["fine_blocks_per_pair"] * st["pairs"]
    print(f"fine pass: {items:.0f} items for a grid of {grid} workgroups")
    assert st["pairs"] == (n_q + 1) // 2 and st["bound_violations"] == 0
    assert items > grid, "the fine list fits its grid: the queues of the XCDs are not walked"
    rx._lib.check(index._lib.rtx_index_set_option(index._h, 17, 0))
    res0 = index.classify(qs.bases, qs.base_off, *ex)
    st0 = index.debug_prune_stats()
    print("first stage only:", st0)
    assert st0["fine_blocks_per_pair"] == 0 and st0["bound_violations"] == 0
    assert st["live_tiles_per_pair_first_stage"] == st0["live_tiles_per_pair"] and st["live_tiles_per_pair"] < st0["live_tiles_per_pair"]
    same_arrays(res, res0, "fine pass on / off")       # a tile taken off the list held nothing above the threshold
    rx._lib.check(index._lib.rtx_index_set_option(index._h, 17, 1))
    sample = np.sort(np.random.default_rng(72).choice(n_q, 100, replace=False))
    exc = Excuses("launch_shapes/fine_list")
    oracle_sample_parity(index, oracle, otree, db, qs, sample, False, exc, full_res=res, chunk=100, emul=emul)
    exc.check()


@pytest.mark.parametrize("n_refs", [20_000, 40_000])
def test_counting_list_built_across_groups(oracle, emul, n_refs):
    """n_q = 4099: 2050 pairs = three groups of 1024 pairs for live_items_kernel (1024, 1024, 2), the last pair a single query.

    20 000 references are three tiles, and the library prunes from four tiles on (RTX_PRUNE_MIN_TILES): there the run has no list at all
    (asserted: no pairs in the statistics) and only the checks of the results apply.  40 000 references (five tiles) is the smallest round
    size at which the list exists; there every assertion on the statistics is made."""
    n_q = 4099
    db = synth.make_db(n_refs)
    qs = synth.make_queries(db, n_q, seed=73)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    index = rx.Index(tree, tile_prune=True, debug_taps=True)
    ex = index.exact_matches(qs.bases, qs.base_off)
    res = index.classify(qs.bases, qs.base_off, *ex)
    check_properties(res, db, n_q)
    st, raw = index.debug_prune_stats(), raw_prune_stats(index)
    print(st)
    assert st["bound_violations"] == 0
    if (n_refs + 8191) // 8192 < 4:
        assert st["pairs"] == 0
    else:
        assert st["pairs"] == (n_q + 1) // 2
        # the blocks the counting pass was handed (live_items_kernel: the group totals, slot 2 of the fine statistics) are the live tiles
        # the statistics report, and -- no fine pass below 16 tiles -- what prune_kernel counted pair by pair
        assert raw[12] > 0 and raw[12] == round(st["live_tiles_per_pair"] * st["pairs"]) and raw[12] == raw[0]
    again = index.classify(qs.bases, qs.base_off, *ex)
    same_arrays(res, again, "the same batch twice")    # the order in which the groups reserve their stretches is nobody's business
    sample = np.sort(np.random.default_rng(74).choice(n_q, 150, replace=False))
    sample[-1] = n_q - 1                                 # (the query without a partner)
    exc = Excuses(f"launch_shapes/groups/{n_refs}")
    oracle_sample_parity(index, oracle, otree, db, qs, np.unique(sample), False, exc, full_res=res, chunk=75, emul=emul)
    exc.check()


def test_records_and_dense_queries_in_one_sub_batch(oracle, emul, db140k):
    """Reads 2 % from their source keep a tile or two and take the records path; reads 15 % from it keep most tiles and take the dense
    epilogues, a row of the counts buffer each, and taxon_prefix_kernel.  Sub-batches of 4096 queries: four of them per batch, two scratch
    sets taken over in turn, 1024 rows to start with.
      A: one read in sixteen is far: the rows suffice, the diet stays on -- taxon_prefix_kernel is launched over the rows;
      B: every other read is far (the batch the diet cannot hold: the rows run out, the download doubles them and repeats the run until
         every query has a row of its own -- the launch per query).
    The samples (100 near and 100 far reads of B, 40 of each of A) are classified as batches of their own as well: a sub-batch too small
    for the diet, the launch per query with the records path on."""
    db, tree, otree = db140k
    L = db.length
    sub = 4096
    index = rx.Index(tree, sub_batch=sub, debug_taps=True)
    npad = ((db.n + 8191) // 8192) * 8192
    for what, n_near, n_far, n_s in (("A", 15_360, 1024, 40), ("B", 8192, 8192, 100)):
        near = synth.make_queries(db, n_near, seed=75, mu_q=0.02)
        far = synth.make_queries(db, n_far, seed=76, mu_q=0.15, exact_frac=0.0)
        n_q = n_near + n_far
        # interleaved, so that every sub-batch holds both kinds whatever the processing order makes of them
        B = np.concatenate([near.bases.reshape(-1, L), far.bases.reshape(-1, L)])
        perm = np.random.default_rng(77).permutation(n_q)
        is_far = (perm >= n_near)
        bases = np.ascontiguousarray(B[perm]).reshape(-1)
        off = (np.arange(n_q + 1) * L).astype(np.uint64)
        qs = SimpleNamespace(bases=bases, base_off=off)
        ex = index.exact_matches(bases, off)
        res = index.classify(bases, off, *ex)
        check_properties(res, db, n_q)
        st, parts = index.debug_prune_stats(), index.workspace_parts()
        rows = parts["counts"] / parts["scratch_sets"] / (npad * 1.25)
        print(f"{what}: {st['record_queries']} of {n_q} queries on the records path; {rows:.0f} rows of counts per set of {sub} queries", st)
        assert st["bound_violations"] == 0 and st["pairs"] == n_q // 2
        assert 0 < st["record_queries"] < n_q, "records path and dense path: both must have been taken"
        if what == "A":
            assert rows < sub, "the counts buffer is off its diet: taxon_prefix_kernel was launched per query"
        rng = np.random.default_rng(78)
        for kind, sel in (("near", np.flatnonzero(~is_far)), ("far", np.flatnonzero(is_far))):
            sample = np.sort(rng.choice(sel, n_s, replace=False))
            exc = Excuses(f"launch_shapes/mixed/{what}/{kind}")
            oracle_sample_parity(index, oracle, otree, db, qs, sample, False, exc, full_res=res, chunk=100, emul=emul)
            exc.check()
        again = index.classify(bases, off, *ex)
        same_arrays(res, again, f"{what} twice")

"""The lineage evaluation of the device on exact inputs (walk_common.py), through the path a run takes.

Every probability is a multiple of 2^-40 and every vector sums to 1, so every partial sum is exact in any order: the rows of the device
must equal the oracle's in number, order, lineage and hundredths, ties included -- no excuse applies.  Each case runs through the three
modes of rtx_debug_evaluate_mode: the walk as a kernel of its own (0), fused into taxon_prefix as on every whole-database handle (1), and
with tile maxima as well, so that tiles without a probability are skipped and their boundaries reach the walk as gaps (2)."""
import numpy as np
import pytest

import raxtax_amd as rx
import walk_common as wc
from raxtax_amd import synth

pytestmark = pytest.mark.gpu

CASES = wc.all_cases()
BY_NAME = {c.name: c for c in CASES}
PROBE = np.full(13, 1, np.uint8), np.array([0, 13], np.uint64)       # a read that shares its one k-mer with every reference of the case trees


class World:
    """One index (and one oracle tree) per distinct tree; the latest is kept, the cases of a tree follow one another."""

    def __init__(self, oracle):
        self.oracle, self.key, self.cur = oracle, None, None

    def get(self, key, lineages):
        if key != self.key:
            self.cur = None                                              # (the handle of the tree before goes first)
            sb, so = wc.sequences(len(lineages))
            otree = self.oracle.tree_new_flat(lineages, sb, so)
            tree = rx.Tree.new_flat(lineages, sb, so)
            assert otree.lineages == lineages and list(tree.lineages) == lineages
            index = rx.Index(tree)
            self.key, self.cur = key, (index, otree, _rows(index.classify(*PROBE)))
        return self.cur


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def _rows(res):
    return (res.status.copy(), res.row_off.copy(), res.row_lineage.copy(), res.row_conf.copy(), res.row_local_signal.copy(), res.global_signal.copy())


def _evaluate(index, before, probs, mode):
    """The tap, and behind it the handle classifies as it did before (the tap drops the uploaded batch and sizes the workspace for itself)."""
    res = index.debug_evaluate(probs, mode=mode)
    in_lds = index.last_evaluate_table_in_lds
    after = _rows(index.classify(*PROBE))
    assert int(after[0][0]) == 0 and int(after[1][1]) >= 1
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    return res, in_lds


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_exact_case_in_every_mode(world, name):
    c = BY_NAME[name]
    index, otree, before = world.get(c.tree, c.lineages)
    want = otree.lineage_evaluate(c.probs)
    got = {}
    for mode in c.modes:
        res, _ = _evaluate(index, before, c.probs, mode)
        wc.compare(res, want, f"{name} mode {mode}")
        got[mode] = _rows(res)
    assert all(np.array_equal(a, b) for a, b in zip(got[1], got[2]))     # skipping tiles drops exactly nothing: every non-zero entry is 2^-40 or more
    assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))


def test_both_table_variants_of_the_prefix_kernel_ran(world):
    """A vector of few distinct values has its table in LDS (the variant barcode-length classes run), one of thousands reads it from
    global memory: the tap reports which the launch took."""
    few, many = BY_NAME["prefix_edges_8193"], BY_NAME["prefix_edges_8193_many_values"]
    index, otree, before = world.get(few.tree, few.lineages)
    for c, lds in ((few, True), (many, False)):
        want = otree.lineage_evaluate(c.probs)
        for mode in (1, 2):
            res, in_lds = _evaluate(index, before, c.probs, mode)
            assert in_lds == lds, (c.name, mode)
            wc.compare(res, want, f"{c.name} mode {mode}")
    res, in_lds = _evaluate(index, before, few.probs, 0)
    assert not in_lds                                                    # mode 0 is the tap as it always was: the table in global memory


@pytest.mark.parametrize("seed", range(wc.FUZZ_TREES))
def test_fuzzed_trees_and_vectors(world, seed):
    lineages = wc.fuzz_tree(seed)
    index, otree, before = world.get(f"fuzz_{seed}", lineages)
    for k, (units, mode) in enumerate(wc.fuzz_vectors(seed, lineages)):
        probs = units.astype(np.float64) * 2.0 ** -40
        res, _ = _evaluate(index, before, probs, mode)
        wc.compare(res, otree.lineage_evaluate(probs), f"fuzz tree {seed} vector {k} mode {mode}")


def test_a_handle_the_tap_used_classifies_real_reads(oracle):
    """The tap resets the state of the uploaded batch: a real run behind it must be the run of a fresh handle (checked as smoke() checks)."""
    db = synth.make_db(1500, fanouts=(2, 2, 3, 3, 3, 2))
    qs = synth.make_queries(db, 64, exact_frac=0.2)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    index = rx.Index(tree, device=0)
    units = np.zeros(db.n, np.int64)
    units[[0, 7, 8, 511, 512, 1023, 1024, db.n - 1]] = wc.U >> 3
    probs = units.astype(np.float64) * 2.0 ** -40
    for mode in (2, 0, 1):
        wc.compare(index.debug_evaluate(probs, mode=mode), otree.lineage_evaluate(probs), f"mode {mode}")
    res = index.classify(qs.bases, qs.base_off)
    for q in range(qs.n):
        rows, _ = otree.classify(qs.seq(q), raw_confidence=True)
        got = res.rows(q)
        assert [r.lineage for r in got] == [r["idx"] for r in rows], q
        for g, r in zip(got, rows):
            assert g.confidence_values == r["conf"], q
            assert abs(g.local_signal - r["local_signal"]) < 1e-9 and abs(g.global_signal - r["global_signal"]) < 1e-9

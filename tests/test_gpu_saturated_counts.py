"""Hit counts at saturated bit planes and class edges, on inputs whose every count has a closed form (tests/debruijn_common.py: windows of
the de Bruijn sequence B(4, 8); tests/test_saturated_counts_cpu.py holds the closed form against the oracle and checks what these
tests presuppose -- no tie between sibling taxa, no confidence on a rounding boundary -- so identical rows are demanded here, without an
excuse).  Every case classifies, asserts through batch_classes() that the class it is about ran, then compares: t = len - 7; the run as
it was left (visited counts bit-exact, no unvisited tile above the threshold, histogram, probabilities); the full recount against the
closed form and the oracle, bit for bit; the probability table at the bins that are present, bin t among them, within 1e-9; the rows.

  1. eight planes: counts of 255 reached as 0 + 255 sparse, 255 dense + 0 and 128 + 127, beside byte neighbours that hold counts;
  2. ten planes: 1023 as 768 + 255 and all dense, either side of the carries at 256 and 512, eight references of a group all at 1023
     beside a group of all 0, packed counts and the pair kernel on and off, a read of t = 1024 in the same batch;
  3. eleven planes: 4 100 reads of t = 1024 .. 2047, 2047 as 1792 + 255, with and without the records path;
  4. twelve and sixteen planes, one query per wave: t = 1024 .. 4096, and a read of 7.9 kb through the global-memory forms;
  5. the number of sparse segments of a (query, tile): around the multiples of 4 and 64 and the cap of 255, on both sides of the edge of
     16 / 17 references, on 4 tiles (one pass per tile) and on 13 tiles + 100 (the bit tables);
  6. the branch of rec_epilogue where a reference sits in more sparse segments than the query's threshold;
  7. pairs that share t - d rows for d = 0 (identical) .. t (disjoint), a read without a k-mer inside a pair, a last pair of one."""
import numpy as np
import pytest

import debruijn_common as D
import raxtax_amd as rx
from raxtax_amd.checks import check_run_as_left

pytestmark = pytest.mark.gpu


class Gpu:
    """A family on the device: the tree, its oracle world, handles by option set."""

    def __init__(self, oracle, n_full, tail):
        self.world = D.World(oracle, n_full, tail)
        self.fam = self.world.fam
        bases, off = self.fam.flat()
        self.tree = rx.Tree.new_flat(self.fam.lineages, bases, off, kmer_map=False)
        assert np.array_equal(self.world.otree.original_index(), np.arange(self.fam.n_refs))      # (tests/test_saturated_counts_cpu.py)
        self._lf = None

    def index(self, **opts):
        ix = rx.Index(self.tree, tile_prune=True, debug_taps=True, **opts)      # (tile_prune=True: the self-sample verdict decides nothing)
        assert ix.n_refs == self.fam.n_refs
        return ix

    def lf(self, oracle):
        if self._lf is None:
            self._lf = np.array([oracle.lib.orc_ln_factorial(i) for i in range(2 * 8000 + 8)], dtype=np.float64)
        return self._lf


@pytest.fixture(scope="module")
def gpu(oracle):
    return Gpu(oracle, 4, 37)


@pytest.fixture(scope="module")
def gpu13(oracle):
    return Gpu(oracle, 13, 100)


def classify(index, qs):
    bases, off = D.concat([D.query(a, t) for a, t in qs])
    res = index.classify(bases, off)
    assert res.n_queries == len(qs)
    for j, (a, t) in enumerate(qs):
        assert int(res.t[j]) == t, (a, t)                                      # t = len - 7: no k-mer of the sequence repeats
        assert int(res.status[j]) == (0 if t > 0 else rx._lib.RTX_Q_NO_KMERS), (a, t)
    return res


def check_as_left(g, index, oracle, emul, case, pos):
    """The run as it was left, for the queries of `case` (batch positions `pos`): before any recounting tap."""
    r = g.world.case(case)
    seen = []
    for j, q in enumerate(pos):
        o = check_run_as_left(index, q, int(r["t"][j]), r["counts"][j], r["tables"][j], index.n_refs, emul, g.lf(oracle), f"{case} {r['qs'][j]}")
        assert o["dp"] < 1e-9
        seen.append(o)
    return seen


def check_recount(g, index, case, pos, res, rows=True):
    """The full recount against the closed form and the oracle, the probabilities, the rows."""
    r = g.world.case(case)
    worst = 0.0
    for j, q in enumerate(pos):
        a, t = r["qs"][j]
        got = index.debug_hit_counts(q)
        want = g.fam.expected_counts(a, t)
        assert np.array_equal(got, want), (case, a, t, "closed form", np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        assert np.array_equal(got, r["counts"][j]), (case, a, t, "oracle")
        tz, z = index.debug_prob_table(q, t)
        present = np.bincount(r["counts"][j], minlength=t + 1)[: t + 1] > 0
        if int(want.max()) == t:
            assert present[t]                                                  # bin t itself: a reference that contains the query
        d = float(np.max(np.abs(tz[present] - r["tables"][j][: t + 1][present])))
        worst = max(worst, d)
        assert d < 1e-9, (case, a, t, f"probabilities differ by {d}")
        if rows:
            check_rows(res, q, r["rows"][j], (case, a, t))
    return worst


def check_rows(res, q, want, label):
    got = res.rows(q)
    assert [x.lineage for x in got] == [x["idx"] for x in want], label
    assert [x.confidence_values for x in got] == [x["conf"] for x in want], label
    for x, y in zip(got, want):
        assert abs(x.local_signal - y["local_signal"]) < 1e-6 and abs(x.global_signal - y["global_signal"]) < 1e-9, label


def largest(g, case):
    """For the summary: the largest count of the case and the split that produced it."""
    r = g.world.case(case)
    j = int(np.argmax([int(c.max()) for c in r["counts"]]))
    ref = int(np.argmax(r["counts"][j]))
    a, t = r["qs"][j]
    return f"largest count {int(r['counts'][j][ref])} (query {a}+{t}, reference {ref}: dense + sparse = {g.fam.split(a, t, ref)} before the cap)"


# ---- 1. eight planes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", [4, 0])
def test_eight_planes(gpu, oracle, emul, records):
    index = gpu.index(records=records)
    qs = D.QUERIES["p8"]
    assert max(t for a, t in qs) == 255 and all(t + 7 <= 262 for a, t in qs)
    res = classify(index, qs)
    classes = index.batch_classes()
    print("classes:", classes, "|", largest(gpu, "p8"))
    assert len(classes) == 1 and classes[0]["planes"] == 8 and classes[0]["pair"] and classes[0]["prune"] and classes[0]["tables"]
    assert classes[0]["records"] == (records > 0)
    pos = list(range(len(qs)))
    seen = check_as_left(gpu, index, oracle, emul, "p8", pos)
    print("as left:", [(o["threshold"], o["live"], o["records"]) for o in seen])
    assert sum(o["threshold"] > 0 for o in seen) >= len(qs) - 1              # (t = 8 has no threshold: prune_kernel wants t >= 16)
    assert any(o["records"] for o in seen) == (records > 0)
    print("max |p - p_oracle| =", check_recount(gpu, index, "p8", pos, res))


# ---- 2. ten planes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed,pair", [(True, True), (True, False), (False, True), (False, False)])
def test_ten_planes(gpu, oracle, emul, packed, pair):
    index = gpu.index(packed_counts=packed, hit_pair=pair)
    qs = D.QUERIES["p10"]
    assert all(263 <= t + 7 <= 1030 for a, t in qs)
    res = classify(index, qs)
    classes = index.batch_classes()
    print("classes:", classes, "|", largest(gpu, "p10"))
    assert len(classes) == 1 and classes[0]["planes"] == 10 and classes[0]["tables"]
    assert classes[0]["pair"] == pair and classes[0]["prune"] == pair          # (the pruned path runs on the pair kernel)
    pos = list(range(len(qs)))
    if pair:
        seen = check_as_left(gpu, index, oracle, emul, "p10", pos)
        print("as left:", [(o["threshold"], o["live"], o["records"]) for o in seen])
        assert all(o["threshold"] > 0 for o in seen)
    print("max |p - p_oracle| =", check_recount(gpu, index, "p10", pos, res))
    # the same reads beside one of 1 031 bases (t = 1024, count 1024): a class of twelve planes or more for that one, the same rows for the others
    qs2 = qs + D.QUERIES["p10_long"]
    res2 = classify(index, qs2)
    classes = index.batch_classes()
    print("classes with the read of 1 031 bases:", classes)
    assert len(classes) == 2 and classes[0]["planes"] == 10 and classes[0]["queries"] == len(qs)
    assert classes[1]["planes"] >= 12 and classes[1]["queries"] == 1 and not classes[1]["pair"]
    check_recount(gpu, index, "p10_long", [len(qs)], res2)                      # (the taps reach the last sub-batch: the long read)
    assert int(index.debug_hit_counts(len(qs)).max()) == 1024
    for j in pos:
        check_rows(res2, j, gpu.world.case("p10")["rows"][j], ("p10 beside the long read", qs[j]))


# ---- 3. eleven planes -----------------------------------------------------------------------------------------------------------------
def test_eleven_planes(gpu, oracle, emul):
    index = gpu.index()
    qs = D.p11_queries()
    pos = D.p11_sampled()
    assert len(qs) >= 4096 and all(1031 <= t + 7 <= 2054 for a, t in qs) and (12000, 2047) in qs[:8]
    runs = {}
    for records in (4, 0):
        rx._lib.check(index._lib.rtx_index_set_option(index._h, 18, records))
        res = classify(index, qs)
        classes = index.batch_classes()
        st = index.debug_prune_stats()
        print(f"RTX_OPT_RECORDS = {records}: classes:", classes, "pruning:", st, "|", largest(gpu, "p11"))
        assert len(classes) == 1 and classes[0]["planes"] == 11 and classes[0]["tables"] and classes[0]["pair"] and classes[0]["prune"]
        assert classes[0]["records"] == (records > 0) and st["pairs"] > 0 and st["bound_violations"] == 0
        assert index.last_sub_batch() == (0, len(qs))
        seen = check_as_left(gpu, index, oracle, emul, "p11_sample", pos)
        assert sum(o["threshold"] > 0 for o in seen) > 0.8 * len(pos) and any(o["records"] for o in seen) == (records > 0)
        print("max |p - p_oracle| =", check_recount(gpu, index, "p11_sample", pos, res))
        runs[records] = res
    for f in ("row_off", "row_lineage", "row_conf", "row_local_signal", "global_signal", "t", "status"):
        assert np.array_equal(getattr(runs[4], f), getattr(runs[0], f)), f     # records or counts: the same rows


# ---- 4. twelve and sixteen planes, one query per wave -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cases,planes,global_forms", [(("p12",), 12, False), (("p12", "p16"), 16, False), (("p12", "p16", "p16_global"), 16, True)])
def test_one_query_per_wave(gpu, cases, planes, global_forms):
    index = gpu.index()
    qs = [q for c in cases for q in D.QUERIES[c]]
    res = classify(index, qs)
    classes = index.batch_classes()
    print("classes:", classes, "|", largest(gpu, cases[-1]))
    assert len(classes) == 1 and classes[0]["planes"] == planes and not classes[0]["pair"] and not classes[0]["prune"]
    assert classes[0]["global_memory_forms"] == global_forms
    at = 0
    for c in cases:
        n = len(D.QUERIES[c])
        print(c, "max |p - p_oracle| =", check_recount(gpu, index, c, list(range(at, at + n)), res))
        at += n


# ---- 5. sparse segments per (query, tile) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["gpu", "gpu13"])
def test_sparse_segment_counts(which, request, oracle, emul):
    g = request.getfixturevalue(which)
    index = g.index()
    qs = D.QUERIES["seg"]
    res = classify(index, qs)
    classes = index.batch_classes()
    print("classes:", classes, "tiles:", g.fam.ntiles)
    assert len(classes) == 1 and classes[0]["planes"] == 10 and classes[0]["pair"] and classes[0]["prune"] and classes[0]["tables"]
    sparse = sorted({g.fam.segments(a, t, tile)[0] for a, t in qs for tile in range(g.fam.ntiles)})
    assert set(D.SPARSE_TARGETS) <= set(sparse)
    print("sparse segments per (query, tile):", sparse)
    pos = list(range(len(qs)))
    seen = check_as_left(g, index, oracle, emul, "seg", pos)
    assert all(o["threshold"] > 0 for o in seen)
    print("max |p - p_oracle| =", check_recount(g, index, "seg", pos, res))


# ---- 6. rec_epilogue: a reference in more sparse segments than the threshold -----------------------------------------------------------
def test_records_epilogue_with_the_sparse_maximum_above_the_threshold(gpu, oracle, emul):
    index = gpu.index(records=4)
    qs = D.QUERIES["p8"]
    res = classify(index, qs)
    classes = index.batch_classes()
    assert len(classes) == 1 and classes[0]["planes"] == 8 and classes[0]["prune"] and classes[0]["records"]
    r = gpu.world.case("p8")
    ran = 0
    for q in ((1000, 255), (999, 255)):
        j = qs.index(q)
        best = int(np.argmax(r["counts"][j]))
        smax = gpu.fam.split(q[0], q[1], best)[1]                               # the best reference is reached through sparse segments alone
        assert smax == int(r["counts"][j][best]) >= 254
        o = check_run_as_left(index, j, q[1], r["counts"][j], r["tables"][j], index.n_refs, emul, gpu.lf(oracle), f"all-sparse query {q}")
        print(q, "threshold", o["threshold"], "sparse maximum", smax, "records path", o["records"], "live tiles", o["live"])
        # the taps: the device's threshold really was below the sparse maximum of a visited tile, on the records path -- the branch ran
        assert o["records"] and 0 < o["threshold"] < smax, (q, o)
        ran += 1
        check_rows(res, j, r["rows"][j], q)
    assert ran == 2


# ---- 7. pairs ---------------------------------------------------------------------------------------------------------------------------
def test_pairs(gpu, oracle, emul):
    index = gpu.index(locator=False)                    # (the order by the min-hashes alone: debruijn_common restates it)
    qs = D.pair_queries()
    res = classify(index, qs)
    classes = index.batch_classes()
    print("classes:", classes)
    assert len(classes) == 1 and classes[0]["planes"] == 10 and classes[0]["pair"] and classes[0]["prune"]
    assert index.last_sub_batch() == (0, len(qs)) and len(qs) % 2 == 1
    order = index.debug_order(len(qs)).astype(np.int64)
    assert sorted(order.tolist()) == list(range(len(qs)))
    kinds = D.pair_kinds(qs, order)
    print("processing order:", order.tolist(), "pairs:", kinds)
    assert kinds["identical"] >= 1 and kinds["disjoint"] >= 1 and kinds["single"] == 1 and kinds["no_kmers_inside"] == 1
    assert kinds["odd_lists"] >= 1 and set(D.PAIR_OFFSETS) | {D.PAIR_T} <= kinds["shifts"], kinds
    empty = [j for j, (a, t) in enumerate(qs) if t == 0]
    assert len(empty) == 1 and len(res.rows(empty[0])) == 0
    pos = [j for j, (a, t) in enumerate(qs) if t > 0]
    seen = check_as_left(gpu, index, oracle, emul, "pairs", pos)
    print("as left:", [(o["threshold"], o["live"], o["records"]) for o in seen])
    print("max |p - p_oracle| =", check_recount(gpu, index, "pairs", pos, res))

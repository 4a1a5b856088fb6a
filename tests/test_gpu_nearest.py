"""The nearest reference of every query (RTX_OPT_NEAREST, rtx_nearest.hip): the lowest reference id whose hit count is the query's peak, and
the number of references that share it, against the oracle's hit counts -- lowest index of the maximum, number of entries equal to it,
RTX_NO_REF / 0 where the maximum is 0 or the reference would panic.  Every comparison is for equality.

  * a small database through every counting path without pruning (packed and u16 counts, the pair kernel and the one-query-per-wave
    kernel, every special read), duplicated references (ties; the nearest moves under skip), both skip modes, plus and both strands;
  * 50 000 references (7 tiles, a last tile of 848): the pruned run with queries on the records path and on the dense epilogues (the
    diet), the tile edges, and the same values with the records path off and with pruning off;
  * several sub-batches, and the host mirror in two chunks with run-ahead;
  * the option off: nothing changes, rtx_batch_nearest refuses."""
import ctypes as C

import numpy as np
import pytest

import raxtax_amd as rx
from gpu_common import last_sub_batch_queries
from raxtax_amd import synth
from test_gpu_mixed_lengths import _concat, _long_read

pytestmark = pytest.mark.gpu
NO_REF = 0xFFFFFFFF

_COMP = np.arange(256, dtype=np.uint8)   # the four bits of a one-hot code reversed; a byte above 15 is no code and stays
for _b in range(16):
    _COMP[_b] = int(f"{_b:04b}"[::-1], 2)


def revcomp(seq):
    return _COMP[np.asarray(seq, dtype=np.uint8)[::-1]]


def _expect_one(otree, seq, skip):
    """(peak, nearest, ties) of one sequence as an input of its own."""
    _, counts = otree.hit_counts(seq, skip_exact=skip)
    try:
        otree.classify(seq, skip_exact=skip, raw_confidence=True)
    except ArithmeticError:
        return 0, NO_REF, 0
    m = int(counts.max())
    if m == 0:
        return 0, NO_REF, 0
    return m, int(np.argmax(counts)), int((counts == m).sum())   # (argmax: the first of equals)


def _expect_batch(oracle, otree, seqs, skip, chunk=250):
    peak, nearest, ties = [], [], []
    for a in range(0, len(seqs), chunk):
        bases, off = _concat(seqs[a:a + chunk])
        t, counts = otree.hit_counts_batch(bases, off, skip_exact=skip, threads=16)
        _, _, rc = oracle.prob_tables_batch(t, counts, threads=16)   # rc != 0: the reference would panic
        m = counts.max(axis=1).astype(np.int64)
        m[rc != 0] = 0
        first = counts.argmax(axis=1).astype(np.int64)
        n = (counts == counts.max(axis=1)[:, None]).sum(axis=1).astype(np.int64)
        peak.append(m)
        nearest.append(np.where(m > 0, first, NO_REF))
        ties.append(np.where(m > 0, n, 0))
    return np.concatenate(peak), np.concatenate(nearest), np.concatenate(ties)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. small database, every path without pruning
# ---------------------------------------------------------------------------------------------------------------------------------
_DUPS = ((100, 101), (100, 102), (555, 1400), (1999, 0))   # (source, copy): same bytes -- ties >= 2, and the nearest moves under skip


@pytest.fixture(scope="module")
def small(oracle):
    db = synth.make_db(2000)
    L = db.length
    seq_bytes = db.seq_bytes.copy()
    refs = seq_bytes.reshape(db.n, L)
    for src, dst in _DUPS:
        refs[dst] = refs[src]
    qs = synth.make_queries(db, 64, seed=5)
    rng = np.random.default_rng(6)
    seqs = [qs.seq(i).copy() for i in range(64)]
    for i in range(1, 64, 2):
        seqs[i] = revcomp(seqs[i])
    ref = refs[17].copy()
    amb = refs[40].copy()
    amb[[10, 100, 300]] = [5, 15, 10]        # R, N, Y
    bad = refs[41].copy()
    bad[200] = 0x20                          # no code of the parser
    seqs += [ref[:7].copy(), ref[:8].copy(), revcomp(ref[:9]), amb, revcomp(amb), bad, revcomp(bad),
             (1 << rng.integers(0, 4, L)).astype(np.uint8),          # unrelated
             revcomp(ref[:200]), ref[:200].copy(),                   # t <= 255
             _long_read(rng, db, 1500), revcomp(_long_read(rng, db, 2500)),
             refs[100].copy(), revcomp(refs[555]), refs[0].copy(), refs[1999].copy()]   # the duplicated references themselves
    tree = rx.Tree.new_flat(db.lineages, seq_bytes, db.seq_off)
    otree = oracle.tree_new_flat(db.lineages, seq_bytes, db.seq_off)
    want = {}
    for skip in (False, True):
        fwd = [_expect_one(otree, s, skip) for s in seqs]
        rev = [_expect_one(otree, revcomp(s), skip) for s in seqs]
        want[skip, "plus"] = (np.zeros(len(seqs), np.uint8), fwd)
        minus = np.array([r[0] > f[0] for f, r in zip(fwd, rev)])
        want[skip, "both"] = (minus.astype(np.uint8), [r if m else f for f, r, m in zip(fwd, rev, minus)])
    return tree, seqs, want


def _assert_hits(res, strand, want, what):
    for q, (peak, nearest, ties) in enumerate(want):
        got = (int(res.peak[q]), int(res.nearest[q]), int(res.nearest_ties[q]))
        assert int(res.strand[q]) == int(strand[q]) and got == (peak, nearest, ties), f"{what}: query {q}: strand {int(res.strand[q])} (peak, nearest, ties) {got}, oracle {int(strand[q])} {(peak, nearest, ties)}"


@pytest.mark.parametrize("options", [{}, {"packed_counts": False}, {"hit_pair": False}, {"cluster": False}], ids=["default", "u16", "no-pair", "no-cluster"])
@pytest.mark.parametrize("strand", ["plus", "both"])
def test_small_database_every_path(small, strand, options):
    tree, seqs, want = small
    bases, off = _concat(seqs)
    index = rx.Index(tree, strand=strand, nearest=True, **options)
    for skip in (False, True):
        res = index.classify(bases, off, skip_exact_matches=skip)
        st, w = want[skip, strand]
        assert res.n_queries == len(seqs) and len(res.nearest) == len(seqs) and len(res.nearest_ties) == len(seqs)
        _assert_hits(res, st, w, f"{strand}, skip {skip}, {options}")
        n_ref, n_tie = sum(x[1] != NO_REF for x in w), sum(x[2] >= 2 for x in w)
        print(f"{strand}, skip {skip}, {options}: {len(seqs)} queries, {n_ref} with a nearest reference, {n_tie} with ties, {int(st.sum())} minus")
        assert n_ref < len(seqs)       # (the read of 7 bases at least)
        assert skip or n_tie >= 3      # (the duplicated references given as queries at least)
    # the duplicated references: a tie without skip; under skip the copies are exact matches too, and the nearest is another reference
    i100 = len(seqs) - 4
    a, b = want[False, strand][1][i100], want[True, strand][1][i100]
    assert a[1] == 100 and a[2] >= 3 and b[1] not in (100, 101, 102)
    print(f"length classes: {index.batch_classes()}")   # t <= 255, the bulk, the reads of 1 500 and 2 500 bases


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pruned: records path and diet
# ---------------------------------------------------------------------------------------------------------------------------------
_EDGES = (0, 8191, 8192, 49151, 49152, 49999)


@pytest.fixture(scope="module")
def pruned(oracle):
    db = synth.make_db(50_000)   # 7 tiles, the last one of 848 references
    qs = synth.make_queries(db, 2000, seed=7)
    far = synth.make_queries(db, 96, seed=11, mu_q=0.25, exact_frac=0.0)   # far from every reference: loose bounds, many live tiles, dense epilogues
    rng = np.random.default_rng(12)
    # ... and reads that share next to nothing with any reference (reverse complements, random bases): no threshold, every tile counted, dense epilogues
    lost = [revcomp(qs.seq(i)) for i in range(24)] + [(1 << rng.integers(0, 4, db.length)).astype(np.uint8) for _ in range(8)]
    seqs = [qs.seq(i) for i in range(2000)] + [db.seq(r).copy() for r in _EDGES] + [far.seq(i) for i in range(far.n)] + lost
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    want = {skip: _expect_batch(oracle, otree, seqs, skip) for skip in (False, True)}
    return db, seqs, tree, want


def _run_modes(index, n):
    """record segments of every query of the last sub-batch (0: the dense epilogues)."""
    modes = {}
    for q in last_sub_batch_queries(index, n):
        nseg = C.c_uint32()
        rx._lib.check(index._lib.rtx_debug_run_mode(index._h, int(q), C.byref(nseg)))
        modes[int(q)] = int(nseg.value)
    return modes


@pytest.mark.parametrize("skip", [False, True])
def test_pruned_records_path_and_diet(pruned, skip):
    db, seqs, tree, want = pruned
    n = len(seqs)
    bases, off = _concat(seqs)
    peak, nearest, ties = want[skip]
    index = rx.Index(tree, nearest=True, sub_batch=4096)   # (one sub-batch: the taps below then see every query)
    res = index.classify(bases, off, skip_exact_matches=skip)
    classes = index.batch_classes()
    st = index.debug_prune_stats()
    modes = _run_modes(index, n)
    n_rec, n_dense = sum(v > 0 for v in modes.values()), sum(v == 0 for v in modes.values())
    print(f"skip {skip}: {n} queries, classes {classes}; {st['queries_with_threshold']} with a threshold, {st['record_queries']} on the records path; "
          f"last sub-batch: {n_rec} on the records path, {n_dense} on the dense epilogues; {int((ties >= 2).sum())} queries with ties, {int((nearest == NO_REF).sum())} without a reference")
    assert all(c["prune"] and c["records"] for c in classes) and st["queries_with_threshold"] > 0 and st["bound_violations"] == 0
    assert n_rec > 0 and n_dense > 0, "the checked set must hold queries on the records path and on the dense epilogues"
    bad = np.nonzero((res.peak != peak) | (res.nearest != nearest) | (res.nearest_ties != ties))[0]
    assert len(bad) == 0, [(int(q), modes.get(int(q)), (int(res.peak[q]), int(res.nearest[q]), int(res.nearest_ties[q])), (int(peak[q]), int(nearest[q]), int(ties[q]))) for q in bad[:8]]
    if not skip:   # a reference given as a query is its own nearest one: the tile edges and the short last tile
        for k, r in enumerate(_EDGES):
            assert int(res.nearest[2000 + k]) == r, (r, int(res.nearest[2000 + k]))
    for what, kw in (("records off", dict(records=0)), ("pruning off", dict(tile_prune=False))):
        other = rx.Index(tree, nearest=True, **kw)
        r2 = other.classify(bases, off, skip_exact_matches=skip)
        c2 = other.batch_classes()
        assert not any(c["records"] for c in c2) and (what != "pruning off" or not any(c["prune"] for c in c2)), (what, c2)
        assert np.array_equal(r2.nearest, res.nearest) and np.array_equal(r2.nearest_ties, res.nearest_ties) and np.array_equal(r2.peak, res.peak), what


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. several sub-batches and chunks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sub_batches_and_chunks_with_run_ahead(pruned):
    db, seqs, tree, want = pruned
    n = len(seqs)
    bases, off = _concat(seqs)
    peak, nearest, ties = want[False]
    index = rx.Index(tree, nearest=True, sub_batch=512)
    res = index.classify(bases, off)
    assert index.sub_batch_size() <= 512 and n > 3 * 512   # at least 4 sub-batches
    assert np.array_equal(res.peak, peak) and np.array_equal(res.nearest, nearest) and np.array_equal(res.nearest_ties, ties)
    queries = [(f"q{i}", s) for i, s in enumerate(seqs)]

    def run(chunk):
        labels, hits = [], []
        rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: labels.append(label), False,
                  hit=lambda *a: hits.append(a))
        return labels, hits

    one_labels, one = run(n)
    ahead0 = index.run_ahead_stats[0]
    two_labels, two = run((n + 1) // 2)
    assert index.run_ahead_stats[0] > ahead0, "the second chunk was not enqueued ahead"
    assert one == two and one_labels == two_labels == [h[0] for h in one]
    ok = np.nonzero(res.status == 0)[0]          # (a query without a message has no hit line either)
    assert [h[0] for h in one] == [f"q{i}" for i in ok]
    assert [h[1:] for h in one] == [(0, int(peak[i]), int(res.t[i]), int(nearest[i]), int(ties[i])) for i in ok]
    # a handle with the option off hands RTX_NO_REF and 0 to the same callback
    plain = rx.Index(tree, sub_batch=512)
    off_hits = []
    rx.raxtax(queries[:300], plain, False, False, 300, lambda *a: None, False, hit=lambda *a: off_hits.append(a))
    assert off_hits and all(h[4:] == (NO_REF, 0) for h in off_hits) and [h[2] for h in off_hits] == [h[2] for h in one[:len(off_hits)]]
    # handles that disagree on the option are refused
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(queries[:8], [index, plain], False, False, 4, lambda *a: None, False, hit=lambda *a: None)
    assert e.value.code == rx._lib.RTX_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. off means off
# ---------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(small):
    tree, seqs, want = small
    bases, off = _concat(seqs)
    on, plain = rx.Index(tree, nearest=True), rx.Index(tree)
    for skip in (False, True):
        a, b = on.classify(bases, off, skip_exact_matches=skip), plain.classify(bases, off, skip_exact_matches=skip)
        assert b.nearest is None and b.nearest_ties is None and a.nearest is not None
        pn, pt = rx._lib.u32p(), rx._lib.u32p()
        assert plain._lib.rtx_batch_nearest(plain._h, C.byref(pn), C.byref(pt)) == rx._lib.RTX_ERR_STATE
        assert on._lib.rtx_batch_nearest(on._h, C.byref(pn), None) == 0 and on._lib.rtx_batch_nearest(on._h, None, C.byref(pt)) == 0
        for f in ("t", "status", "global_signal", "row_off", "row_lineage", "row_node", "row_depth", "row_conf", "row_local_signal", "peak", "strand"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        ea, eb = on.device_exact_matches(), plain.device_exact_matches()
        assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    # setting the option drops the uploaded batch
    plain.upload(bases, off)
    rx._lib.check(plain._lib.rtx_index_set_option(plain._h, 26, 1))
    with pytest.raises(rx.RtxError) as e:
        plain.run()
    assert e.value.code == rx._lib.RTX_ERR_STATE
    plain.nearest_on = True
    res = plain.classify(bases, off)   # ... and the handle names the nearest references from the next upload on
    _assert_hits(res, *want[False, "plus"], "switched on later")
    # ... and off again
    rx._lib.check(plain._lib.rtx_index_set_option(plain._h, 26, 0))
    plain.nearest_on = False
    assert plain.classify(bases, off).nearest is None
    assert plain._lib.rtx_index_set_option(plain._h, 26, 2) == rx._lib.RTX_ERR_INVALID
    # a reference shard refuses it
    from raxtax_amd.sharded import ShardIndex, shard_cuts
    shard = ShardIndex(tree, 0, shard_cuts(tree.num_tips, 2))
    with pytest.raises(rx.RtxError) as e:
        rx._lib.check(shard._lib.rtx_index_set_option(shard._h, 26, 1))
    assert e.value.code == rx._lib.RTX_ERR_INVALID

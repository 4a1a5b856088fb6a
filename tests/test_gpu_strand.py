"""Both-strand mode (RTX_OPT_STRAND, rtx_strand.hip): a read given as its reverse complement is classified as its reverse complement.

The library appends the reverse complement of every query on the device, classifies both orientations and reports, per query, the one
with the larger PEAK (the largest hit count over the references as the probability stage sees them; ties go to the given orientation).
Everything a query gets must be what the oracle gives for the chosen sequence as an input of its own.  The reverse complements the
expectations are made from are numpy's, never the library's.

  * a small database (dense paths) with every kind of read the issue names, both skip modes, and the option off;
  * the pruned and the records path: a flipped batch under both strands equals the un-flipped batch under plus, query by query;
  * the refusals, the option dropping the batch, and the host mirror in two chunks with run-ahead."""
import numpy as np
import pytest

import raxtax_amd as rx
from gpu_common import assert_rows_equivalent, rows_of
from raxtax_amd import synth
from test_gpu_mixed_lengths import _concat, _long_read

pytestmark = pytest.mark.gpu

_COMP = np.arange(256, dtype=np.uint8)   # the four bits of a one-hot code reversed; a byte above 15 is no code and stays
for _b in range(16):
    _COMP[_b] = int(f"{_b:04b}"[::-1], 2)


def revcomp(seq):
    return _COMP[np.asarray(seq, dtype=np.uint8)[::-1]]


def _oracle_view(oracle, otree, seq, skip):
    """(peak, t, rows or None, counts) of one sequence as an input of its own: peak 0 and no rows where the reference would panic."""
    t, counts = otree.hit_counts(seq, skip_exact=skip)
    try:
        rows, _ = otree.classify(seq, skip_exact=skip, raw_confidence=True)
    except ArithmeticError:
        return 0, int(t), None, counts
    return int(counts.max()), int(t), rows, counts


def _check_queries(oracle, otree, res, ex, seqs, ids, skip, both, what):
    """Strand by the tie rule, peak bit-exact, t / status / rows / exact matches those of the chosen sequence.  Returns (strands, verified ties)."""
    ex_ids, ex_off = ex
    ties = 0
    strands = []
    for q in ids:
        q = int(q)
        fwd = _oracle_view(oracle, otree, seqs[q], skip)
        rev = _oracle_view(oracle, otree, revcomp(seqs[q]), skip) if both else None
        minus = both and rev[0] > fwd[0]   # strictly larger, else the given orientation
        strands.append(int(minus))
        chosen = revcomp(seqs[q]) if minus else seqs[q]
        peak, t, want, counts = rev if minus else fwd
        label = f"{what}: query {q} (length {len(seqs[q])}, skip {skip})"
        assert int(res.strand[q]) == int(minus), f"{label}: strand {int(res.strand[q])}, peaks fwd {fwd[0]} rev {rev[0] if both else None}"
        assert int(res.peak[q]) == peak, f"{label}: peak {int(res.peak[q])}, oracle {peak}"
        assert int(res.t[q]) == t, f"{label}: t {int(res.t[q])}, oracle {t}"
        assert np.array_equal(ex_ids[int(ex_off[q]):int(ex_off[q + 1])], otree.exact_matches(chosen)), f"{label}: exact matches"
        got = res.rows(q)
        if want is None:
            assert int(res.status[q]) != 0 and not got, label
            continue
        assert int(res.status[q]) == 0, label
        if [g.lineage for g in got] != [r["idx"] for r in want] or [g.confidence_values for g in got] != [r["conf"] for r in want]:
            tables, _, rc = oracle.prob_tables_batch(np.array([t], np.uint32), counts[None, :])
            assert rc[0] == 0
            ties += assert_rows_equivalent(got, want, tables[0][counts], otree.lineages, label) > 0
        else:
            for g, r in zip(got, want):
                assert abs(g.local_signal - r["local_signal"]) < 1e-6 and abs(g.global_signal - r["global_signal"]) < 1e-9, label
    return np.array(strands), ties


def test_small_database_every_kind_of_read(oracle):
    db = synth.make_db(2000)
    qs = synth.make_queries(db, 64, seed=5)
    L = db.length
    rng = np.random.default_rng(6)
    seqs = [qs.seq(i).copy() for i in range(64)]
    for i in range(1, 64, 2):
        seqs[i] = revcomp(seqs[i])
    ref = db.seq(17)
    amb = db.seq(40).copy()
    amb[[10, 100, 300]] = [5, 15, 10]        # R, N, Y
    bad = db.seq(41).copy()
    bad[200] = 0x20                          # no code of the parser
    palin = np.tile(np.array([1, 2, 4, 8], np.uint8), 4)   # ACGT x 4
    assert np.array_equal(revcomp(palin), palin)
    n_special = len(seqs)
    seqs += [ref[:7].copy(), ref[:8].copy(), revcomp(ref[:9]), amb, revcomp(amb), bad, revcomp(bad), palin,
             (1 << rng.integers(0, 4, L)).astype(np.uint8),          # unrelated
             revcomp(ref[:200]),                                     # t <= 255
             revcomp(_long_read(rng, db, 1500)), revcomp(_long_read(rng, db, 2500))]
    i_palin = n_special + 7
    bases, off = _concat(seqs)
    n = len(seqs)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    both, plus = rx.Index(tree, strand="both"), rx.Index(tree)
    for skip in (False, True):
        res = both.classify(bases, off, skip_exact_matches=skip)
        assert res.n_queries == n and len(res.strand) == n and len(res.peak) == n
        strands, ties = _check_queries(oracle, otree, res, both.device_exact_matches(), seqs, range(n), skip, True, "both")
        assert res.strand[i_palin] == 0
        assert strands[:64].tolist() == [i & 1 for i in range(64)], "the flipped synthetic queries were not all recognised by the oracle's peaks"
        print(f"both strands, skip {skip}: {n} queries, {int(strands.sum())} minus, {ties} with a verified tie between sibling taxa")
        # the option off: the orientation as given, the peak still filled
        res0 = plus.classify(bases, off, skip_exact_matches=skip)
        assert (res0.strand == 0).all()
        _check_queries(oracle, otree, res0, plus.device_exact_matches(), seqs, range(n), skip, False, "plus")


def _oracle_peaks(otree, seqs, skip, chunk=250):
    out = []
    for a in range(0, len(seqs), chunk):
        bases, off = _concat(seqs[a:a + chunk])
        _, counts = otree.hit_counts_batch(bases, off, skip_exact=skip, threads=16)
        out.append(counts.max(axis=1).astype(np.int64))
    return np.concatenate(out)


@pytest.fixture(scope="module")
def pruned():
    db = synth.make_db(50_000)   # 7 tiles
    qs = synth.make_queries(db, 2000, seed=7)
    flip = np.random.default_rng(8).random(2000) < 0.5
    seqs = [qs.seq(i) for i in range(2000)]
    flipped = [revcomp(s) if f else s for s, f in zip(seqs, flip)]
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    return db, qs, flip, seqs, flipped, tree


def test_pruned_and_records_path(oracle, pruned):
    db, qs, flip, seqs, flipped, tree = pruned
    n = len(seqs)
    fb, foff = _concat(flipped)
    both, plus = rx.Index(tree, strand="both"), rx.Index(tree)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    sample = np.sort(np.random.default_rng(9).choice(n, 64, replace=False))
    for skip in (False, True):
        res = both.classify(fb, foff, skip_exact_matches=skip)
        st = both.debug_prune_stats()
        print(f"skip {skip}: prune stats of the batch of {2 * n}: {st['queries_with_threshold']} with a threshold, {st['record_queries']} on the records path")
        assert st["pairs"] > 0 and st["queries_with_threshold"] > 0 and st["record_queries"] > 0 and st["bound_violations"] == 0
        ex = both.device_exact_matches()
        _check_queries(oracle, otree, res, ex, flipped, sample, skip, True, "pruned, both")
        ref = plus.classify(qs.bases, qs.base_off, skip_exact_matches=skip)
        ex_ref = plus.device_exact_matches()
        # no ties on this fixture, from the oracle's peaks of every query in both orientations: the orientation that lost is far below
        fwd_peak, rev_peak = _oracle_peaks(otree, seqs, skip), _oracle_peaks(otree, [revcomp(x) for x in seqs], skip)
        print(f"skip {skip}: smallest forward peak {int(fwd_peak.min())}, largest reverse-complement peak {int(rev_peak.max())}, smallest margin {int((fwd_peak - rev_peak).min())}")
        assert (fwd_peak > rev_peak).all()
        assert np.array_equal(ref.peak, fwd_peak)
        assert np.array_equal(res.strand.astype(bool), flip)
        assert np.array_equal(res.peak, ref.peak) and np.array_equal(res.t, ref.t) and np.array_equal(res.status, ref.status)
        assert np.array_equal(res.global_signal, ref.global_signal) and np.array_equal(res.row_off, ref.row_off)
        for a, b in ((res.row_lineage, ref.row_lineage), (res.row_node, ref.row_node), (res.row_depth, ref.row_depth), (res.row_conf, ref.row_conf),
                     (res.row_local_signal, ref.row_local_signal), (ex[0], ex_ref[0]), (ex[1], ex_ref[1])):
            assert np.array_equal(a, b)
        for q in sample[:8]:
            assert all(np.array_equal(x, y) for x, y in zip(rows_of(res, int(q)), rows_of(ref, int(q))))


def test_refusals_and_state(oracle, pruned):
    db, qs, flip, seqs, flipped, tree = pruned
    small = synth.make_db(1500, fanouts=(2, 2, 3, 3, 3, 2))
    sq = synth.make_queries(small, 32, seed=3)
    stree = rx.Tree.new_flat(small.lineages, small.seq_bytes, small.seq_off)
    both = rx.Index(stree, strand="both")
    # exact-match ids passed by the caller
    with pytest.raises(rx.RtxError) as e:
        both.classify(sq.bases, sq.base_off, *both.exact_matches(sq.bases, sq.base_off))
    assert e.value.code == rx._lib.RTX_ERR_INVALID and "exact" in str(e.value)
    # a handle without the device lookup
    with pytest.raises(rx.RtxError) as e:
        rx.Index(stree, strand="both", device_exact=False).classify(sq.bases, sq.base_off)
    assert e.value.code == rx._lib.RTX_ERR_STATE
    # a reference shard
    from raxtax_amd.sharded import ShardIndex, shard_cuts
    shard = ShardIndex(stree, 0, shard_cuts(small.n, 2))
    with pytest.raises(rx.RtxError) as e:
        rx._lib.check(shard._lib.rtx_index_set_option(shard._h, 25, 1))
    assert e.value.code == rx._lib.RTX_ERR_INVALID
    # no device text
    both.classify(sq.bases, sq.base_off)
    with pytest.raises(rx.RtxError) as e:
        both.last_text()
    assert e.value.code == rx._lib.RTX_ERR_STATE and "STRAND" in str(e.value)
    # setting the option drops the uploaded batch
    plain = rx.Index(stree)
    plain.upload(sq.bases, sq.base_off)
    rx._lib.check(plain._lib.rtx_index_set_option(plain._h, 25, 1))
    with pytest.raises(rx.RtxError) as e:
        plain.run()
    assert e.value.code == rx._lib.RTX_ERR_STATE
    res = plain.classify(sq.bases, sq.base_off)   # ... and the handle classifies both strands from the next upload on
    assert res.n_queries == sq.n and len(res.strand) == sq.n

    # the host mirror: two chunks, the second enqueued ahead of the end of the first, give the messages of one chunk
    queries = [(f"q{i}", s) for i, s in enumerate(flipped)]
    index = rx.Index(tree, strand="both", sub_batch=512)

    def run(chunk):
        msgs, infos = [], []
        rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: msgs.append((label, out, tsv)), True,
                  info=lambda label, strand, peak, t: infos.append((label, strand, peak, t)))
        return msgs, infos

    one, one_info = run(len(queries))
    ahead0 = index.run_ahead_stats[0]
    two, two_info = run(len(queries) // 2)
    assert index.run_ahead_stats[0] > ahead0, "the second chunk was not enqueued ahead"
    assert one == two and one_info == two_info
    assert [m[0] for m in one] == [q[0] for q in queries] == [i[0] for i in one_info]
    assert [bool(i[1]) for i in one_info] == flip.tolist()
    # the `.tsv` sequence column prints the orientation that was classified: the un-flipped read
    for k in np.nonzero(flip)[0][:4].tolist() + np.nonzero(~flip)[0][:2].tolist():
        assert one[k][2].split("\n")[0].split("\t")[-1] == oracle.decompress_sequence(seqs[k]), k

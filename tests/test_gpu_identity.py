"""Alignment identity (RTX_OPT_IDENTITY, rtx_identity.hip): the semi-global edit distance of every query, in the orientation that was
classified, to its nearest reference.  Every comparison is for equality: the nearest reference comes from the oracle's hit counts (as in
test_gpu_nearest.py), the distance from the numpy Sellers recurrence of test_identity_cpu.py on the chosen orientation against that
reference's bytes, and it is NO_DIST exactly where there is no nearest reference or the query is longer than 4096 bases.

  * 2000 references of many lengths (64, 65, 128, 600, 658, 2500 among them: text-chunk edges and the end of the systolic drain), some
    duplicated; about a hundred queries -- copies, substitutions, indels, infixes, overhangs, ambiguity codes, a byte that is no code, short
    reads, reads of 1023 .. 4097 bases around a reference (the switch from groups of 16 lanes to the whole wave at 1024), half of them as
    reverse complements -- through both strand modes, both skip modes and three count layouts / processing orders, each batch once raw
    (it holds a byte above 15) and once packed two bases per byte (without that read);
  * 50 000 references (7 tiles): the pruned path feeds the same nearest reference; several sub-batches; the host mirror in two chunks with
    run-ahead, and with dereplication;
  * the option off changes nothing, and the option is refused where it cannot work."""
import ctypes as C

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth
from test_gpu_mixed_lengths import _concat
from test_gpu_nearest import NO_REF, _DUPS, _expect_batch, _expect_one, revcomp
from test_identity_cpu import sellers

pytestmark = pytest.mark.gpu
NO_DIST = 0xFFFFFFFF
MAX_QUERY = 4096


def _subst(rng, s, k):
    s = s.copy()
    for p in rng.choice(len(s), k, replace=False):
        s[p] = {1: 2, 2: 4, 4: 8, 8: 1}.get(int(s[p]), 1)
    return s


def _indel(rng, s, n_ins, n_del):
    s = list(s)
    for _ in range(n_ins):
        s.insert(int(rng.integers(0, len(s) + 1)), int(1 << rng.integers(0, 4)))
    for _ in range(n_del):
        del s[int(rng.integers(0, len(s)))]
    return np.array(s, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. small database, references of many lengths
# ---------------------------------------------------------------------------------------------------------------------------------
_LENGTHS = {3: 64, 4: 65, 5: 128, 6: 600, 8: 2500, 9: 63, 10: 129, 13: 1024, 14: 1025, 15: 656}


@pytest.fixture(scope="module")
def small(oracle):
    db = synth.make_db(2000)
    L = db.length   # 658
    rng = np.random.default_rng(28)
    rnd = lambda n: (1 << rng.integers(0, 4, n)).astype(np.uint8)
    refs = [r.copy() for r in db.seq_bytes.reshape(db.n, L)]
    for i, n in _LENGTHS.items():
        refs[i] = refs[i][:n] if n <= L else np.concatenate([refs[i], rnd(n - L)])
    for i in range(20, 2000, 37):                       # ... and a spread of lengths around the usual one
        refs[i] = refs[i][:L - 1 - (i % 90)]
    for src, dst in _DUPS:
        refs[dst] = refs[src].copy()
    seq_bytes, seq_off = _concat(refs)
    seqs = [refs[17].copy(), refs[3].copy(), refs[4].copy(), refs[5].copy(), refs[6].copy(), refs[8].copy(), refs[13].copy(), refs[14].copy(),
            refs[100].copy(), refs[555].copy(), refs[0].copy(), refs[1999].copy(), refs[57].copy(), refs[15].copy()]        # exact copies
    seqs += [_subst(rng, refs[200 + k], k) for k in (1, 2, 3, 5, 8, 13, 20, 30, 40)]                                      # substitutions
    seqs += [_subst(rng, refs[8], 25), _subst(rng, refs[6], 7), _subst(rng, refs[5], 3), _subst(rng, refs[3], 2)]
    seqs += [_indel(rng, refs[300 + k], a, b) for k, (a, b) in enumerate(((1, 0), (0, 1), (2, 2), (5, 0), (0, 5), (3, 7), (10, 10)))]
    seqs += [np.insert(refs[310], 0, 1), np.delete(refs[311], 0), np.append(refs[312], 2), refs[313][:-1].copy()]        # ... at the ends
    seqs += [refs[400 + k][a:a + 200].copy() for k, a in enumerate((0, 1, 63, 64, 229, 458))]                             # infixes of 200 bases
    seqs += [_subst(rng, refs[410][100:300], 4), _indel(rng, refs[411][300:500], 2, 1)]
    seqs += [np.concatenate([refs[6], rnd(30)]), np.concatenate([refs[5], rnd(30)]), np.concatenate([refs[3], rnd(30)]),  # hang over a short reference
             np.concatenate([rnd(30), refs[6]]), np.concatenate([refs[420][:300], rnd(30)]), np.concatenate([rnd(12), refs[4], rnd(12)])]
    amb = refs[40].copy()
    amb[[10, 100, 300]] = [5, 15, 10]                   # R, N, Y
    amb2 = refs[42].copy()
    amb2[[0, 63, 64, 657]] = [3, 6, 12, 15]
    bad = refs[41].copy()
    bad[200] = 0x20                                     # no code of the parser
    bad0 = refs[43].copy()
    bad0[[5, 640]] = [0x7F, 0x41]
    seqs += [amb, amb2, _subst(rng, amb, 6)]
    i_bad = len(seqs)
    seqs += [bad, bad0]
    seqs += [rnd(L), rnd(300)]                          # unrelated
    seqs += [refs[17][:7].copy(), refs[17][:8].copy(), refs[17][:9].copy(), refs[17][100:120].copy()]                     # short reads
    for k, n in enumerate((1023, 1024, 1025, 1500, 4095, 4096, 4097)):  # around a reference: the lane-group switch and the longest read
        core = _subst(rng, refs[500 + k], 3 * k)
        a = (n - len(core)) // 3
        seqs.append(np.concatenate([rnd(a), core, rnd(n - len(core) - a)]))
    seqs += [np.concatenate([rnd(100), refs[8], rnd(200)]), _indel(rng, refs[8], 6, 6), refs[8][700:2300].copy()]          # ... and the long reference
    seqs += [_subst(rng, refs[600 + k], 1 + k % 9) for k in range(max(0, 100 - len(seqs)))]
    n_plain = len(seqs)
    for i in range(1, n_plain, 2):                      # half of them given as reverse complements
        seqs[i] = revcomp(seqs[i])
    tree = rx.Tree.new_flat(db.lineages, seq_bytes, seq_off)
    otree = oracle.tree_new_flat(db.lineages, seq_bytes, seq_off)
    by_id = [refs[int(i)] for i in tree.original_index()]   # reference ids are the order of the tree's (sorted) lineages
    dist_of = {}

    def dist(q, minus, ref):
        key = (q, minus, ref)
        if key not in dist_of:
            s = revcomp(seqs[q]) if minus else seqs[q]
            dist_of[key] = sellers(s, by_id[ref])
        return dist_of[key]

    want = {}
    for skip in (False, True):
        fwd = [_expect_one(otree, s, skip) for s in seqs]
        rev = [_expect_one(otree, revcomp(s), skip) for s in seqs]
        for strand in ("plus", "both"):
            minus = [strand == "both" and r[0] > f[0] for f, r in zip(fwd, rev)]
            rows = []
            for q, (f, r, m) in enumerate(zip(fwd, rev, minus)):
                peak, nearest, _ = r if m else f
                d = NO_DIST if nearest == NO_REF or len(seqs[q]) > MAX_QUERY else dist(q, m, nearest)
                rows.append((int(m), nearest, d, len(seqs[q])))
            want[skip, strand] = rows
    return tree, seqs, want, i_bad, by_id


def _assert_identity(res, want, ids, what):
    assert len(res.nearest_dist) == len(ids) and len(res.query_len) == len(ids)
    for k, q in enumerate(ids):
        got = (int(res.strand[k]), int(res.nearest[k]), int(res.nearest_dist[k]), int(res.query_len[k]))
        assert got == want[q], f"{what}: query {q}: (strand, nearest, dist, qlen) {got}, expected {want[q]}"


@pytest.mark.parametrize("strand, skip, options", [("plus", False, {}), ("plus", True, {}), ("both", False, {}), ("both", True, {}),
                                                   ("plus", False, {"packed_counts": False}), ("plus", False, {"hit_pair": False}),
                                                   ("plus", False, {"cluster": False})],
                         ids=["plus", "plus-skip", "both", "both-skip", "u16", "no-pair", "no-cluster"])
def test_small_database_sweep(small, strand, skip, options):
    tree, seqs, want, i_bad, _ = small
    w = want[skip, strand]
    index = rx.Index(tree, strand=strand, identity=True, **options)
    everything = list(range(len(seqs)))
    clean = [q for q in everything if seqs[q].max() <= 15]
    assert len(clean) == len(seqs) - 2 and i_bad not in clean
    for ids, form in ((everything, "raw"), (clean, "packed")):   # a byte above 15 in the batch: its input set travels one byte per base
        bases, off = _concat([seqs[q] for q in ids])
        res = index.classify(bases, off, skip_exact_matches=skip)
        _assert_identity(res, w, ids, f"{strand}, skip {skip}, {options}, {form}")
    n_dist = sum(x[2] != NO_DIST for x in w)
    n_zero = sum(x[2] == 0 for x in w)
    print(f"{strand}, skip {skip}, {options}: {len(seqs)} queries, {n_dist} with a distance ({n_zero} of them 0), {sum(x[0] for x in w)} minus, "
          f"largest distance {max(x[2] for x in w if x[2] != NO_DIST)}")
    assert len(seqs) >= 100 and n_dist < len(seqs)     # (the read of 4097 bases at least)
    long_one = [q for q in everything if len(seqs[q]) == 4097]
    assert len(long_one) == 1 and w[long_one[0]][2] == NO_DIST and w[long_one[0]][1] != NO_REF
    assert all((x[2] == NO_DIST) == (x[1] == NO_REF or x[3] > MAX_QUERY) for x in w)
    if strand == "both" and not skip:
        assert n_zero >= 14                              # the exact copies and the infixes, whichever way round they were given


def test_the_distance_is_the_host_function_s(small):
    """rtx_semiglobal_distance on the pairs the device aligned: what a caller would spot-check with."""
    tree, seqs, want, _, refs = small
    for q, (minus, nearest, d, n) in enumerate(want[False, "both"]):
        if d != NO_DIST:
            assert rx.semiglobal_distance(revcomp(seqs[q]) if minus else seqs[q], refs[nearest]) == d, q


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pruned path, several sub-batches, the host mirror
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pruned(oracle):
    db = synth.make_db(50_000)   # 7 tiles
    qs = synth.make_queries(db, 600, seed=7)
    seqs = [qs.seq(i) for i in range(600)]
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    otree = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    _, nearest, _ = _expect_batch(oracle, otree, seqs, False)
    index = rx.Index(tree, identity=True, sub_batch=128)
    res = index.classify(*_concat(seqs))
    by_id = tree.original_index()                           # reference id -> its place in db (ids are the order of the sorted lineages)
    return db, seqs, tree, nearest, index, res, by_id


def test_pruned_path_feeds_the_same_nearest(pruned):
    db, seqs, tree, nearest, index, res, by_id = pruned
    classes = index.batch_classes()
    assert all(c["prune"] for c in classes), classes
    assert index.sub_batch_size() <= 128 and len(seqs) > 3 * 128   # at least 4 sub-batches
    assert np.array_equal(res.nearest, nearest)
    assert np.array_equal(res.query_len, [len(s) for s in seqs])
    sample = np.random.default_rng(3).choice(len(seqs), 32, replace=False)
    for q in sample:
        want = NO_DIST if nearest[q] == NO_REF else sellers(seqs[q], db.seq(int(by_id[int(nearest[q])])))
        assert int(res.nearest_dist[q]) == want, (int(q), int(res.nearest_dist[q]), want)
    print(f"{len(seqs)} queries over {index.sub_batch_size()} per sub-batch, 32 checked; distances of the batch: min {int(res.nearest_dist.min())}, "
          f"median {int(np.median(res.nearest_dist))}, max {int(res.nearest_dist.max())}")


def test_host_mirror_in_two_chunks_with_run_ahead(pruned):
    db, seqs, tree, nearest, index, res, _ = pruned
    n = len(seqs)
    queries = [(f"q{i}", s) for i, s in enumerate(seqs)]
    ok = np.nonzero(res.status == 0)[0]
    direct = [(f"q{i}", int(res.strand[i]), int(res.peak[i]), int(res.t[i]), int(res.nearest[i]), int(res.nearest_ties[i]), int(res.nearest_dist[i]),
               int(res.query_len[i])) for i in ok]

    def run(handle, qs, chunk):
        got = []
        rx.raxtax(qs, handle, False, False, chunk, lambda label, out, tsv: None, False, align=lambda *a: got.append(a))
        return got

    ahead0 = index.run_ahead_stats[0]
    two = run(index, queries, (n + 1) // 2)
    assert index.run_ahead_stats[0] > ahead0, "the second chunk was not enqueued ahead"
    assert two == direct
    # dereplication: a chunk with copies -- every copy reports its representative's distance
    copies = queries[:200] + [(f"c{i}", queries[i % 50][1]) for i in range(150)] + queries[200:]
    derep = rx.Index(tree, identity=True, derep=True, sub_batch=128)
    got = run(derep, copies, (len(copies) + 1) // 2)
    assert rx.raxtax_last_derep()[1] < rx.raxtax_last_derep()[0]
    by_label = {d[0]: d[1:] for d in direct}
    assert [g[0] for g in got] == [c[0] for c in copies if (c[0] if c[0][0] == "q" else f"q{int(c[0][1:]) % 50}") in by_label]
    for g in got:
        src = g[0] if g[0][0] == "q" else f"q{int(g[0][1:]) % 50}"
        assert g[1:] == by_label[src], g[0]
    # a handle with the option off hands NO_DIST and the length to the same callback
    plain = rx.Index(tree, nearest=True, sub_batch=128)
    off = run(plain, queries[:100], 100)
    assert off and all(h[6] == NO_DIST and h[7] == len(seqs[int(h[0][1:])]) for h in off) and [h[:6] for h in off] == [d[:6] for d in direct[:len(off)]]
    # handles that disagree on the option are refused
    with pytest.raises(rx.RtxError) as e:
        run([index, plain], queries[:8], 4)
    assert e.value.code == rx._lib.RTX_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the option
# ---------------------------------------------------------------------------------------------------------------------------------
def test_option_handling(small):
    tree, seqs, want, _, _ = small
    bases, off = _concat(seqs)
    on, plain = rx.Index(tree, identity=True), rx.Index(tree, nearest=True)
    assert on.nearest_on and on.identity_on
    pd, pl = rx._lib.u32p(), rx._lib.u32p()
    for skip in (False, True):
        a, b = on.classify(bases, off, skip_exact_matches=skip), plain.classify(bases, off, skip_exact_matches=skip)
        assert b.nearest_dist is None and b.query_len is None and a.nearest_dist is not None
        assert plain._lib.rtx_batch_identity(plain._h, C.byref(pd), C.byref(pl)) == rx._lib.RTX_ERR_STATE
        assert on._lib.rtx_batch_identity(on._h, C.byref(pd), None) == 0 and on._lib.rtx_batch_identity(on._h, None, C.byref(pl)) == 0
        for f in ("t", "status", "global_signal", "row_off", "row_lineage", "row_node", "row_depth", "row_conf", "row_local_signal", "peak", "strand",
                  "nearest", "nearest_ties"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        ea, eb = on.device_exact_matches(), plain.device_exact_matches()
        assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    set_option = lambda ix, opt, v: ix._lib.rtx_index_set_option(ix._h, opt, v)
    # nearest cannot be switched off under it; the option itself can, and drops the uploaded batch both ways
    assert set_option(on, 26, 0) == rx._lib.RTX_ERR_STATE
    on.upload(bases, off)
    assert set_option(on, 28, 0) == 0
    with pytest.raises(rx.RtxError) as e:
        on.run()
    assert e.value.code == rx._lib.RTX_ERR_STATE
    on.identity_on = False
    assert on.classify(bases, off).nearest_dist is None
    assert set_option(on, 28, 2) == rx._lib.RTX_ERR_INVALID
    plain.upload(bases, off)
    assert set_option(plain, 28, 1) == 0
    with pytest.raises(rx.RtxError) as e:
        plain.run()
    assert e.value.code == rx._lib.RTX_ERR_STATE
    plain.identity_on = True
    _assert_identity(plain.classify(bases, off), want[False, "plus"], list(range(len(seqs))), "switched on later")
    # refused without nearest ...
    bare = rx.Index(tree)
    assert set_option(bare, 28, 1) == rx._lib.RTX_ERR_STATE
    # ... on a handle created from postings (it holds no reference sequences) ...
    from raxtax_amd.sharded import KmerShardIndex, ShardIndex, shard_cuts
    posts = KmerShardIndex(tree, 0, [0, 65536])
    assert set_option(posts, 26, 1) == 0
    assert set_option(posts, 28, 1) == rx._lib.RTX_ERR_STATE
    # ... and on a reference shard
    shard = ShardIndex(tree, 0, shard_cuts(tree.num_tips, 2))
    assert set_option(shard, 28, 1) == rx._lib.RTX_ERR_INVALID

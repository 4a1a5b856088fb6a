"""The taxon profile of a run, accumulated on the device (rtx_index_profile_*, rtx_profile.hip): clade, direct and conf_sum per node and the
totals, held for equality (np.array_equal) against checks.profile_expected -- the numpy restatement of the definition in
include/raxtax_hip.h -- on the Result that the same classify call returned.  The rows themselves are held against the oracle by the rest
of the suite; what is under test here is the accumulation: every kind of query, the edges of a wave, a ragged and deep tree, runs that are
repeated or abandoned, several handles, and that nothing changes while no profile is open."""
import ctypes as C

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import checks, synth
from test_gpu_mixed_lengths import _concat, _long_read
from test_gpu_nearest import _DUPS, revcomp
from test_profile_cpu import LINEAGES, make_tree

pytestmark = pytest.mark.gpu


def _expected(index, res, cutoff, override_ok):
    ids, off = index.device_exact_matches()
    return checks.profile_expected(index.tree.nodes(), res, off, ids, cutoff, override_ok)


def _assert_same(prof, want, what):
    for name, w in zip(("clade", "direct", "conf_sum", "totals"), want[:4]):
        g = getattr(prof, name)
        assert np.array_equal(g, w), f"{what}: {name} differs at {np.nonzero(g != w)[0][:8]}: device {g[g != w][:8]}, expected {w[g != w][:8]}"


def _assert_invariants(nodes, prof):
    assert prof.clade[0] == 0 and prof.direct[0] == 0 and prof.conf_sum[0] == 0
    assert int(prof.direct.sum()) == int(prof.totals[1]) and int(prof.totals[1:].sum()) == int(prof.totals[0])
    kids = np.zeros(len(prof.clade), np.uint64)
    np.add.at(kids, nodes["parent"][1:].astype(np.int64), prof.clade[1:])
    assert np.array_equal(prof.clade[1:], (prof.direct + kids)[1:])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. small database, every kind of query
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    db = synth.make_db(2000)
    L = db.length
    seq_bytes = db.seq_bytes.copy()
    refs = seq_bytes.reshape(db.n, L)
    for src, dst in _DUPS:
        refs[dst] = refs[src]
    qs = synth.make_queries(db, 64, seed=5)
    far = synth.make_queries(db, 32, seed=9, mu_q=0.25, exact_frac=0.0)
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
             revcomp(ref[:200]), ref[:200].copy(),
             _long_read(rng, db, 1500), revcomp(_long_read(rng, db, 2500)),
             refs[100].copy(), revcomp(refs[555]), refs[0].copy(), refs[1999].copy(),   # the duplicated references themselves: several exact matches
             refs[300].copy(), revcomp(refs[301]), revcomp(refs[1200])]                 # references with one exact match, given in either orientation
    seqs += [far.seq(i).copy() for i in range(far.n)]
    tree = rx.Tree.new_flat(db.lineages, seq_bytes, db.seq_off)
    return tree, seqs


@pytest.mark.parametrize("skip", [False, True], ids=["override", "skip"])
@pytest.mark.parametrize("strand", ["plus", "both"])
def test_small_database_every_category(small, strand, skip):
    tree, seqs = small
    bases, off = _concat(seqs)
    nodes = tree.nodes()
    index = rx.Index(tree, strand=strand)
    for cutoff in (1, 80, 100):
        index.profile_begin(cutoff / 100, skip_exact_matches=skip)
        res = index.classify(bases, off, skip_exact_matches=skip)
        prof = index.profile_read()
        want = _expected(index, res, cutoff, not skip)
        seen = want[4]
        print(f"{strand}, skip {skip}, cutoff {cutoff}: totals {prof.totals.tolist()}, {int((prof.clade > 0).sum())} nodes, {seen}")
        assert (prof.cutoff, prof.flags) == (cutoff, 1 if skip else 0) and int(prof.totals[0]) == len(seqs)
        _assert_same(prof, want, f"{strand}, skip {skip}, cutoff {cutoff}")
        _assert_invariants(nodes, prof)
        if cutoff == 80:   # every kind of query is in the expectation: the comparison above is not a comparison of zeros
            assert seen["several_exact"] >= 1 and seen["l_zero"] >= 1 and seen["l_partial"] >= 1 and seen["l_full"] >= 1 and seen["not_ok"] >= 1, seen
            assert (seen["override"] >= 1) == (not skip), seen
            if strand == "both" and not skip:
                ids, xoff = index.device_exact_matches()
                one = np.diff(xoff.astype(np.int64)) == 1
                minus = (res.strand == 1) & one & (res.status == 0) & (np.diff(res.row_off.astype(np.int64)) > 0)
                assert minus.any(), "no minus-strand query with an override"
        index.profile_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the edges of a wave
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wave_edges():
    db = synth.make_db(2000)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 130, seed=21)
    index = rx.Index(tree)
    index.profile_begin(0.8)
    batches = [(f"{n} queries", [qs.seq(i) for i in range(n)]) for n in (1, 63, 64, 65, 130)]
    batches.append(("130 copies of one read", [qs.seq(3)] * 130))          # every lane holds the same path
    for what, seqs in batches:
        bases, off = _concat(seqs)
        index.profile_reset()
        res = index.classify(bases, off)
        prof = index.profile_read()
        _assert_same(prof, _expected(index, res, 80, True), what)
        assert int(prof.totals[0]) == len(seqs)
    assert int(prof.clade.max()) == int(prof.totals[1]) == 130 and int((prof.clade > 0).sum()) <= 6    # (one path: at most its six levels)
    index.profile_end()
    # 64 reads from 64 different top-level clades: every lane of the wave holds a different path
    wide = synth.make_db(1280, fanouts=(64, 1, 1, 1, 1, 2))
    assert len({l.split(",")[0] for l in wide.lineages}) == 64
    wtree = rx.Tree.new_flat(wide.lineages, wide.seq_bytes, wide.seq_off)
    first = {}
    for i, l in enumerate(wide.lineages):
        first.setdefault(l.split(",")[0], i)
    rng = np.random.default_rng(22)
    seqs = []
    for i in first.values():
        s = wide.seq(i).copy()
        at = rng.integers(0, len(s), 4)
        s[at] = (1 << rng.integers(0, 4, 4)).astype(np.uint8)
        seqs.append(s)
    bases, off = _concat(seqs)
    windex = rx.Index(wtree)
    windex.profile_begin(0.5)
    res = windex.classify(bases, off)
    prof = windex.profile_read()
    want = _expected(windex, res, 50, True)
    _assert_same(prof, want, "64 top-level clades")
    nodes = wtree.nodes()
    top = np.nonzero(nodes["parent"] == 0)[0]
    assert len(top) == 64 and int((prof.clade[top] > 0).sum()) >= 60, prof.clade[top]   # (the lanes really are on different nodes)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a ragged and deep tree
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ragged_and_deep_tree():
    tree, seqs = make_tree()
    bases, off = _concat(seqs)
    nodes = tree.nodes()
    index = rx.Index(tree)
    for raw in (False, True):   # with the override every reference lands on its own Taxon node with 100s; under raw_confidence its own row counts
        index.profile_begin(0.8, raw_confidence=raw)
        res = index.classify(bases, off)
        prof = index.profile_read()
        want = _expected(index, res, 80, not raw)
        _assert_same(prof, want, f"raw {raw}")
        _assert_invariants(nodes, prof)
        assert want[4]["override"] == (0 if raw else len(LINEAGES))
        if not raw:
            ends = np.nonzero(prof.direct)[0]   # A, B,b1, B,b2 (two references share that leaf), the two C leaves, the 32nd level of D
            assert int(prof.clade.sum()) == 1 + 3 * 2 + 2 * 5 + 32 and len(ends) == 6 and int(prof.direct.sum()) == 7 and int(prof.direct.max()) == 2
            assert np.array_equal(prof.conf_sum, prof.clade * np.uint64(100))
        index.profile_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. no double counting: repeated runs, sub-batches, chunks, abandoned run-aheads, a second download
# ---------------------------------------------------------------------------------------------------------------------------------
_EDGES = (0, 8191, 8192, 49151, 49152, 49999)


@pytest.fixture(scope="module")
def pruned():
    db = synth.make_db(50_000)   # 7 tiles: pruned, records path and dense epilogues
    qs = synth.make_queries(db, 2000, seed=7)
    far = synth.make_queries(db, 96, seed=11, mu_q=0.25, exact_frac=0.0)
    rng = np.random.default_rng(12)
    lost = [revcomp(qs.seq(i)) for i in range(24)] + [(1 << rng.integers(0, 4, db.length)).astype(np.uint8) for _ in range(8)]
    seqs = [qs.seq(i) for i in range(2000)] + [db.seq(r).copy() for r in _EDGES] + [far.seq(i) for i in range(far.n)] + lost
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    return tree, seqs


def test_no_double_counting(pruned):
    tree, seqs = pruned
    n = len(seqs)
    bases, off = _concat(seqs)
    # (a) a fresh handle: its first run is repeated while its buffers find their size; the profile holds the batch once
    index = rx.Index(tree)
    index.profile_begin(0.8)
    res = index.classify(bases, off)
    a = index.profile_read()
    want = _expected(index, res, 80, True)
    classes = index.batch_classes()
    print(f"{n} queries, classes {classes}, totals {a.totals.tolist()}, {want[4]}")
    assert any(c["prune"] for c in classes)
    assert int(a.totals[0]) == n
    _assert_same(a, want, "fresh handle")
    assert want[4]["l_zero"] > 0 and want[4]["l_full"] > 0 and want[4]["override"] > 0
    # (b) four or more sub-batches
    small = rx.Index(tree, sub_batch=512)
    small.profile_begin(0.8)
    small.classify(bases, off)
    assert small.sub_batch_size() <= 512 and n > 3 * 512
    _assert_same(small.profile_read(), want, "sub-batches of 512")
    # (c) the host mirror in one chunk and in two chunks with run-ahead, (d) with every second run-ahead abandoned
    # (on the handle with sub-batches of 512: a chunk needs two sub-batches for the next one to be enqueued ahead of its end)
    index = small
    queries = [(f"q{i}", s) for i, s in enumerate(seqs)]
    for what, chunk, aid in (("one chunk", n, 0), ("two chunks", (n + 1) // 2, 0), ("four chunks, run-aheads abandoned", (n + 3) // 4, 2)):
        index.profile_reset()
        ahead0, retry0 = index.run_ahead_stats
        if aid:
            rx._lib.check(index._lib.rtx_index_set_option(index._h, 23, aid))
        rx.raxtax(queries, index, False, False, chunk, lambda *args: None, False)
        if aid:
            rx._lib.check(index._lib.rtx_index_set_option(index._h, 23, 0))
        ahead, retry = index.run_ahead_stats
        if chunk < n:
            assert ahead > ahead0, f"{what}: no chunk was enqueued ahead"
        if aid:
            assert retry > retry0, f"{what}: no run-ahead was abandoned"
        _assert_same(index.profile_read(), want, what)
    # a second read returns the same values; reset gives zeros
    again = index.profile_read()
    _assert_same(again, want, "second read")
    index.profile_reset()
    z = index.profile_read()
    assert not z.clade.any() and not z.direct.any() and not z.conf_sum.any() and not z.totals.any()
    # a second download of one run adds nothing
    index.upload(bases, off)
    index.run()
    index.download()
    once = index.profile_read()
    index.download()
    _assert_same(index.profile_read(), (once.clade, once.direct, once.conf_sum, once.totals), "second download")
    _assert_same(once, want, "staged interface")
    index.profile_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. several handles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_several_handles(small):
    tree, seqs = small
    bases, off = _concat(seqs)
    a, b = rx.Index(tree), rx.Index(tree)
    res = a.classify(bases, off)
    want = _expected(a, res, 80, True)
    queries = [(f"q{i}", s) for i, s in enumerate(seqs)]
    a.profile_begin(0.8)
    with pytest.raises(rx.RtxError) as e:      # one handle has a profile open, the other has none
        rx.raxtax(queries, [a, b], False, False, 32, lambda *args: None, False)
    assert e.value.code == rx._lib.RTX_ERR_INVALID
    b.profile_begin(0.8)
    with pytest.raises(rx.RtxError) as e:      # the profiles' flags are not the call's
        rx.raxtax(queries, [a, b], True, False, 32, lambda *args: None, False)
    assert e.value.code == rx._lib.RTX_ERR_INVALID
    assert not a.profile_read().totals.any() and not b.profile_read().totals.any()   # (a refused call adds nothing)
    rx.raxtax(queries, [a, b], False, False, 32, lambda *args: None, False)
    pa, pb = a.profile_read(), b.profile_read()
    assert int(pa.totals[0]) > 0 and int(pb.totals[0]) > 0 and int(pa.totals[0] + pb.totals[0]) == len(seqs)
    _assert_same(rx.profile_merge([pa, pb]), want, "two handles")
    a.profile_end()
    b.profile_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. off means off
# ---------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(small):
    tree, seqs = small
    bases, off = _concat(seqs)

    def life(kind):
        """One handle from creation to destruction, two batches; `ended` has a profile open over the first one.  One handle at a time: the
        workspace of a handle is sized against the HBM that is free when its batch is uploaded."""
        ix = rx.Index(tree)
        if kind == "ended":
            ix.profile_begin(0.8)
        ix.classify(bases, off)
        if kind == "ended":
            assert int(ix.profile_read().totals[0]) == len(seqs)
            ix.profile_end()
        return ix.classify(bases, off), ix.workspace_bytes, ix.device_bytes

    plain = life("plain")
    for kind in ("never", "ended"):
        other = life(kind)
        for f in ("t", "status", "global_signal", "row_off", "row_lineage", "row_node", "row_depth", "row_conf", "row_local_signal", "peak", "strand"):
            assert np.array_equal(getattr(plain[0], f), getattr(other[0], f)), (kind, f)
        assert other[1:] == plain[1:], (kind, other[1:], plain[1:])
    never, ended = rx.Index(tree), rx.Index(tree)
    ended.profile_begin(0.8)
    ended.profile_end()
    view = rx._lib.ProfileView()
    for ix in (never, ended):
        assert ix._lib.rtx_index_profile_read(ix._h, C.byref(view)) == rx._lib.RTX_ERR_STATE
        assert ix._lib.rtx_index_profile_reset(ix._h) == rx._lib.RTX_ERR_STATE and ix._lib.rtx_index_profile_end(ix._h) == rx._lib.RTX_ERR_STATE
    for cutoff in (0, 101):
        assert never._lib.rtx_index_profile_begin(never._h, cutoff, 0) == rx._lib.RTX_ERR_INVALID
    assert never._lib.rtx_index_profile_begin(never._h, 80, 4) == rx._lib.RTX_ERR_INVALID      # (no flag of a profile)
    never.profile_begin(1.0)
    assert never._lib.rtx_index_profile_begin(never._h, 80, 0) == rx._lib.RTX_ERR_STATE        # open already
    never.profile_end()
    from raxtax_amd.sharded import ShardIndex, shard_cuts
    shard = ShardIndex(tree, 0, shard_cuts(tree.num_tips, 2))
    assert shard._lib.rtx_index_profile_begin(shard._h, 80, 0) == rx._lib.RTX_ERR_INVALID

"""Dereplication on the device (rtx_derep.hip) and its use by the host mirror (RTX_OPT_DEREP).  The expected map everywhere is the first
index of each bytes(seq), computed with a Python dict; the runs through rx.raxtax under the option are held for equality against the same
runs without it: the same sender calls, the same hit tuples, the same profile.  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from test_gpu_mixed_lengths import _long_read
from test_gpu_nearest import _DUPS, revcomp

pytestmark = pytest.mark.gpu


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(0, np.uint8)])
    return flat, off


def first_index(seqs):
    """rep[q] = the first query with the bytes of q; the number of distinct sequences."""
    seen, rep = {}, np.zeros(len(seqs), np.uint32)
    for q, s in enumerate(seqs):
        rep[q] = seen.setdefault(bytes(np.asarray(s, np.uint8)), q)
    return rep, len(seen)


def random_seq(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


def check(d, seqs, what):
    bases, off = concat(seqs)
    rep = d.run(bases, off)
    want, n_unique = first_index(seqs)
    bad = np.nonzero(rep != want)[0]
    assert len(bad) == 0, f"{what}: rep differs at {bad[:8]}: device {rep[bad[:8]]}, expected {want[bad[:8]]}"
    assert d.n_unique == n_unique, (what, d.n_unique, n_unique)
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 - 3. word and nibble edges, forced collisions, raw bytes
# ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 658)


@pytest.fixture(scope="module")
def edges():
    rng = np.random.default_rng(31)
    base = {n: random_seq(rng, n) for n in LENGTHS}
    base[65][5] = 2
    for short, long in ((8, 9), (16, 17), (512, 513)):   # one sequence a prefix of another
        base[short] = base[long][:short].copy()
    distinct = [base[n] for n in LENGTHS]
    for n in (1, 9, 17, 65, 513, 658):   # pairs that differ only in the first base, and only in the last
        first, last = base[n].copy(), base[n].copy()
        first[0] = 1 if first[0] != 1 else 2
        last[-1] = 4 if last[-1] != 4 else 8
        distinct += [first] + ([last] if n > 1 else [])
    plain, amb = base[65].copy(), base[65].copy()   # an ambiguity code against a plain base
    plain[5], amb[5] = 1, 15
    distinct += [plain, amb]
    distinct += [random_seq(rng, 658) for _ in range(40 - len(distinct))]
    assert len({bytes(s) for s in distinct}) == len(distinct) == 40
    picks = list(rng.integers(0, len(distinct), 290))
    picks += [0, 0, 0, 0] + list(range(len(distinct)))        # several empty queries; every sequence at least once
    picks = [int(x) for x in rng.permutation(picks)]
    picks = [14] + picks + [14]                                # copies at both ends of the batch
    seqs = [distinct[i] for i in picks]
    _, off = concat(seqs)
    dup = np.array([picks.index(p) != i for i, p in enumerate(picks)])
    starts = off[:-1].astype(np.int64)
    assert (starts[dup] % 2 == 0).any() and (starts[dup] % 2 == 1).any()   # copies start on even and on odd nibbles
    assert sum(len(s) == 0 for s in seqs) >= 4 and 300 <= len(seqs) <= 340
    return seqs


def test_word_and_nibble_edges(edges):
    rep = check(rx.Derep(), edges, "edges")
    assert rep[-1] == 0 and rep[0] == 0


def test_forced_collisions(edges):
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_DEREP_HASH_MASK, 3))
    try:
        check(rx.Derep(), edges, "hash of two bits")
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_DEREP_HASH_MASK, 0))
    check(rx.Derep(), edges, "mask restored")


def test_raw_bytes(edges):
    seqs = [s.copy() for s in edges]
    k = next(i for i, s in enumerate(seqs) if len(s) == 658)
    seqs[k][100] = 0x20    # no code of the parser: the batch travels as raw bytes
    bases, _ = concat(seqs)
    assert _lib.load().rtx_pack_bases(_lib.ptr(bases, _lib.u8p), len(bases), _lib.ptr(np.zeros(len(bases), np.uint8), _lib.u8p)) == 0
    check(rx.Derep(), seqs, "raw bytes")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. larger, and buffer reuse; 5. contention
# ---------------------------------------------------------------------------------------------------------------------------------
def test_larger_and_buffer_reuse():
    rng = np.random.default_rng(32)
    pool = rng.integers(0, 4, (3000, 658))
    src = rng.integers(0, 2000, 1000)
    pool[2000:] = pool[src]                                   # a third are single-base variants of another
    at = rng.integers(0, 658, 1000)
    pool[np.arange(2000, 3000), at] = (pool[src, at] + 1) % 4
    pool = (1 << pool).astype(np.uint8)
    picks = rng.integers(0, 3000, 20_000)
    d = rx.Derep()
    check(d, list(pool[picks]), "20 000 queries from 3 000 sequences")
    assert d.n_unique > 2900
    check(d, list(pool[rng.integers(0, 100, 500)]), "500 queries on the same object")   # buffers reused, the table cleared
    check(d, [], "no query")
    assert d.n_unique == 0


def test_contention():
    rng = np.random.default_rng(33)
    d = rx.Derep()
    one = random_seq(rng, 658)
    rep = check(d, [one] * 5000, "5 000 copies of one sequence")   # every wave meets one slot and one atomicMin
    assert d.n_unique == 1 and not rep.any()
    check(d, list((1 << rng.integers(0, 4, (5000, 658))).astype(np.uint8)), "5 000 distinct sequences")
    assert d.n_unique == 5000


def test_invalid_arguments():
    d = rx.Derep()
    with pytest.raises(rx.RtxError) as e:
        d.run(np.zeros(16, np.uint8), np.array([0, 8, 4, 16], np.uint64))   # base_off not monotone
    assert e.value.code == _lib.RTX_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. end to end through rx.raxtax; 7. the profile
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run600():
    """600 queries with unique labels from 150 distinct reads: one read in a stretch of 64 copies (queries 128 .. 191: a whole chunk of 64),
    64 distinct reads in a stretch (320 .. 383: a chunk without copies), the rest shuffled with multiplicities 1 .. 20."""
    db = synth.make_db(2000)
    L = db.length
    seq_bytes = db.seq_bytes.copy()
    refs = seq_bytes.reshape(db.n, L)
    for src, dst in _DUPS:
        refs[dst] = refs[src]
    rng = np.random.default_rng(34)
    qs = synth.make_queries(db, 132, seed=35)
    amb = refs[40].copy()
    amb[[10, 100, 300]] = [5, 15, 10]
    bad = refs[41].copy()
    bad[200] = 0x20
    special = [refs[17][:7].copy(),                                   # shorter than 8 bases: status not OK
               amb, bad,
               refs[300].copy(), revcomp(refs[301]),                  # one exact match, in either orientation
               refs[100].copy(), revcomp(refs[555]), refs[0].copy(),  # several exact matches
               _long_read(rng, db, 1500)]
    reads = [qs.seq(i).copy() for i in range(132)]
    for i in range(0, 132, 5):
        reads[i] = revcomp(reads[i])                                  # some reads given as reverse complements
    reads = reads[:1] + special + reads[1:]                           # (read 0, a reverse complement, is the one with 64 copies; the special reads are in the stretch of distinct ones)
    reads += [reads[20][:200 + k].copy() for k in range(150 - len(reads))]
    # a handful of synthetic queries may coincide (exact copies of one reference): keep the first of each
    reads = list({bytes(r): r for r in reads}.values())
    while len(reads) < 150:
        reads.append(random_seq(rng, L))
    assert len({bytes(r) for r in reads}) == len(reads) == 150
    mult = np.zeros(150, np.int64)
    mult[65:] = 1
    while mult.sum() < 600 - 128:
        j = int(rng.integers(1, 149))
        if mult[j] < 19:
            mult[j] += 1
    pool = [int(x) for x in rng.permutation(np.repeat(np.arange(150), mult))]
    order = pool[:128] + [0] * 64 + pool[128:256] + list(range(1, 65)) + pool[256:]
    assert len(order) == 600 and len(set(order)) == 150
    counts = np.bincount(order, minlength=150)
    assert counts[0] == 64 and counts[149] == 1 and counts[1:].max() <= 20
    queries = [(f"read{i:03d};copy_of={r}", reads[r]) for i, r in enumerate(order)]
    tree = rx.Tree.new_flat(db.lineages, seq_bytes, db.seq_off)
    return tree, queries


def _distinct_per_chunk(queries, chunk):
    n = len(queries)
    chunk = chunk if 0 < chunk <= n else n
    return sum(len({bytes(s) for _, s in queries[a:a + chunk]}) for a in range(0, n, chunk))


def _through_raxtax(index, queries, skip, chunk):
    sent, hits = [], []
    rx.raxtax(queries, index, skip, False, chunk, lambda label, out, tsv: sent.append((label, out, tsv)), True,
              hit=lambda *a: hits.append(a))
    return sent, hits


@pytest.mark.parametrize("skip", [False, True], ids=["override", "skip"])
@pytest.mark.parametrize("strand", ["plus", "both"])
def test_end_to_end(run600, strand, skip):
    tree, queries = run600
    plain = rx.Index(tree, strand=strand, nearest=True)
    derep = rx.Index(tree, strand=strand, nearest=True, derep=True)
    for chunk in (0, 64, 257):
        want_sent, want_hits = _through_raxtax(plain, queries, skip, chunk)
        assert rx.raxtax_last_derep() == (0, 0, 0.0)
        got_sent, got_hits = _through_raxtax(derep, queries, skip, chunk)
        n_q, n_u, busy = rx.raxtax_last_derep()
        print(f"{strand}, skip {skip}, chunk {chunk}: {n_q} queries, {n_u} distinct, stage busy {busy * 1e3:.2f} ms, {len(want_sent)} messages")
        assert (n_q, n_u) == (600, _distinct_per_chunk(queries, chunk)) and n_u < n_q and busy > 0
        assert 580 <= len(want_sent) < 600 and len(want_hits) == len(want_sent)      # (the short read, up to 20 times, has no message)
        assert [s[0] for s in got_sent] == [s[0] for s in want_sent]
        assert got_sent == want_sent
        assert got_hits == want_hits
    if strand == "both":
        assert any(h[1] == 1 for h in want_hits) and any(h[1] == 0 for h in want_hits)
    if not skip:
        assert any(h[4] != rx.NO_REF and h[5] >= 2 for h in want_hits)   # (the copies of a duplicated reference tie)


def test_handles_must_agree(run600):
    tree, queries = run600
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(queries, [rx.Index(tree, derep=True), rx.Index(tree)], False, False, 64, lambda *a: None, False)
    assert e.value.code == _lib.RTX_ERR_INVALID


def _profile(index, queries, skip, chunk):
    index.profile_begin(0.8, skip_exact_matches=skip)
    rx.raxtax(queries, index, skip, False, chunk, lambda *a: None, False)
    p = index.profile_read()
    index.profile_end()
    return p


def _assert_profiles_equal(a, b, what):
    for f in ("clade", "direct", "conf_sum", "totals"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("strand", ["plus", "both"])
def test_profile_counts_every_copy(run600, strand):
    tree, queries = run600
    plain, derep = rx.Index(tree, strand=strand), rx.Index(tree, strand=strand, derep=True)
    for skip in (False, True):
        for chunk in (0, 64, 257):
            want = _profile(plain, queries, skip, chunk)
            got = _profile(derep, queries, skip, chunk)
            assert int(want.totals[0]) == 600 and int(want.totals[1]) > 100 and int(want.totals[3]) >= 1
            _assert_profiles_equal(got, want, (strand, skip, chunk))


@pytest.mark.parametrize("strand", ["plus", "both"])
def test_weights_alone(run600, strand):
    tree, queries = run600
    reads = list({bytes(s): s for _, s in queries}.values())
    rng = np.random.default_rng(36)
    w = rng.integers(0, 6, len(reads)).astype(np.uint32)
    assert set(w.tolist()) == set(range(6))
    index = rx.Index(tree, strand=strand)
    index.profile_begin(0.8)
    index.classify(*concat([r for r, k in zip(reads, w) for _ in range(int(k))]))
    want = index.profile_read()
    assert int(want.totals[0]) == int(w.sum())
    index.profile_reset()
    bases, off = concat(reads)
    index.prefetch_weights(w)
    index.classify(bases, off)
    _assert_profiles_equal(index.profile_read(), want, "weights 0 .. 5")
    # the weights belonged to that batch alone
    index.profile_reset()
    index.classify(bases, off)
    unweighted = index.profile_read()
    assert int(unweighted.totals[0]) == len(reads)
    # a weights array of the wrong length is dropped
    index.profile_reset()
    index.prefetch_weights(w[:-1])
    index.classify(bases, off)
    _assert_profiles_equal(index.profile_read(), unweighted, "wrong length")
    index.profile_end()

"""Primer trimming on the device (rtx_trim.hip) and its use by the host mirror (rtx_index_set_primers).  The expected values everywhere come
from the numpy recurrence of tests/trim_common.py; the runs through rx.raxtax with primers set are held for equality, message for message
and byte for byte, against runs without the option on the reads cut at the recurrence's positions.  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from trim_common import NO_DIST, concat, trim_many

pytestmark = pytest.mark.gpu

A, Cc, G, T = 1, 2, 4, 8


def random_seq(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


def other(b):
    return {1: 2, 2: 4, 4: 8, 8: 1}[int(b)]


def edits(p):
    """A substitution, an insertion and a deletion at the first, a middle and the last base of p."""
    out = []
    for pos in (0, len(p) // 2, len(p) - 1):
        s = p.copy()
        s[pos] = other(s[pos])
        out += [s, np.insert(p, pos, other(p[pos])), np.delete(p, pos)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2. rx.Trim against the recurrence
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage():
    """Four patterns, two per end: 20 codes (2 errors) and 64 codes (6 errors, degenerate: W, Y, N), and 257 reads."""
    rng = np.random.default_rng(41)
    f20, r20 = random_seq(rng, 20), random_seq(rng, 20)
    f64, r64 = random_seq(rng, 64), random_seq(rng, 64)
    f64i, r64i = f64.copy(), r64.copy()            # an instance of each degenerate pattern
    f64[[3, 30, 63]] = [f64[3] | T | A, 15, f64[63] | Cc]
    r64[[0, 31, 60]] = [15, r64[31] | G, r64[60] | T | Cc]
    pats = [rx.TrimPrimer(f20, rx.TRIM_5P, 2), rx.TrimPrimer(f64, rx.TRIM_5P, 6), rx.TrimPrimer(r20, rx.TRIM_3P, 2), rx.TrimPrimer(r64, rx.TRIM_3P, 6)]
    amp = lambda n=658: random_seq(rng, n)
    reads = [np.concatenate([f20, amp(), r20]),                       # n = 1 is this one
             np.zeros(0, np.uint8), amp(1), amp(20), f20.copy(), r20.copy(), amp(),
             np.concatenate([f64i, amp(), r64i]), np.concatenate([f20, amp(5000 - 40), r20]),
             np.concatenate([f20, r20]),                              # a bare primer pair: nothing is left
             np.concatenate([f20[:15], r20[5:]]), np.concatenate([f20, r20[10:]]), np.concatenate([f64i[:40], r64i[30:]]),   # so short that the cuts overlap
             np.concatenate([f20, f20, amp(), r20, r20]),             # a primer twice: only the outer copy goes
             np.concatenate([amp(3), f20, amp(), r20, amp(4)])]       # a few bases outside the primers go with them
    # the 20-mer and a 64-mer that begins with it, both without an error: equal errors, the lower index wins (and cuts less)
    g64 = np.concatenate([f20, random_seq(rng, 44)])
    tie_pats = [rx.TrimPrimer(g64, rx.TRIM_5P, 6), rx.TrimPrimer(f20, rx.TRIM_5P, 2)]
    reads.append(np.concatenate([g64, amp()]))
    for e5 in edits(f20):
        reads.append(np.concatenate([e5, amp(), r20]))
    for e3 in edits(r20):
        reads.append(np.concatenate([f20, amp(300), e3]))
    for e5, e3 in zip(edits(f64i), edits(r64i)):
        reads.append(np.concatenate([e5, amp(), e3]))
    for endpos in (15, 16, 17, 31, 32, 33):                          # primers ending at these positions from either end
        reads.append(np.concatenate([amp(endpos - 12), f20[8:], amp(100), r20[:12], amp(endpos - 12)]))
        if endpos > 20:
            reads.append(np.concatenate([amp(endpos - 20), f20, amp(100), r20, amp(endpos - 20)]))
    for byte in (15, 5, 0, 0x20, 200):                               # ambiguity codes and bytes that are no code, in the primers and behind them
        s = np.concatenate([f20, amp(), r20])
        s[[7, 25, len(s) - 4]] = byte
        reads.append(s)
    three = f20.copy()
    three[[4, 9, 15]] = [other(three[4]), other(three[9]), other(three[15])]
    reads.append(np.concatenate([three, np.full(100, 200, np.uint8), r20]))   # three errors where two are allowed: not found
    reads.append(np.concatenate([np.full(4, f20[0], np.uint8), f20, amp()]))
    while len(reads) < 257:                                          # the bulk: amplicons with 0 .. 3 edits in either primer, some without one
        k = len(reads)
        a, b = (f20, r20) if k % 3 else (f64i, r64i)
        a, b = list(a), list(b)
        for s in (a, b):
            for _ in range(int(rng.integers(0, 4))):
                pos = int(rng.integers(0, len(s)))
                op = int(rng.integers(0, 3))
                if op == 0:
                    s[pos] = int(rng.choice([1, 2, 4, 8, 15, 0x20]))
                elif op == 1:
                    s.insert(pos, int(rng.choice([1, 2, 4, 8])))
                else:
                    del s[pos]
        parts = [np.array(a, np.uint8)] * (k % 7 != 0) + [amp(int(rng.integers(100, 700)))] + [np.array(b, np.uint8)] * (k % 5 != 0)
        reads.append(np.concatenate(parts))
    assert len(reads) == 257
    want = trim_many(pats, reads)
    return pats, reads, want, tie_pats


def _assert_equal(got, want, what):
    for name, g, w in zip(("lo", "hi", "hit"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:8]}: device {np.asarray(g)[bad[:8]]}, expected {np.asarray(w)[bad[:8]]}"


def test_trim_run_equals_the_recurrence(stage):
    pats, reads, want, tie_pats = stage
    lo, hi, hit = want
    found5, found3 = (hit & 0xFF) != 0xFF, ((hit >> 16) & 0xFF) != 0xFF
    assert 150 < found5.sum() < 257 and 150 < found3.sum() < 257 and (lo == hi).sum() >= 4     # the expectation itself has every kind in it
    assert set(np.unique(hit & 0xFF)) == {0, 1, 0xFF} and set(np.unique((hit >> 16) & 0xFF)) == {2, 3, 0xFF}
    assert (((hit >> 8) & 0xFF) == 2).any() and ((hit >> 24) == 3).any()
    t = rx.Trim(0, pats)
    for n in (257, 1, 63, 64, 65):                                   # (the buffers of the largest batch are reused by the smaller ones)
        got = t.run(*concat(reads[:n]))
        _assert_equal(got, [w[:n] for w in want], f"{n} reads")
    got = t.run(*concat(reads[::-1]))
    _assert_equal(got, [w[::-1] for w in want], "the batch reversed: a read's values do not depend on its batch")
    got = t.run(*concat([]))
    assert all(len(g) == 0 for g in got)
    assert t.kernel_ms() >= 0.0
    # two patterns of one end found with equal errors: the lower index, though the other would cut more
    tie_want = trim_many(tie_pats, reads)
    k = next(i for i, r in enumerate(reads) if len(r) == 64 + 658)
    assert tie_want[0][k] == 64 and tie_want[2][k] & 0xFFFF == 0
    _assert_equal(rx.Trim(0, tie_pats).run(*concat(reads)), tie_want, "equal errors")
    tie_swapped = trim_many(tie_pats[::-1], reads)
    assert tie_swapped[0][k] == 20 and tie_swapped[2][k] & 0xFFFF == 0
    _assert_equal(rx.Trim(0, tie_pats[::-1]).run(*concat(reads)), tie_swapped, "equal errors, the list reversed")
    # one end alone
    _assert_equal(rx.Trim(0, pats[2:]).run(*concat(reads)), trim_many(pats[2:], reads), "3' patterns alone")
    _assert_equal(rx.Trim(0, pats[:1]).run(*concat(reads)), trim_many(pats[:1], reads), "one 5' pattern alone")


def test_windows_of_every_size(stage):
    pats, reads, _, _ = stage
    for w in (1, 19, 20, 31, 32, 33, 64, 255, 256):
        ps = [rx.TrimPrimer(pats[0].codes, 0, 2, w), rx.TrimPrimer(pats[2].codes, 1, 2, w), rx.TrimPrimer(pats[3].codes, 1, 63, min(256, w + 7))]
        _assert_equal(rx.Trim(0, ps).run(*concat(reads[:70])), trim_many(ps, reads[:70]), f"window {w}")


def test_the_order_of_the_list_changes_the_indices_alone(stage):
    pats, reads, want, _ = stage
    perm = [2, 0, 3, 1]                                              # the order within either end stays: the same pattern wins every tie
    got = rx.Trim(0, [pats[i] for i in perm]).run(*concat(reads))
    new_of = {old: new for new, old in enumerate(perm)}
    new_of[0xFF] = 0xFF
    lo, hi, hit = want
    mapped = np.array([new_of[int(h) & 0xFF] | (int(h) & 0xFF00) | new_of[(int(h) >> 16) & 0xFF] << 16 | (int(h) & 0xFF000000) for h in hit], np.uint32)
    _assert_equal(got, (lo, hi, mapped), "permuted list")
    swapped = [pats[1], pats[0], pats[3], pats[2]]                   # the order within the ends changes as well: against the recurrence
    _assert_equal(rx.Trim(0, swapped).run(*concat(reads)), trim_many(swapped, reads), "ends swapped within")


def test_invalid_arguments(stage):
    pats = stage[0]
    t = rx.Trim(0, pats)
    with pytest.raises(rx.RtxError) as e:
        t.run(np.zeros(16, np.uint8), np.array([0, 8, 4, 16], np.uint64))   # base_off not monotone
    assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.Trim(0, [rx.TrimPrimer(np.array([1, 0, 2], np.uint8), 0, 0)])
    assert e.value.code == _lib.RTX_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 - 5. end to end through rx.raxtax
# ---------------------------------------------------------------------------------------------------------------------------------
FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"      # LCO1490 / HCO2198 with two degenerate positions each


def revcomp(s):
    return rx.api.revcomp(np.asarray(s, np.uint8))


@pytest.fixture(scope="module")
def run280():
    """280 queries against 400 references: primer + amplicon + revcomp(primer), some with a primer error, some without primers (queries 64 ..
    127: a whole chunk of 64 in which nothing is found), a bare primer pair, copies; every second one also as its reverse complement."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 200, seed=43)
    rng = np.random.default_rng(44)
    inst = lambda text: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(text)], np.uint8)
    reads = []
    for i in range(280):
        amplicon = qs.seq(i % 200).copy()
        if i % 10 == 3:
            amplicon = db.seq(int(rng.integers(0, db.n))).copy()     # exact matches of a reference, once trimmed
        f, r = inst(FWD), revcomp(inst(REV))
        if i % 4 == 1:                                               # one primer error
            pos = int(rng.integers(0, len(f)))
            f = [np.delete(f, pos), np.insert(f, pos, 1), np.concatenate([f[:pos], [other(f[pos])], f[pos + 1:]])][i % 3].astype(np.uint8)
        if i % 4 == 2:
            pos = int(rng.integers(0, len(r)))
            r = np.concatenate([r[:pos], [other(r[pos])], r[pos + 1:]]).astype(np.uint8)
        if 64 <= i < 128 or i % 9 == 0:
            read = amplicon                                          # no primers
        elif i % 11 == 0:
            read = np.concatenate([f, amplicon])                     # one end only
        else:
            read = np.concatenate([f, amplicon, r])
        reads.append(read)
    reads[5] = np.concatenate([inst(FWD), revcomp(inst(REV))])       # a bare primer pair
    reads[6] = np.zeros(0, np.uint8)
    for i in range(200, 280, 2):
        reads[i] = reads[i - 190].copy()                             # copies (of reads in other chunks and in the same one)
    reads[131] = reads[130].copy()
    # reads[17] and reads[19]: one amplicon whose primers differ by a sequencing error -- copies only once trimmed
    reads[19] = reads[17].copy()
    reads[19][3] = other(reads[19][3])
    queries = [(f"read{i:03d}", r) for i, r in enumerate(reads)]
    flipped = [(l, revcomp(r) if i % 2 else r) for i, (l, r) in enumerate(queries)]
    return tree, queries, flipped


def _through_raxtax(index, queries, chunk, trim=False, align=False):
    sent, trims, aligns = [], [], []
    kw = {}
    if trim:
        kw["trim"] = lambda *a: trims.append(a)
    if align:
        kw["align"] = lambda *a: aligns.append(a)
    rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: sent.append((label, out, tsv)), True, **kw)
    return sent, trims, aligns


@pytest.mark.parametrize("mode", ["plain", "derep", "both_strands", "identity", "device_text"])
def test_end_to_end(run280, mode):
    tree, queries, flipped = run280
    both = mode == "both_strands"
    given = flipped if both else queries
    pats = rx.primer_patterns((FWD, REV), error_percent=8, both_strands=both)
    assert [p.max_errors for p in pats] == [2, 2] * (2 if both else 1)
    lo, hi, hit = trim_many(pats, [r for _, r in given])
    expected = [(l, r[int(a):int(b)].copy()) for (l, r), a, b in zip(given, lo, hi)]   # from the recurrence's cuts, not from the construction
    n5, n3 = int(((hit & 0xFF) != 0xFF).sum()), int((((hit >> 16) & 0xFF) != 0xFF).sum())
    emptied = int(((lo == hi) & (np.array([len(r) for _, r in given]) > 0)).sum())
    assert 150 < n5 < 230 and 150 < n3 < 230 and emptied == 1
    assert bytes(expected[17][1]) == bytes(expected[19][1]) and bytes(given[17][1]) != bytes(given[19][1])
    if both:
        assert set(np.unique(hit & 0xFF)) == {0, 2, 0xFF} and set(np.unique((hit >> 16) & 0xFF)) == {1, 3, 0xFF}
    kw = dict(derep=mode == "derep", strand="both" if both else "plus", identity=mode == "identity", device_text=mode == "device_text")
    plain, trimming = rx.Index(tree, **kw), rx.Index(tree, primers=pats, **kw)
    assert trimming.primers == len(pats) and plain.primers == 0
    ident = mode == "identity"
    for chunk in (0, 64, 100):
        want_sent, no_trims, want_aligns = _through_raxtax(plain, expected, chunk, trim=True, align=ident)
        assert rx.raxtax_last_trim() == (0, 0, 0, 0, 0.0)
        assert no_trims == [(l, len(r), 0, len(r), 0xFF | 0xFF << 16) for l, r in expected]      # without primers: nothing found, per query
        got_sent, got_trims, got_aligns = _through_raxtax(trimming, given, chunk, trim=True, align=ident)
        n_q, w5, w3, n_e, busy = rx.raxtax_last_trim()
        print(f"{mode}, chunk {chunk}: {n_q} queries, {w5} / {w3} with a 5' / 3' primer, {n_e} left empty, stage busy {busy * 1e3:.2f} ms, {len(want_sent)} messages")
        assert (n_q, w5, w3, n_e) == (280, n5, n3, emptied) and busy > 0
        assert 270 <= len(want_sent) <= 278                                                       # (the bare primer pair and the empty read have no message)
        assert [s[0] for s in got_sent] == [s[0] for s in want_sent]
        assert got_sent == want_sent
        assert got_trims == [(l, len(r), int(a), int(b), int(h)) for (l, r), a, b, h in zip(given, lo, hi, hit)]
        if ident:
            assert got_aligns == want_aligns and len(got_aligns) == len(got_sent)
            span = {l: int(b) - int(a) for (l, _), a, b in zip(given, lo, hi)}
            assert all(a[7] == span[a[0]] for a in got_aligns)                                   # query_len is that of the trimmed read
            assert any(a[6] == 0 for a in got_aligns) and any(0 < a[6] < NO_DIST for a in got_aligns)
    if mode == "derep":
        q, u, _ = rx.raxtax_last_derep()
        assert q == 280 and u < 280
    # the same handle with the primers cleared is the plain handle again; set again, it trims again
    trimming.set_primers([])
    assert trimming.primers == 0
    assert _through_raxtax(trimming, expected, 64)[0] == want_sent_of(plain, expected)
    trimming.set_primers(pats)
    assert _through_raxtax(trimming, given, 64)[0] == want_sent


def want_sent_of(index, queries):
    return _through_raxtax(index, queries, 64)[0]


def test_classify_ignores_the_primers(run280):
    tree, queries, _ = run280
    pats = rx.primer_patterns((FWD, REV), error_percent=8)
    bases, off = concat([r for _, r in queries[:40]])
    a = rx.Index(tree).classify(bases, off)
    b = rx.Index(tree, primers=pats).classify(bases, off)
    assert np.array_equal(a.t, b.t) and np.array_equal(a.row_lineage, b.row_lineage) and np.array_equal(a.row_conf, b.row_conf)


def test_handles_must_hold_the_same_list(run280):
    tree, queries, _ = run280
    pats = rx.primer_patterns((FWD, REV), error_percent=8)
    fewer = rx.primer_patterns((FWD, REV), error_percent=4)
    for other_list in ([], pats[:1], fewer):
        with pytest.raises(rx.RtxError) as e:
            rx.raxtax(queries, [rx.Index(tree, primers=pats), rx.Index(tree, primers=other_list)], False, False, 64, lambda *a: None, False)
        assert e.value.code == _lib.RTX_ERR_INVALID
    sent = []
    rx.raxtax(queries, [rx.Index(tree, primers=pats), rx.Index(tree, primers=pats)], False, False, 64, lambda *a: sent.append(a), True)
    assert sent == _through_raxtax(rx.Index(tree, primers=pats), queries, 64)[0]


def test_set_and_cleared_primers_leave_a_fresh_handle(run280):
    tree, queries, _ = run280
    pats = rx.primer_patterns((FWD, REV), error_percent=8)
    fresh = _through_raxtax(rx.Index(tree), queries, 64, trim=True)
    used = rx.Index(tree, primers=pats)
    _through_raxtax(used, queries, 64)
    assert rx.raxtax_last_trim()[0] == 280
    used.set_primers([])
    assert _through_raxtax(used, queries, 64, trim=True) == fresh
    assert rx.raxtax_last_trim() == (0, 0, 0, 0, 0.0)

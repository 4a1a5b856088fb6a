"""The quality filter in the host mirror (rtx_index_set_quality, rtx_raxtax_multi_ex5), end to end through rx.raxtax: the messages, callbacks
and profile of a handle with the setting are held for equality, element for element, against a handle without it on the reads cut and
emptied at the positions of the plain-integer restatement (tests/qual_common.py).  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from qual_common import concat, qual_ref
from trim_common import trim_many

pytestmark = pytest.mark.gpu

FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"
PARAMS = rx.QualParams(trunc_qual=2, max_ee=2.0, min_len=32, max_ns=4)
MODES = ["plain", "derep", "both_strands", "identity", "device_text", "primers", "profile"]


def revcomp(s):
    return rx.api.revcomp(np.asarray(s, np.uint8))


@pytest.fixture(scope="module")
def run280():
    """280 reads with quality strings against 400 references.  Q falls along a read; most reads have a base of Q 2 somewhere in their last
    third (cut there), some are bad all along (max_ee), some hold N bases, one is cut to fewer than min_len bases, one has no bases;
    reads 64 .. 127 are good to the end (a whole chunk of 64 that passes as it came); copies of reads with other quality strings.
    Every read also with primers around it."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 200, seed=53, n_frac=0.0)
    rng = np.random.default_rng(54)
    inst = lambda text: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(text)], np.uint8)

    def quality(n, i):
        q = np.clip(40 - (np.arange(n) * 12) // max(n, 1) - rng.integers(0, 4, n), 3, 41)
        if 64 <= i < 128:
            return (33 + q).astype(np.uint8)
        if i % 7 == 2:
            q = rng.integers(3, 12, n)                               # bad all along: expected errors far above 2
        elif n:
            q[int(rng.integers(2 * n // 3, n))] = int(rng.integers(0, 3))    # cut in front of this base
        if i % 13 == 5 and n:
            q[int(rng.integers(0, 20))] = 1                          # fewer than min_len bases are left
        return (33 + q).astype(np.uint8)

    reads, quals = [], []
    for i in range(280):
        amplicon = qs.seq(i % 200).copy()
        if i % 10 == 3:
            amplicon = db.seq(int(rng.integers(0, db.n))).copy()     # exact matches of a reference where the filter leaves it whole
        if i % 17 == 4 and not 64 <= i < 128:
            amplicon[rng.integers(0, len(amplicon) // 2, 6)] = 15    # N bases
        reads.append(amplicon)
        quals.append(quality(len(amplicon), i))
    reads[6], quals[6] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    for i in range(200, 280, 2):                                     # copies, with quality strings of their own: not always copies afterwards
        reads[i] = reads[i - 190].copy()
        quals[i] = quality(len(reads[i]), i) if i % 4 else quals[i - 190].copy()
    queries = [(f"read{i:03d}", r, q) for i, (r, q) in enumerate(zip(reads, quals))]
    flipped = [(l, revcomp(r) if i % 2 else r, q[::-1].copy() if i % 2 else q) for i, (l, r, q) in enumerate(queries)]
    with_primers = []
    for i, (l, r, q) in enumerate(queries):
        f, b = (inst(FWD), revcomp(inst(REV))) if i % 9 and not 64 <= i < 128 else (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        qf, qb = np.full(len(f), 33 + 38, np.uint8), np.full(len(b), 33 + 8, np.uint8)
        with_primers.append((l, np.concatenate([f, r, b]).astype(np.uint8), np.concatenate([qf, q, qb]).astype(np.uint8)))
    return tree, queries, flipped, with_primers


def _through_raxtax(index, queries, chunk, **want):
    got = {"sent": []}
    kw = {}
    for name in ("trim", "align", "qual"):
        if want.get(name):
            got[name] = []
            kw[name] = (lambda box: lambda *a: box.append(a))(got[name])
    rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: got["sent"].append((label, out, tsv)), True, **kw)
    return got


def _expect(given, pats):
    """Per query: the range the primers leave (the whole read without), the restatement's (hi, ee, verdict) on it, and the read downstream."""
    if pats:
        lo, hi, hit = trim_many(pats, [r for _, r, _ in given])
    else:
        lo, hi, hit = np.zeros(len(given), np.uint32), np.array([len(r) for _, r, _ in given], np.uint32), np.full(len(given), 0xFF | 0xFF << 16, np.uint32)
    rows = [qual_ref(PARAMS, r, q, int(a), int(b)) for (_, r, q), a, b in zip(given, lo, hi)]
    reads = [(l, r[int(a):(int(a) if v else h)].copy()) for (l, r, _), a, (h, _, v) in zip(given, lo, rows)]
    return lo, hi, hit, rows, reads


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end(run280, mode):
    tree, queries, flipped, with_primers = run280
    given = {"both_strands": flipped, "primers": with_primers}.get(mode, queries)
    pats = rx.primer_patterns((FWD, REV), error_percent=8) if mode == "primers" else []
    lo, hi, hit, rows, expected = _expect(given, pats)
    verdicts = np.array([v for _, _, v in rows])
    n_pass = int((verdicts == 0).sum())
    n_trunc = int(sum(1 for (h, _, v), b in zip(rows, hi) if v == 0 and h < int(b)))
    reasons = [int(((verdicts >> b) & 1).sum()) for b in range(7)]
    assert 150 < n_pass < 260 and n_trunc > 100 and reasons[2] >= 5 and reasons[4] >= 3 and reasons[5] >= 20 and reasons[0] == 0
    assert all(v == 0 and h == len(r) for (_, r, _), (h, _, v) in zip(given[64:128], rows[64:128])) or mode == "primers"   # a chunk of 64 that passes as it came
    kw = dict(derep=mode == "derep", strand="both" if mode == "both_strands" else "plus", identity=mode == "identity", device_text=mode == "device_text")
    if pats:
        kw["primers"] = pats
    plain, filtering = rx.Index(tree, **kw), rx.Index(tree, quality=PARAMS, **kw)
    assert filtering.quality == PARAMS and plain.quality is None
    if pats:
        plain.set_primers([])                                       # the expected reads are cut already
    ident = mode == "identity"
    for chunk in (0, 64, 100):
        if mode == "profile":
            plain.profile_begin(0.8)
            filtering.profile_begin(0.8)
        want = _through_raxtax(plain, expected, chunk, trim=True, qual=True, align=ident)
        assert rx.raxtax_last_qual() == (0, 0, 0, [0] * 7, 0.0)     # the call before holds zeros
        assert want["qual"] == [(l, len(r), 0, len(r), 0, 0) for l, r in expected]     # without a filter: the whole read, per query
        got = _through_raxtax(filtering, given, chunk, trim=True, qual=True, align=ident)
        n_q, passed, truncated, why, busy = rx.raxtax_last_qual()
        print(f"{mode}, chunk {chunk}: {n_q} queries, {passed} passed, {truncated} of them cut short, reasons {why}, stage busy {busy * 1e3:.2f} ms, {len(want['sent'])} messages")
        assert (n_q, passed, truncated, why) == (280, n_pass, n_trunc, reasons) and busy > 0
        assert [s[0] for s in got["sent"]] == [s[0] for s in want["sent"]]
        assert got["sent"] == want["sent"]
        assert len(got["sent"]) <= n_pass and len(got["sent"]) > n_pass - 10               # a discarded read has no message
        assert got["qual"] == [(l, len(r), int(a), int(h), int(e), int(v)) for (l, r, _), a, (h, e, v) in zip(given, lo, rows)]
        assert got["trim"] == [(l, len(r), int(a), int(b), int(w)) for (l, r, _), a, b, w in zip(given, lo, hi, hit)]
        if ident:
            assert got["align"] == want["align"] and len(got["align"]) == len(got["sent"])
            span = {l: len(r) for l, r in expected}
            assert all(a[7] == span[a[0]] for a in got["align"])    # query_len is that of the kept bases
        if mode == "profile":
            a, b = plain.profile_read(), filtering.profile_read()
            assert np.array_equal(a.clade, b.clade) and np.array_equal(a.direct, b.direct) and np.array_equal(a.conf_sum, b.conf_sum)
            assert np.array_equal(a.totals, b.totals) and int(a.totals[0]) > 0
            plain.profile_end()
            filtering.profile_end()
    if mode == "derep":
        q, u, _ = rx.raxtax_last_derep()
        assert q == 280 and u < 280
    # the same handle with the setting cleared is the plain handle again; set again, it filters again
    filtering.set_quality(None)
    assert filtering.quality is None
    two = [(l, r) for l, r in expected]
    assert _through_raxtax(filtering, two, 64)["sent"] == _through_raxtax(plain, two, 64)["sent"]
    filtering.set_quality(PARAMS)
    assert _through_raxtax(filtering, given, 64)["sent"] == want["sent"]


def test_a_setting_needs_quality_strings_and_quals_alone_are_ignored(run280):
    tree, queries, _, _ = run280
    bare = [(l, r) for l, r, _ in queries]
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(bare, rx.Index(tree, quality=PARAMS), False, False, 64, lambda *a: None, False)
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert _through_raxtax(rx.Index(tree), queries, 64, qual=True)["sent"] == _through_raxtax(rx.Index(tree), bare, 64)["sent"]
    assert rx.raxtax_last_qual() == (0, 0, 0, [0] * 7, 0.0)
    off = rx.Index(tree, quality=rx.QualParams())                    # parameters that are entirely off are no filter
    assert off.quality is None
    for p in (rx.QualParams(ascii_base=50, max_ee=1.0), rx.QualParams(trunc_qual=94), rx.QualParams(max_ee=float("nan"))):
        with pytest.raises(rx.RtxError) as e:
            rx.Index(tree, quality=p)
        assert e.value.code == _lib.RTX_ERR_INVALID


def test_classify_ignores_the_setting(run280):
    tree, queries, _, _ = run280
    bases, off = concat([r for _, r, _ in queries[:40]])
    a = rx.Index(tree).classify(bases, off)
    b = rx.Index(tree, quality=PARAMS).classify(bases, off)
    assert np.array_equal(a.t, b.t) and np.array_equal(a.row_lineage, b.row_lineage) and np.array_equal(a.row_conf, b.row_conf)


def test_handles_must_hold_the_same_setting(run280):
    tree, queries, _, _ = run280
    for other in (None, rx.QualParams(trunc_qual=2, max_ee=2.5, min_len=32, max_ns=4), rx.QualParams(ascii_base=64, trunc_qual=2, max_ee=2.0, min_len=32, max_ns=4)):
        with pytest.raises(rx.RtxError) as e:
            rx.raxtax(queries, [rx.Index(tree, quality=PARAMS), rx.Index(tree, quality=other)], False, False, 64, lambda *a: None, False)
        assert e.value.code == _lib.RTX_ERR_INVALID
    sent = []
    rx.raxtax(queries, [rx.Index(tree, quality=PARAMS), rx.Index(tree, quality=PARAMS)], False, False, 64, lambda *a: sent.append(a), True)
    assert sent == _through_raxtax(rx.Index(tree, quality=PARAMS), queries, 64)["sent"]


def test_set_and_cleared_setting_leaves_a_fresh_handle(run280):
    tree, queries, _, _ = run280
    bare = [(l, r) for l, r, _ in queries]
    fresh = _through_raxtax(rx.Index(tree), bare, 64, trim=True, qual=True)
    used = rx.Index(tree, quality=PARAMS)
    _through_raxtax(used, queries, 64)
    assert rx.raxtax_last_qual()[0] == 280
    used.set_quality(None)
    assert _through_raxtax(used, bare, 64, trim=True, qual=True) == fresh
    assert rx.raxtax_last_qual() == (0, 0, 0, [0] * 7, 0.0)
    used.set_quality(PARAMS)
    used.set_quality(rx.QualParams())
    assert used.quality is None

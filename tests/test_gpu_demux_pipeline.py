"""The demultiplexing stage in front of the host mirror (rtx_index_set_tags, rtx_raxtax_multi_ex7).  A run of rx.raxtax on a handle with tags
is held for equality, message for message and byte for byte, against a run of a handle without them on the reads cut at the positions the
numpy restatement of tests/demux_common.py gives, the reads that are not assigned replaced by the empty read.  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from demux_common import AMBIGUOUS, NO_TAG, NO_TAG3, NO_TAG5, NONE, OK, UNKNOWN_PAIR, concat, demux_ref, other, spaced_tags

pytestmark = pytest.mark.gpu

FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"      # LCO1490 / HCO2198 with two degenerate positions each
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}
PARAMS = rx.DemuxParams(1, 2)
N_SAMPLES = 5                                                            # s3 owns a line and receives no read


def revcomp(s):
    return rx.api.revcomp(np.asarray(s, np.uint8))


def text(codes):
    return "".join(LETTER[int(c)] for c in codes)


@pytest.fixture(scope="module")
def run280():
    """280 queries against 400 references: tag + primer + amplicon + revcomp(primer) + tag for the samples of a sheet of six lines (s2 owns two of
    them, s3 receives nothing), some with a spacer, some with a substitution in a tag, and reads of every failing verdict; every second one
    also as its reverse complement."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 200, seed=43)
    rng = np.random.default_rng(46)
    ftag, rtag = spaced_tags(rng, 6, 8), spaced_tags(rng, 6, 8)           # rtag: as on the oligo
    owner = ["s0", "s1", "s2", "s2", "s3", "s4"]
    sheet = "# sample\tfwd\trev\n" + "".join(f"{owner[k]}\t{text(ftag[k])}\t{text(rtag[k])}\n" for k in range(6))
    inst = lambda t: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(t)], np.uint8)
    reads = []
    for i in range(280):
        amplicon = qs.seq(i % 200).copy()
        if i % 10 == 3:
            amplicon = db.seq(int(rng.integers(0, db.n))).copy()         # exact matches of a reference, once cut
        k = (0, 1, 2, 3, 5)[i % 5]
        t5, t3 = ftag[k].copy(), revcomp(rtag[k])
        if i % 6 == 1 or i % 12 == 4:                                    # (odd and even reads: either end, once every second read is flipped)
            t5[int(rng.integers(0, 8))] = 0x20                           # one position that matches nothing
        if i % 6 == 2:
            p = int(rng.integers(0, 8))
            t3[p] = other(t3[p])
        sp5, sp3 = (1 << rng.integers(0, 4, i % 3)).astype(np.uint8), (1 << rng.integers(0, 4, (i // 3) % 3)).astype(np.uint8)
        body = np.concatenate([inst(FWD), amplicon, revcomp(inst(REV))])
        if 64 <= i < 128:
            read = body                                                  # a whole chunk of 64 without tags
        elif i % 17 == 0:
            read = np.concatenate([sp5, t5, body])                       # no 3' tag
        elif i % 19 == 0:
            read = np.concatenate([sp5, ftag[0], body, revcomp(rtag[1]), sp3])        # both found, no such pair
        elif i % 23 == 0:
            tie = ftag[0].copy()
            tie[ftag[0] != ftag[1]] = 15                                 # N wherever two tags differ: both at distance 0
            read = np.concatenate([tie, body, t3, sp3])
        else:
            read = np.concatenate([sp5, t5, body, t3, sp3])
        reads.append(read)
    reads[5] = np.concatenate([ftag[0], revcomp(rtag[0])])               # a bare tag pair: assigned, and nothing is left
    reads[6] = np.zeros(0, np.uint8)
    for i in range(200, 280, 2):
        reads[i] = reads[i - 190].copy()                                 # copies
    queries = [(f"read{i:03d}", r) for i, r in enumerate(reads)]
    flipped = [(l, revcomp(r) if i % 2 else r) for i, (l, r) in enumerate(queries)]
    return tree, queries, flipped, sheet


def restated(sheet, given, both):
    """(tags, pairs, names, the restatement's five arrays, the reads as they go on)"""
    tags, pairs, names = rx.sample_sheet(sheet, both_orientations=both)
    sample, lo, hi, hit, info = demux_ref([(t.codes, t.end) for t in tags], pairs, PARAMS.max_mismatches, PARAMS.max_offset, [r for _, r in given])[:5]
    ok = (info & 0xFF) == OK
    cut = [(l, r[int(a):int(b)].copy() if k else r[:0].copy()) for (l, r), a, b, k in zip(given, lo, hi, ok)]
    return tags, pairs, names, (sample, lo, hi, hit, info), cut


def through(index, queries, chunk, **cbs):
    sent = []
    got = {k: [] for k in cbs}
    kw = {k: (lambda *a, k=k: got[k].append(a)) for k in cbs}
    rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: sent.append((label, out, tsv)), True, **kw)
    return sent, got


@pytest.mark.parametrize("mode", ["plain", "primers", "identity", "derep", "device_text", "both_strands"])
def test_end_to_end(run280, mode):
    tree, queries, flipped, sheet = run280
    both = mode == "both_strands"
    given = flipped if both else queries
    tags, pairs, names, want, cut = restated(sheet, given, both)
    sample, lo, hi, hit, info = want
    verdict = info & 0xFF
    assert names == ["s0", "s1", "s2", "s3", "s4"]
    assert set(np.unique(verdict)) == {OK, NO_TAG5, NO_TAG3, AMBIGUOUS, UNKNOWN_PAIR}                  # the expectation has every verdict in it ...
    assert set(np.unique(sample)) == {0, 1, 2, 4, NONE} and 150 < (verdict == OK).sum() < 215          # ... and every sample but s3
    assert (((info >> 8) & 0xFF) == 1).any() and (((info >> 16) & 0xFF) == 1).any() and ((info >> 28) == 2).any()
    primers = rx.primer_patterns((FWD, REV), error_percent=8, both_strands=both) if mode != "plain" else None
    kw = dict(derep=mode == "derep", strand="both" if both else "plus", identity=mode == "identity", device_text=mode == "device_text", primers=primers)
    plain, tagged = rx.Index(tree, **kw), rx.Index(tree, tags=(tags, pairs, PARAMS), **kw)
    assert tagged.tags == len(tags) and plain.tags == 0
    cbs = dict(demux=True, trim=True)
    if mode == "identity":
        cbs["align"] = True
    for chunk in (0, 64, 100):
        want_sent, want_cb = through(plain, cut, chunk, **cbs)
        assert rx.raxtax_last_demux() == (0, 0, [0] * 5, 0.0)
        assert want_cb["demux"] == [(l, len(r), NONE, 0, len(r), NO_TAG | NO_TAG << 16, 0) for l, r in cut]      # without tags: nothing, per query
        got_sent, got_cb = through(tagged, given, chunk, **cbs)
        n_q, n_ok, reasons, busy = rx.raxtax_last_demux()
        print(f"{mode}, chunk {chunk}: {n_q} queries, {n_ok} assigned, verdicts {reasons}, stage busy {busy * 1e3:.2f} ms, {len(want_sent)} messages")
        assert (n_q, n_ok, reasons) == (280, int((verdict == OK).sum()), [int((verdict == v).sum()) for v in range(5)]) and busy > 0
        assert 100 < len(want_sent) < 215
        assert [s[0] for s in got_sent] == [s[0] for s in want_sent]
        assert got_sent == want_sent
        assert got_cb["demux"] == [(l, len(r), int(s), int(a), int(b), int(h), int(f)) for (l, r), s, a, b, h, f in zip(given, sample, lo, hi, hit, info)]
        assert got_cb["trim"] == want_cb["trim"]                         # the callbacks behind it speak of the cut read
        if mode != "plain":
            assert sum(1 for t in got_cb["trim"] if t[4] & 0xFF != 0xFF) > 100
        if mode == "identity":
            assert got_cb["align"] == want_cb["align"] and len(got_cb["align"]) == len(got_sent)
    # the same handle with the tags cleared is the plain handle again; set again, it demultiplexes again
    tagged.set_tags([])
    assert tagged.tags == 0
    assert through(tagged, cut, 64)[0] == want_sent
    tagged.set_tags(tags, pairs, PARAMS)
    assert through(tagged, given, 64)[0] == want_sent


def test_classify_ignores_the_tags(run280):
    tree, queries, _, sheet = run280
    tags, pairs, _ = rx.sample_sheet(sheet)
    bases, off = concat([r for _, r in queries[:40]])
    a = rx.Index(tree).classify(bases, off)
    b = rx.Index(tree, tags=(tags, pairs, PARAMS)).classify(bases, off)
    assert np.array_equal(a.t, b.t) and np.array_equal(a.row_lineage, b.row_lineage) and np.array_equal(a.row_conf, b.row_conf)


def test_handles_must_hold_the_same_list(run280):
    tree, queries, _, sheet = run280
    tags, pairs, _ = rx.sample_sheet(sheet)
    for other_list in (None, (tags[:2], pairs[:1], PARAMS), (tags, pairs[:-1], PARAMS), (tags, pairs, rx.DemuxParams(0, 2))):
        with pytest.raises(rx.RtxError) as e:
            rx.raxtax(queries, [rx.Index(tree, tags=(tags, pairs, PARAMS)), rx.Index(tree, tags=other_list)], False, False, 64, lambda *a: None, False)
        assert e.value.code == _lib.RTX_ERR_INVALID
    sent = []
    rx.raxtax(queries, [rx.Index(tree, tags=(tags, pairs, PARAMS)), rx.Index(tree, tags=(tags, pairs, PARAMS))], False, False, 64, lambda *a: sent.append(a), True)
    assert sent == through(rx.Index(tree, tags=(tags, pairs, PARAMS)), queries, 64)[0]


def test_set_and_cleared_tags_leave_a_fresh_handle(run280):
    tree, queries, _, sheet = run280
    tags, pairs, _ = rx.sample_sheet(sheet)
    fresh = through(rx.Index(tree), queries, 64, demux=True)
    used = rx.Index(tree, tags=(tags, pairs, PARAMS))
    through(used, queries, 64)
    assert rx.raxtax_last_demux()[0] == 280
    used.set_tags([])
    assert through(used, queries, 64, demux=True) == fresh
    assert rx.raxtax_last_demux() == (0, 0, [0] * 5, 0.0)


def test_sample_profile_through_the_mirror(run280):
    """The per-sample counters of a run with tags equal the plain profiles of each sample's cut reads run alone."""
    tree, queries, _, sheet = run280
    tags, pairs, names, want, cut = restated(sheet, queries, False)
    sample = want[0]
    tagged = rx.Index(tree, tags=(tags, pairs, PARAMS))
    tagged.profile_begin(0.8, n_samples=N_SAMPLES)
    through(tagged, queries, 64)
    got = tagged.profile_read_samples()
    glob = tagged.profile_read()
    plain = rx.Index(tree)
    for k in range(N_SAMPLES):
        plain.profile_begin(0.8)
        mine = [c for c, s in zip(cut, sample) if s == k]
        if mine:
            through(plain, mine, 64)
        alone = plain.profile_read()
        plain.profile_end()
        assert np.array_equal(got.direct[k], alone.direct) and np.array_equal(got.totals[k], alone.totals), f"sample {k}"
        assert bool(alone.totals.any()) == (k != 3)
    assert int(glob.totals[0]) == 280 and int(got.totals[:, 0].sum()) == int((sample != NONE).sum())
    table = rx.sample_table_text(tree, names, got)
    assert table.split("\n")[5] == "depth\ttaxon\tlineage\t" + "\t".join(names)
    tagged.profile_end()
    # dereplication beside tags: allowed alone, refused with a profile open
    both = rx.Index(tree, tags=(tags, pairs, PARAMS), derep=True)
    both.profile_begin(0.8, n_samples=N_SAMPLES)
    with pytest.raises(rx.RtxError, match="RTX_OPT_DEREP") as e:
        through(both, queries, 64)
    assert e.value.code == _lib.RTX_ERR_INVALID
    both.profile_end()

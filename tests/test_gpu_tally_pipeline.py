"""The distinct-read table as the last stage of the read front (rtx_index_set_tally): a run of rx.raxtax on a handle with a tally sends what
the run without it sends, and the table is the Python dict over the reads that went on to be classified -- plain, under RTX_OPT_DEREP,
behind a chimera check that flags reads, and per sample behind the tags.  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth
import chimera_common as cc
from demux_common import spaced_tags
from tally_common import expected_table

pytestmark = pytest.mark.gpu

CHUNK = 16
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}


def revcomp(s):
    return rx.api.revcomp(np.asarray(s, np.uint8))


@pytest.fixture(scope="module")
def rnd():
    """The small random database of the chimera pipeline test, and 70 queries in chunks of 16: plain reads with copies inside a chunk and across
    chunks, planted chimeras (one of them twice), an empty read and one of seven bases."""
    db = synth.make_db(2000)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    chim, _ = cc.planted_chimeras(db)
    qs = synth.make_queries(db, 300)
    plain = [qs.seq(i).copy() for i in range(40)]
    seqs = plain[:20] + chim[:10] + [plain[3].copy(), chim[5].copy(), np.zeros(0, np.uint8), plain[7][:7].copy()] + plain[20:40] + [plain[i].copy() for i in (0, 3, 3, 17, 21, 39)] + \
        [plain[25].copy()] * 10
    assert len(seqs) == 70 and len({bytes(s) for s in seqs}) == 52            # (the empty read among them: 51 entries)
    return dict(tree=tree, seqs=seqs, queries=[(f"q{i}", s) for i, s in enumerate(seqs)])


def through(index, queries, **cbs):
    sent = []
    rx.raxtax(queries, index, False, False, CHUNK, lambda label, out, tsv: sent.append((label, out, tsv)), True, **cbs)
    return sent


def assert_table(table, want):
    got = table.as_dict()
    assert got.keys() == want.keys() and got == want
    assert table.totals == {"reads": sum(map(sum, want.values())), "entries": len(want), "overflow_reads": 0}


@pytest.mark.parametrize("derep", (False, True), ids=("plain", "derep"))
def test_table_of_a_run_and_two_calls_accumulate(rnd, derep):
    queries, seqs = rnd["queries"], rnd["seqs"]
    base = through(rx.Index(rnd["tree"], derep=derep), queries)
    assert rx.raxtax_last_tally() == (0, 0, 0, 0.0)
    tally = rx.Tally(initial_entries=8, initial_bytes=1024)
    index = rx.Index(rnd["tree"], derep=derep, tally=tally)
    assert index.tally is tally
    assert through(index, queries) == base and len(base) == 68          # the sender calls of the run without it
    want = expected_table(seqs)                                           # copies count as reads, with and without RTX_OPT_DEREP
    assert len(want) == 51 and max(v[0] for v in want.values()) == 11
    assert_table(tally.read(), want)
    n_q, counted, added, busy = rx.raxtax_last_tally()
    assert (n_q, counted, added) == (70, 69, 51) and busy > 0
    # a second call on the same object: every count doubles, no entry is added
    assert through(index, queries) == base
    assert_table(tally.read(), {k: (2 * v[0],) for k, v in want.items()})
    assert rx.raxtax_last_tally()[:3] == (70, 69, 0)
    # switched off, the handle is the plain handle again and the object keeps what it has
    index.set_tally(None)
    assert through(index, queries) == base and rx.raxtax_last_tally()[:3] == (0, 0, 0)
    assert tally.read().totals["reads"] == 138


@pytest.mark.parametrize("derep", (False, True), ids=("plain", "derep"))
def test_flagged_chimeras_are_not_counted(rnd, derep):
    queries, seqs = rnd["queries"], rnd["seqs"]
    tally = rx.Tally()
    index = rx.Index(rnd["tree"], derep=derep, chimera=rx.ChimeraParams(), tally=tally)
    flags = {}
    sent = through(index, queries, chimera=lambda label, rec: flags.__setitem__(label, int(rec["flag"])))
    flagged = [i for i in range(70) if flags[f"q{i}"]]
    assert 8 <= len(flagged) <= 12 and flags["q25"] and flags["q31"] and not flags["q30"]
    assert [m[0] for m in sent] == [f"q{i}" for i in range(70) if i not in flagged and len(seqs[i]) >= 8]
    want = expected_table(seqs, None, [0 if i in flagged else 1 for i in range(70)])
    assert bytes(seqs[25]) not in want and len(want) == 51 - len({bytes(seqs[i]) for i in flagged})
    assert_table(tally.read(), want)
    assert rx.raxtax_last_tally()[:3] == (70, 69 - len(flagged), len(want))


def test_per_sample_cells_behind_the_tags(rnd):
    rng = np.random.default_rng(51)
    ftag, rtag = spaced_tags(rng, 3, 8), spaced_tags(rng, 3, 8)
    text = lambda codes: "".join(LETTER[int(c)] for c in codes)
    sheet = "".join(f"s{k}\t{text(ftag[k])}\t{text(rtag[k])}\n" for k in range(3))
    tags, pairs, names = rx.sample_sheet(sheet)
    assert names == ["s0", "s1", "s2"]
    reads = []
    for i, s in enumerate(rnd["seqs"]):
        k = i % 4
        reads.append(s.copy() if k == 3 else np.concatenate([ftag[k], s, revcomp(rtag[k])]))   # every fourth read carries no tags: unassigned
    queries = [(f"q{i}", r) for i, r in enumerate(reads)]
    params = rx.DemuxParams(0, 0)
    for derep in (False, True):          # tags + derep + tally is allowed: every read counts in its own sample
        base, seen = [], {}
        rx.raxtax(queries, rx.Index(rnd["tree"], tags=(tags, pairs, params), derep=derep), False, False, CHUNK, lambda *m: base.append(m), True,
                  demux=lambda label, raw_len, sample, lo, hi, hit, info: seen.__setitem__(label, (sample, lo, hi, info & 0xFF)))
        tally = rx.Tally(samples=3)
        index = rx.Index(rnd["tree"], tags=(tags, pairs, params), derep=derep, tally=tally)
        assert through(index, queries) == base
        cut, sample, weight = [], [], []
        for i, r in enumerate(reads):
            s, lo, hi, verdict = seen[f"q{i}"]
            ok = verdict == rx.DEMUX_OK
            assert ok == (i % 4 != 3) and (not ok or (s == i % 4 and (lo, hi) == (8, len(r) - 8))) and (ok or s == rx.DEMUX_NONE)
            cut.append(r[lo:hi] if ok else r[:0])
            sample.append(s)
            weight.append(1 if ok else 0)
        want = expected_table(cut, sample, weight, 3)
        assert all(any(v[c] for v in want.values()) for c in range(3)) and any(sum(1 for c in v if c) > 1 for v in want.values())
        table = tally.read()
        assert table.columns == 3
        assert_table(table, want)
        assert rx.tally_table_text(table, names).splitlines()[0] == "#uniq\ts0\ts1\ts2"
    # the samples of the object are those of the tag list
    with pytest.raises(rx.RtxError) as e:
        through(rx.Index(rnd["tree"], tags=(tags, pairs, params), tally=rx.Tally(samples=2)), queries)
    assert "n_samples 2" in str(e.value) and "must be 3" in str(e.value)
    with pytest.raises(rx.RtxError):
        through(rx.Index(rnd["tree"], tags=(tags, pairs, params), tally=rx.Tally()), queries)


def test_two_handles_merged_equal_one(rnd):
    queries, seqs = rnd["queries"], rnd["seqs"]
    one = rx.Tally()
    base = through(rx.Index(rnd["tree"], tally=one), queries)
    a, b = rx.Tally(), rx.Tally()
    assert through([rx.Index(rnd["tree"], tally=a), rx.Index(rnd["tree"], tally=b)], queries) == base
    ta, tb = a.read(), b.read()
    # chunk c goes to handle c mod 2, and to that handle's object
    assert_table(ta, expected_table([s for i, s in enumerate(seqs) if (i // CHUNK) % 2 == 0]))
    assert_table(tb, expected_table([s for i, s in enumerate(seqs) if (i // CHUNK) % 2 == 1]))
    merged, single = rx.tally_merge([ta, tb]), one.read()
    assert [bytes(s) for s in merged.seqs] == [bytes(s) for s in single.seqs]
    assert np.array_equal(merged.counts, single.counts) and merged.totals == single.totals
    assert rx.tally_fasta(merged) == rx.tally_fasta(single) and rx.tally_fasta(single).count(">") == 51
    assert rx.raxtax_last_tally()[:3] == (70, 69, len(ta.seqs) + len(tb.seqs))

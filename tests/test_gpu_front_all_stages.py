"""Every stage of the read front in ONE call of rx.raxtax: tags, primers, quality filter, dereplication and chimera check on the same handle
(rtx_raxtax_multi_ex7).  The expectation never passes through the front of the host mirror: it is put together from the stand-alone stage
objects -- rx.Demux, rx.Trim, rx.Qual, rx.trim_apply, rx.Derep / rx.derep_plan, rx.Chimera -- in the order the mirror runs them, and the
messages are those of a plain handle on the reads that remain.  Messages byte for byte, callbacks tuple for tuple, the totals of
raxtax_last_* from the same arrays; for chunk sizes 0, 64 and 100, on one handle and on two handles of one device.  No tolerance anywhere.

The reads are those of tests/test_gpu_demux_pipeline.py (tag + primer + amplicon + revcomp(primer) + tag, every demux verdict, a bare tag
pair, the empty read) with the quality strings of tests/test_gpu_qual_pipeline.py and a few planted chimeras of tests/chimera_common.py.
Reads 64 .. 127 carry no tags: the tag stage finds nothing to cut in that chunk of 64 (lo = 0, hi = the length).  Such a read is assigned to
no sample and so goes on as the empty read; a chunk that the tag stage hands on without a copy holds empty reads alone, which
test_a_chunk_of_empty_reads_goes_on_as_it_came runs."""
import numpy as np
import pytest

import chimera_common as cc
import raxtax_amd as rx
from raxtax_amd import synth
from demux_common import AMBIGUOUS, NO_TAG3, NO_TAG5, OK, UNKNOWN_PAIR, concat, other, spaced_tags
from qual_common import TOO_SHORT

pytestmark = pytest.mark.gpu

FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"      # LCO1490 / HCO2198 with two degenerate positions each
LETTER = {1: "A", 2: "C", 4: "G", 8: "T"}
DEMUX = rx.DemuxParams(1, 2)
QUAL = rx.QualParams(trunc_qual=2, max_ee=2.0, min_len=32, max_ns=4)
CHIMERIC = (9, 27, 141, 155)                                             # reads whose amplicon is a planted chimera
N = 280


def revcomp(s):
    return rx.api.revcomp(np.asarray(s, np.uint8))


def build_inputs():
    """(db, tree, sheet, queries): 280 (label, bases, quals) triples against 400 references."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 200, seed=43, n_frac=0.0)
    rng = np.random.default_rng(46)
    ftag, rtag = spaced_tags(rng, 6, 8), spaced_tags(rng, 6, 8)           # rtag: as on the oligo
    owner = ["s0", "s1", "s2", "s2", "s3", "s4"]
    text = lambda codes: "".join(LETTER[int(c)] for c in codes)
    sheet = "# sample\tfwd\trev\n" + "".join(f"{owner[k]}\t{text(ftag[k])}\t{text(rtag[k])}\n" for k in range(6))
    inst = lambda t: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(t)], np.uint8)
    chim, _ = cc.planted_chimeras(db, n=len(CHIMERIC))

    def quality(n, i, good):
        q = np.clip(40 - (np.arange(n) * 12) // max(n, 1) - rng.integers(0, 4, n), 3, 41)
        if good:
            return (33 + q).astype(np.uint8)                             # good to the end
        if i % 7 == 2:
            q = rng.integers(3, 12, n)                                   # bad all along: expected errors far above 2
        elif n:
            q[int(rng.integers(2 * n // 3, n))] = int(rng.integers(0, 3))    # cut in front of this base
        if i % 13 == 5 and n:
            q[int(rng.integers(0, 20))] = 1                              # fewer than min_len bases are left
        return (33 + q).astype(np.uint8)

    amplicons, aquals = [], []
    for i in range(N):
        src = i - 190 if i >= 200 and i % 2 == 0 else i - 3 if i in range(132, 190, 6) else i    # copies: only once the tags are cut
        if src != i:
            amplicon = amplicons[src].copy()
        elif i in CHIMERIC:
            amplicon = chim[CHIMERIC.index(i)].copy()
        elif i % 10 == 3:
            amplicon = db.seq(int(rng.integers(0, db.n))).copy()         # exact matches of a reference, once cut
        else:
            amplicon = qs.seq(i % 200).copy()
            if i % 17 == 4 and not 64 <= i < 128:
                amplicon[rng.integers(0, len(amplicon) // 2, 6)] = 15    # N bases
        amplicons.append(amplicon)
        # (a copy with a quality string of its own is not always a copy afterwards)
        aquals.append(aquals[src].copy() if src != i and i % 4 == 0 else quality(len(amplicon), i, 64 <= i < 128 or src in CHIMERIC))
    reads, quals = [], []
    for i in range(N):
        k = (0, 1, 2, 3, 5)[i % 5]
        t5, t3 = ftag[k].copy(), revcomp(rtag[k])
        if i % 6 == 1 or i % 12 == 4:
            t5[int(rng.integers(0, 8))] = 0x20                           # one position that matches nothing
        if i % 6 == 2:
            p = int(rng.integers(0, 8))
            t3[p] = other(t3[p])
        sp5, sp3 = (1 << rng.integers(0, 4, i % 3)).astype(np.uint8), (1 << rng.integers(0, 4, (i // 3) % 3)).astype(np.uint8)
        p5, p3 = inst(FWD), revcomp(inst(REV))
        if 64 <= i < 128:
            head, tail = [p5], [p3]                                      # a whole chunk of 64 without tags
        elif i % 17 == 0:
            head, tail = [sp5, t5, p5], [p3]                             # no 3' tag
        elif i % 19 == 0:
            head, tail = [sp5, ftag[0], p5], [p3, revcomp(rtag[1]), sp3]                  # both found, no such pair
        elif i % 23 == 0:
            tie = ftag[0].copy()
            tie[ftag[0] != ftag[1]] = 15                                 # N wherever two tags differ: both at distance 0
            head, tail = [tie, p5], [p3, t3, sp3]
        else:
            head, tail = [sp5, t5, p5], [p3, t3, sp3]
        head, tail = np.concatenate(head), np.concatenate(tail)
        reads.append(np.concatenate([head, amplicons[i], tail]).astype(np.uint8))
        quals.append(np.concatenate([np.full(len(head), 33 + 38, np.uint8), aquals[i], np.full(len(tail), 33 + 8, np.uint8)]))
    reads[5] = np.concatenate([ftag[0], revcomp(rtag[0])])               # a bare tag pair: assigned, and nothing is left
    quals[5] = np.full(len(reads[5]), 33 + 38, np.uint8)
    reads[6], quals[6] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    return db, tree, sheet, [(f"read{i:03d}", r, q) for i, (r, q) in enumerate(zip(reads, quals))]


def chunks_of(n, chunk, n_handles):
    """The chunks of a call as the mirror deals them: [begin, end) each."""
    if chunk == 0 or chunk > n:
        chunk = max(1, (n + n_handles - 1) // n_handles)
    return [(a, min(a + chunk, n)) for a in range(0, n, chunk)]


@pytest.fixture(scope="module")
def front():
    """The inputs and the expectation, from the stand-alone stage objects; computed once and left unchanged."""
    db, tree, sheet, queries = build_inputs()
    tags, pairs, names = rx.sample_sheet(sheet)
    pats = rx.primer_patterns((FWD, REV), error_percent=8)
    bases, off = concat([r for _, r, _ in queries])
    qflat, _ = concat([q for _, _, q in queries])
    # 1, 2: the sample of every read; the reads without their tags, one that is not assigned empty
    sample, dlo, dhi, dhit, dinfo = rx.Demux(0, tags, pairs, DEMUX).run(bases, off)
    verdict = dinfo & 0xFF
    keep = np.where(verdict == OK, dhi, dlo)
    b1, off1 = rx.trim_apply(bases, off, dlo, keep)
    q1, _ = rx.trim_apply(qflat, off, dlo, keep)
    len1 = np.diff(off1).astype(np.int64)
    # 3, 4, 5: the primers, the quality filter on what they left, both ranges applied at once; a discarded read empty
    tlo, thi, thit = rx.Trim(0, pats).run(b1, off1)
    qhi, ee, qv = rx.Qual(0, QUAL).run(b1, q1, off1, tlo, thi)
    b2, off2 = rx.trim_apply(b1, off1, tlo, np.where(qv != 0, tlo, qhi))
    # 6, 7: the distinct reads (of the whole call: a record does not depend on the batch); a flagged one empty
    derep = rx.Derep()
    uniq, slot, _ = rx.derep_plan(derep.run(b2, off2))
    plain = rx.Index(tree)
    bu, offu = concat([b2[int(off2[u]):int(off2[u + 1])] for u in uniq])
    recs = rx.Chimera(plain).run(bu, offu)
    b3, off3 = rx.trim_apply(bu, offu, np.zeros(len(uniq), np.uint32), np.where(recs["flag"] != 0, 0, np.diff(offu)).astype(np.uint32))
    # 8: the messages of a plain handle on what remains, per query through slot
    remain = [(l, b3[int(off3[s]):int(off3[s + 1])].copy()) for (l, _, _), s in zip(queries, slot)]
    sent = []
    rx.raxtax(remain, plain, False, False, 64, lambda label, out, tsv: sent.append((label, out, tsv)), True)
    # 9: the callbacks
    cbs = dict(
        demux=[(l, len(r), int(s), int(a), int(b), int(h), int(f)) for (l, r, _), s, a, b, h, f in zip(queries, sample, dlo, dhi, dhit, dinfo)],
        trim=[(l, int(n), int(a), int(b), int(h)) for (l, _, _), n, a, b, h in zip(queries, len1, tlo, thi, thit)],
        qual=[(l, int(n), int(a), int(h), int(e), int(v)) for (l, _, _), n, a, h, e, v in zip(queries, len1, tlo, qhi, ee, qv)],
        chimera=[(l, cc.as_tuple(recs[s])) for (l, _, _), s in zip(queries, slot)])
    flag = recs["flag"][slot] != 0
    totals = dict(
        demux=(N, int((verdict == OK).sum()), [int((verdict == v).sum()) for v in range(5)]),
        trim=(N, int(((thit & 0xFF) != 0xFF).sum()), int((((thit >> 16) & 0xFF) != 0xFF).sum()), int(((len1 != 0) & (thi == tlo)).sum())),
        qual=(N, int((qv == 0).sum()), int(((qv == 0) & (qhi < thi)).sum()), [int(((qv >> b) & 1).sum()) for b in range(7)]),
        flagged=int(flag.sum()))

    def distinct(chunk, n_handles):
        """The distinct reads the handles are given: per chunk, as the dereplication works."""
        return sum(len(rx.derep_plan(derep.run(b2[int(off2[a]):int(off2[b])], off2[a:b + 1] - off2[a]))[0]) for a, b in chunks_of(N, chunk, n_handles))

    # the conditions on the inputs
    assert names == ["s0", "s1", "s2", "s3", "s4"]
    assert set(np.unique(verdict)) == {OK, NO_TAG5, NO_TAG3, AMBIGUOUS, UNKNOWN_PAIR}                  # every demux verdict
    assert (qv != 0).any() and totals["qual"][2] > 0                                                   # discarded by the filter, and cut short
    assert totals["trim"][1] > 100 and totals["trim"][2] > 100                                         # primers found
    assert 1 <= totals["flagged"] and all(flag[i] for i in CHIMERIC) and flag[144]                     # the planted chimeras, and the copy of one
    assert len(uniq) < N and distinct(64, 1) < N and distinct(100, 1) < N                              # copies, also within a chunk
    assert (dlo[64:128] == 0).all() and np.array_equal(dhi[64:128], np.diff(off)[64:128].astype(np.uint32))   # a chunk of 64 the tag stage leaves uncut
    assert len1[5] == 0 and sample[5] == 0 and len(queries[6][1]) == 0                                 # the bare tag pair and the empty read
    assert 60 < len(sent) < 215 and {m[0] for m in sent}.isdisjoint({queries[i][0] for i in np.nonzero(flag)[0]})
    return dict(tree=tree, queries=queries, tags=(tags, pairs, DEMUX), pats=pats, sent=sent, cbs=cbs, totals=totals, distinct=distinct)


def through(handles, queries, chunk):
    sent, got = [], {k: [] for k in ("demux", "trim", "qual", "chimera")}
    rx.raxtax(queries, handles, False, False, chunk, lambda label, out, tsv: sent.append((label, out, tsv)), True,
              demux=lambda *a: got["demux"].append(a), trim=lambda *a: got["trim"].append(a), qual=lambda *a: got["qual"].append(a),
              chimera=lambda label, rec: got["chimera"].append((label, cc.as_tuple(rec))))
    return sent, got


def all_stages(front):
    return rx.Index(front["tree"], tags=front["tags"], primers=front["pats"], quality=QUAL, derep=True, chimera=rx.ChimeraParams())


@pytest.mark.parametrize("n_handles", (1, 2))
def test_all_stages_in_one_call(front, n_handles):
    handles = [all_stages(front) for _ in range(n_handles)]              # two handles of one device share its stage objects
    want = front["totals"]
    for chunk in (0, 64, 100):
        sent, got = through(handles if n_handles > 1 else handles[0], front["queries"], chunk)
        assert [m[0] for m in sent] == [m[0] for m in front["sent"]]
        assert sent == front["sent"]
        for name in ("demux", "trim", "qual", "chimera"):
            assert got[name] == front["cbs"][name], name
        n_distinct = front["distinct"](chunk, n_handles)
        demux, trim, qual, derep, chim = rx.raxtax_last_demux(), rx.raxtax_last_trim(), rx.raxtax_last_qual(), rx.raxtax_last_derep(), rx.raxtax_last_chimera()
        print(f"{n_handles} handle(s), chunk {chunk}: {len(sent)} messages, {n_distinct} distinct reads, {want['flagged']} flagged; busy ms: demux {demux[-1] * 1e3:.2f}, "
              f"trim {trim[-1] * 1e3:.2f}, qual {qual[-1] * 1e3:.2f}, derep {derep[-1] * 1e3:.2f}, chimera {chim[-1] * 1e3:.2f}")
        assert demux[:-1] == want["demux"] and demux[-1] > 0
        assert trim[:-1] == want["trim"] and trim[-1] > 0
        assert qual[:-1] == want["qual"] and qual[-1] > 0
        assert derep[:-1] == (N, n_distinct) and derep[-1] > 0
        assert chim[:-1] == (N, n_distinct, want["flagged"]) and chim[-1] > 0


def test_a_chunk_of_empty_reads_goes_on_as_it_came(front):
    """64 empty reads: no stage cuts anything, the chunk reaches the handle as the caller's arrays.  Every callback speaks, nothing is sent."""
    empty = [(f"e{i}", np.zeros(0, np.uint8), np.zeros(0, np.uint8)) for i in range(64)]
    sent, got = through(all_stages(front), empty, 64)
    assert sent == []
    assert got["demux"] == [(l, 0, 0xFFFFFFFF, 0, 0, 0xFFFF | 0xFFFF << 16, NO_TAG5) for l, _, _ in empty]
    assert got["trim"] == [(l, 0, 0, 0, 0xFF | 0xFF << 16) for l, _, _ in empty]
    assert got["qual"] == [(l, 0, 0, 0, 0, TOO_SHORT) for l, _, _ in empty]                          # (min_len = 32)
    assert [r[1][0] for r in got["chimera"]] == [cc.NO_KMER] * 64
    assert rx.raxtax_last_demux()[:3] == (64, 0, [0, 64, 0, 0, 0]) and rx.raxtax_last_derep()[:2] == (64, 1) and rx.raxtax_last_chimera()[:3] == (64, 1, 0)

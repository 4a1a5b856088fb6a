"""The contaminant screen in the host mirror (rtx_index_set_screen, rtx_raxtax_multi_ex8), end to end through rx.raxtax: the messages and
callbacks of the passing reads of a handle with the setting are held for equality, element for element, against a handle without it that
is given the passing reads alone; the screen callback against the plain-Python restatement (tests/screen_common.py).  No tolerance anywhere."""
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from qual_common import qual_ref
from screen_common import NONE, World, plant, random_codes, revcomp, screen_ref
from trim_common import trim_many

pytestmark = pytest.mark.gpu

FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"
DEFAULT = rx.ScreenParams()
MODES = ["plain", "derep", "identity", "profile", "primers_quality"]


@pytest.fixture(scope="module")
def mix():
    """260 reads against 400 references: barcodes, reads cut from a 5 386-base genome in either orientation (every fourth read), copies of
    both kinds, a barcode that carries a short genome stretch (hits, but no contaminant), an empty read."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 200, seed=61, n_frac=0.0)
    rng = random.Random(62)
    world = World([random_codes(random.Random(5386), 5386), random_codes(rng, 200)])
    g = world.seqs[0]
    reads = []
    for i in range(260):
        if i % 4 == 1:
            n, at = rng.randint(150, 300), rng.randrange(0, 5000)
            r = g[at:at + n].copy()
            reads.append(revcomp(r) if i % 8 == 1 else r)
        else:
            reads.append(qs.seq(i % 200).copy())
    reads[10] = plant(reads[10].copy(), 300, g, 2000, 40)             # 25 hits among 643 windows: reported, passes
    reads[6] = np.zeros(0, np.uint8)
    for i in range(200, 260, 3):                                       # copies of barcodes and of contaminants
        reads[i] = reads[i - 190].copy()
    return tree, world, [(f"read{i:03d}", r) for i, r in enumerate(reads)]


def _through_raxtax(index, queries, chunk, **kw):
    got = {"sent": [], "events": []}
    cbs = {}
    for name in ("trim", "qual", "screen", "align"):
        got[name] = []
        cbs[name] = (lambda nm: lambda *a: (got[nm].append(a), got["events"].append((nm, a[0]))))(name)
    rx.raxtax(queries, index, False, False, chunk, lambda label, out, tsv: (got["sent"].append((label, out, tsv)), got["events"].append(("sent", label))), True, **cbs, **kw)
    return got


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end(mix, mode):
    tree, world, queries = mix
    p = DEFAULT
    kw = dict(derep=mode == "derep", identity=mode == "identity")
    given, quals, pats, qparams = queries, None, [], None
    lo = np.zeros(len(queries), np.uint32)
    keep = np.array([len(r) for _, r in queries], np.uint32)
    if mode == "primers_quality":
        # primers around every read and a quality string; in front of the forward primer of every fifth read lie 24 genome bases (9 hits):
        # they are trimmed away with the primer and must not count
        rng = np.random.default_rng(63)
        p = rx.ScreenParams(min_hits=2, min_pct=0)
        inst = lambda text: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(text)], np.uint8)
        given, quals = [], []
        for i, (l, r) in enumerate(queries):
            front = world.seqs[0][3000:3024] if i % 5 == 0 else np.zeros(0, np.uint8)
            full = np.concatenate([front, inst(FWD), r, revcomp(inst(REV))]).astype(np.uint8)
            q = np.full(len(full), 33 + 38, np.uint8)
            if i % 7 == 3 and len(r) > 100:
                q[len(front) + 25 + len(r) - 40] = 33 + 1             # the quality filter cuts 40 bases in front of the reverse primer
            given.append((l, full))
            quals.append(q)
        pats = rx.primer_patterns((FWD, REV), error_percent=8)
        qparams = rx.QualParams(trunc_qual=2)
        kw.update(primers=pats, quality=qparams)
        lo, hi, _ = trim_many(pats, [r for _, r in given])
        keep = np.array([qual_ref(qparams, r, q, int(a), int(b))[0] for (_, r), q, a, b in zip(given, quals, lo, hi)], np.uint32)
        assert all(int(a) >= 49 for a in lo[::5]) and (keep < hi).sum() > 20
        whole = [screen_ref(world.ref, p, r) for _, r in given[::5]]
        assert all(w[1] >= 9 for w in whole)                          # the whole read holds the stretch ...
    rows = [screen_ref(world.ref, p, r, int(a), int(b)) for (_, r), a, b in zip(given, lo, keep)]
    verdict = np.array([row[4] for row in rows])
    n_contam = int(verdict.sum())
    assert 60 < n_contam < 90
    if mode != "primers_quality":
        assert rows[10][:4] == (643, 25, 300, 0) and rows[10][4] == 0    # hits that make no contaminant
    if mode == "primers_quality":
        assert all(rows[i][4] == 0 and rows[i][1] == 0 for i in range(0, 260, 5) if i % 4 != 1 and i != 10 and i < 200)   # ... the kept range does not
    passing = [(l, r[int(a):int(b)].copy()) for (l, r), a, b, v in zip(given, lo, keep, verdict) if not v]
    plain = rx.Index(tree, derep=kw["derep"], identity=kw["identity"])
    screening = rx.Index(tree, contaminants=(world.obj, p), **kw)
    assert screening.screen[0] == p and screening.screen[1] != 0 and plain.screen is None
    for chunk in (0, 64, 100):
        if mode == "profile":
            plain.profile_begin(0.8)
            screening.profile_begin(0.8)
        want = _through_raxtax(plain, passing, chunk)
        assert rx.raxtax_last_screen() == (0, 0, 0, 0.0)               # the call before holds zeros
        assert want["screen"] == [(l, 0, 0, NONE, NONE, 0) for l, _ in passing]   # without a screen: the "off" values, per query
        got = _through_raxtax(screening, given, chunk, **({"quals": quals} if quals else {}))
        n_q, screened, contaminants, busy = rx.raxtax_last_screen()
        print(f"{mode}, chunk {chunk}: {n_q} queries, {screened} screened, {contaminants} contaminants, stage busy {busy * 1e3:.2f} ms, {len(got['sent'])} messages")
        assert (n_q, screened, contaminants) == (260, int((keep > lo).sum()), n_contam) and busy > 0
        assert got["screen"] == [(l, *row) for (l, _), row in zip(given, rows)]
        assert got["sent"] == want["sent"] and 120 < len(got["sent"]) <= len(passing)
        ok = {l for l, _ in passing}
        assert not ({l for l, v in zip([l for l, _ in given], verdict) if v} & {s[0] for s in got["sent"]})   # a contaminant has no message
        assert [a for a in got["align"]] == want["align"] and len(got["align"]) == len(got["sent"])
        if mode != "primers_quality":                                  # (there the plain handle sees reads that are cut already)
            assert [a for a in got["trim"] if a[0] in ok] == want["trim"]
            assert [a for a in got["qual"] if a[0] in ok] == want["qual"]
        # every query, in input order: trim, qual, screen, then align and the message where it has one
        order = {}
        for kind, label in got["events"]:
            order.setdefault(label, []).append(kind)
        assert [l for k, l in got["events"] if k == "screen"] == [l for l, _ in given]
        sent = {s[0] for s in got["sent"]}
        assert all(order[l] == ["trim", "qual", "screen"] + (["align", "sent"] if l in sent else []) for l, _ in given)
        if mode == "profile":
            a, b = plain.profile_read(), screening.profile_read()
            assert np.array_equal(a.clade, b.clade) and np.array_equal(a.direct, b.direct) and np.array_equal(a.conf_sum, b.conf_sum)
            assert np.array_equal(a.totals[1:3], b.totals[1:3]) and int(a.totals[1]) > 100   # classified and unclassified alike ...
            assert int(b.totals[0]) == 260 and int(b.totals[3]) - int(a.totals[3]) == n_contam   # ... a contaminant is unclassifiable, like any empty read
            plain.profile_end()
            screening.profile_end()
    if mode == "derep":
        q, u, _ = rx.raxtax_last_derep()
        assert q == 260 and u < 260 - 15
    # the same handle with the setting cleared is the plain handle again
    if mode == "plain":
        screening.set_screen(None)
        assert screening.screen is None
        assert _through_raxtax(screening, passing, 64)["sent"] == want["sent"]
        assert rx.raxtax_last_screen() == (0, 0, 0, 0.0)


def test_the_handle_keeps_the_set(mix):
    tree, world, queries = mix
    sset = rx.ScreenSet(world.seqs)
    index = rx.Index(tree, contaminants=sset)                          # (a set alone: the default parameters)
    assert index.screen[0] == DEFAULT
    want = [screen_ref(world.ref, DEFAULT, r) for _, r in queries]
    del sset                                                           # freed by the caller
    got = _through_raxtax(index, queries, 64)
    assert got["screen"] == [(l, *row) for (l, _), row in zip(queries, want)]


def test_handles_must_hold_the_same_set_and_parameters(mix):
    tree, world, queries = mix
    other_set = rx.ScreenSet([world.seqs[0][:5000]])
    for other in (None, (other_set, DEFAULT), (world.obj, rx.ScreenParams(min_hits=3)), (world.obj, rx.ScreenParams(min_pct=51))):
        with pytest.raises(rx.RtxError) as e:
            rx.raxtax(queries, [rx.Index(tree, contaminants=(world.obj, DEFAULT)), rx.Index(tree, contaminants=other)], False, False, 64, lambda *a: None, False)
        assert e.value.code == _lib.RTX_ERR_INVALID
    same = rx.ScreenSet(world.seqs)                                    # another object with the same keys
    sent = []
    rx.raxtax(queries, [rx.Index(tree, contaminants=(world.obj, DEFAULT)), rx.Index(tree, contaminants=(same, DEFAULT))], False, False, 64, lambda *a: sent.append(a), True)
    assert sent == _through_raxtax(rx.Index(tree, contaminants=(world.obj, DEFAULT)), queries, 64)["sent"]
    for bad in (rx.ScreenParams(min_hits=0), rx.ScreenParams(min_pct=101)):
        with pytest.raises(rx.RtxError) as e:
            rx.Index(tree, contaminants=(world.obj, bad))
        assert e.value.code == _lib.RTX_ERR_INVALID


def test_classify_ignores_the_setting(mix):
    tree, world, queries = mix
    from screen_common import concat
    bases, off = concat([r for _, r in queries[:40]])
    a = rx.Index(tree).classify(bases, off)
    b = rx.Index(tree, contaminants=(world.obj, DEFAULT)).classify(bases, off)
    assert np.array_equal(a.t, b.t) and np.array_equal(a.row_lineage, b.row_lineage) and np.array_equal(a.row_conf, b.row_conf)

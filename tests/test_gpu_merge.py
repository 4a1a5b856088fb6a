"""Paired-end merging on the device (rx.Merge, rtx_merge.hip) against the plain-Python restatement of tests/merge_common.py, exactly, on all four
result arrays and on every merged byte.  The cases (merge_common.cases): mate lengths at +-1 of a word of 16 bases, of one stride of candidates
(min_overlap + 64) and of the cap, unequal mates in both directions; true overlaps around min_overlap, around min_overlap + 64, at min(nf, nr) and
one below, at every (nf - ov) mod 16; diffs at exactly max_diffs, at 100 d == pct * ov and at score == min_overlap, each with its neighbour on the
other side; a diff at the first and the last position of the overlap, on both sides of a word boundary and in the last nibble of a partly filled
word; periodic amplicons whose best score is shared by several candidates; the consensus at every (qa, qb) of {0, 1, 2, 20, 21, 40, 41, 93}^2 on
an agreement and on a diff, IUPAC codes that intersect, code 0, N around the overlap's edges; bad bytes in either mate inside and outside the
overlap and at its ends, ascii_base 64; every verdict and their order; batches at +-1 of the pairs of a block through one object."""
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from merge_common import (BAD_QUALITY, BASE64, CONS, CONS_CAP0, CONS_CAP93, DEFAULT, LENGTHS, NO_OVERLAP, PCT, QS, SCORE1, TOO_LONG, TOO_SHORT, P, cases, concat,
                          expected, merge_ref)

pytestmark = pytest.mark.gpu


def _run(stage, pairs):
    fb, fo = concat([p[0] for p in pairs])
    fq, _ = concat([p[1] for p in pairs])
    rb, ro = concat([p[2] for p in pairs])
    rq, _ = concat([p[3] for p in pairs])
    return stage.run(fb, fq, fo, rb, rq, ro)


def _assert_equal(got, want, what):
    ov, d, v, ml, mb, mq, slot = got
    assert len(ov) == len(d) == len(v) == len(ml) == len(want) and len(slot) == len(want) + 1, what
    for name, g, k in (("overlap", ov, 0), ("diffs", d, 1), ("verdict", v, 2)):
        w = np.array([x[k] for x in want], np.uint32)
        bad = np.nonzero(np.asarray(g) != w)[0]
        assert len(bad) == 0, f"{what}: {name} differs at pairs {bad[:8].tolist()}: {np.asarray(g)[bad[:8]].tolist()} != {w[bad[:8]].tolist()}"
    for i, w in enumerate(want):
        assert int(ml[i]) == len(w[3]), f"{what}: merged length of pair {i}: {int(ml[i])} != {len(w[3])}"
        at = int(slot[i])
        assert at % 16 == 0 and int(slot[i + 1]) >= at + len(w[3])
        assert np.array_equal(mb[at:at + len(w[3])], w[3]), f"{what}: merged bases of pair {i}"
        assert np.array_equal(mq[at:at + len(w[3])], w[4]), f"{what}: merged quality bytes of pair {i}"


def test_the_expectation_covers_what_it_should():
    cs, ex = cases(), expected()
    by_tag = {}
    for p in cs:
        for c, e in zip(cs[p], ex[p]):
            by_tag.setdefault(c.tag, []).append((p, c, e))
    assert 150 <= sum(len(v) for v in cs.values()) <= 400
    lens = {(len(c.pair[0]), len(c.pair[2])) for c in cs[DEFAULT]}
    assert {(n, n) for n in LENGTHS} <= lens and any(a > b for a, b in lens) and any(a < b for a, b in lens)
    hit = lambda c, e: e[2] == 0 and (e[0], e[1]) == c.planted             # merged where and how it was planted
    assert all(hit(c, e) for _, c, e in by_tag["len"] if 16 <= len(c.pair[0]) <= 1024)
    assert {c.planted[0] for _, c, e in by_tag["len"] + by_tag["len2"] if hit(c, e)} >= {16, 17, 31, 32, 33, 79, 80, 81, 250, 251, 300, 1023, 1024}
    assert {e[0] for _, c, e in by_tag["len2"] if hit(c, e) and e[0] == min(len(c.pair[0]), len(c.pair[2])) - 1} >= {249, 1022, 78}
    assert {e[0] for _, c, e in by_tag["ov"] if hit(c, e)} == {16, 17, 79, 80, 81, 249, 250} and [e[2] for _, c, e in by_tag["ov"] if c.planted[0] == 15] == [NO_OVERLAP]
    assert {(250 - e[0]) % 16 for _, c, e in by_tag["ovmod"] if hit(c, e)} == set(range(16))
    assert hit(*by_tag["maxdiffs"][0][1:]) and by_tag["maxdiffs+1"][0][2][2] == NO_OVERLAP
    (_, c, e), = by_tag["score=min"]
    assert hit(c, e) and e[0] - 5 * e[1] == DEFAULT.min_overlap
    assert by_tag["score=min-1"][0][2][2] == NO_OVERLAP
    assert all(hit(c, e) and 100 * e[1] == PCT.max_diff_pct * e[0] for _, c, e in by_tag["pct="]) and len(by_tag["pct="]) == 2
    assert all(e[2] == NO_OVERLAP for _, c, e in by_tag["pct+1"]) and len(by_tag["pct+1"]) == 2
    assert all(hit(c, e) for _, c, e in by_tag["diffpos"]) and len(by_tag["diffpos"]) == 9
    assert all(hit(c, e) and e[0] % 16 for _, c, e in by_tag["tail"])
    for tag in ("tieA", "tieACGT"):                                          # several candidates share the best score; the largest ov is taken
        (_, c, e), = by_tag[tag]
        assert hit(c, e) and e[5] >= 2 and e[0] - 5 * e[1] == 40
        assert all(hit(c2, e2) for _, c2, e2 in by_tag[tag + "0"])
    for p in (CONS, CONS_CAP93, CONS_CAP0):
        (_, c, e), = [x for x in by_tag["consensus"] if x[0] == p]
        assert hit(c, e)
        qa, qb = c.pair[1][20:420].astype(int) - 33, c.pair[3][::-1][:400].astype(int) - 33
        fcodes, rcodes = c.pair[0][20:420], np.array([((int(x) & 1) << 3) | ((int(x) & 2) << 1) | ((int(x) & 4) >> 1) | ((int(x) & 8) >> 3) for x in c.pair[2][::-1][:400]])
        diff = (fcodes & rcodes) == 0
        assert {(a, b) for a, b, dd in zip(qa, qb, diff) if dd} >= {(a, b) for a in QS for b in QS}
        assert {(a, b) for a, b, dd in zip(qa, qb, diff) if not dd} >= {(a, b) for a in QS for b in QS}
        assert e[3][20 + 300:20 + 305].tolist() == [1, 15, 6, 2, 3]          # the IUPAC intersections
        assert c.pair[0][19] == 15 and c.pair[0][20] == 15 and e[3][19] == 15 and e[3][419] != 15 and e[3][420] == 15
        (_, c, e), = [x for x in by_tag["zero"] if x[0] == p]
        assert hit(c, e) and (e[3] == 0).sum() >= 1
    out = [e[4] for p, c, e in by_tag["consensus"]]
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[0], out[2])   # q_cap matters
    assert len(by_tag["bad"]) == 24 + 4 and all(e[2] == BAD_QUALITY for _, c, e in by_tag["bad"])
    assert all(hit(c, e) for _, c, e in by_tag["base64"] + by_tag["base64as33"])
    assert all(e[2] == BAD_QUALITY for _, c, e in by_tag["order:bad>long"] + by_tag["order:bad>short"]) and all(e[2] == TOO_LONG for _, c, e in by_tag["order:long>short"] + by_tag["long"])
    assert all(e[2] == NO_OVERLAP for _, c, e in by_tag["unrelated"])
    assert {e[2] for e in ex[DEFAULT]} == {0, BAD_QUALITY, TOO_LONG, TOO_SHORT, NO_OVERLAP}
    assert all(hit(c, e) for _, c, e in by_tag["min1"] if c.planted[0] >= 20) and {e[2] for _, c, e in by_tag["min1"]} == {0}


@pytest.mark.parametrize("p", [DEFAULT, PCT, SCORE1, CONS, CONS_CAP93, CONS_CAP0, BASE64], ids=["default", "pct", "min1", "cons", "cap93", "cap0", "base64"])
def test_device_equals_the_restatement(p):
    pairs = [c.pair for c in cases()[p]]
    stage = rx.Merge(0, rx.MergeParams(*p))
    _assert_equal(_run(stage, pairs), expected()[p], "cases")
    assert stage.kernel_ms() > 0 and stage.stage_seconds()[2] > 0
    _assert_equal(_run(stage, pairs[::-1]), expected()[p][::-1], "reversed")            # through the same object


def test_batches_of_every_size_through_one_object():
    stage = rx.Merge(0, rx.MergeParams(*DEFAULT))
    rng = random.Random(2)
    pool = [(c.pair, e) for c, e in zip(cases()[DEFAULT], expected()[DEFAULT])]
    first = None
    for n in (257, 1, 3, 4, 5, 63, 64, 65, 0):
        part = [pool[rng.randrange(len(pool))] for _ in range(n)]
        first = first or part
        _assert_equal(_run(stage, [x[0] for x in part]), [x[1] for x in part], f"batch of {n}")
    _assert_equal(_run(stage, [x[0] for x in first[::-1]]), [x[1] for x in first[::-1]], "the first batch reversed")
    assert stage.kernel_ms() > 0


def test_merge_queries_on_the_device():
    pool = [(c.pair, e) for c, e in zip(cases()[DEFAULT], expected()[DEFAULT]) if c.tag in ("ovmod", "diffpos", "unrelated", "len") and len(c.pair[0]) <= 1024]
    fwd = [(f"p{i}/1 a", x[0][0], x[0][1]) for i, x in enumerate(pool)]
    rev = [(f"p{i}/2 b", x[0][2], x[0][3]) for i, x in enumerate(pool)]
    recs, report = rx.merge_queries(rx.Merge(0, rx.MergeParams()), fwd, rev, queries_to_skip=["p1/1 a"])
    keep = [i for i in range(len(pool)) if i != 1]
    assert [r[0] for r in recs] == [fwd[i][0] for i in keep]
    for r, rep, i in zip(recs, report, keep):
        e = pool[i][1]
        assert rep == (len(fwd[i][1]), len(rev[i][1]), e[0], e[1], e[2]), i
        assert np.array_equal(r[1], e[3]) and np.array_equal(r[2], e[4]), i


def test_invalid_arguments():
    stage = rx.Merge(0, rx.MergeParams())
    b, q = np.full(40, 1, np.uint8), np.full(40, 70, np.uint8)
    ok = np.array([0, 20, 40], np.uint64)
    with pytest.raises(rx.RtxError) as e:
        stage.run(b, q, np.array([0, 30, 20, 40], np.uint64), b, q, np.array([0, 10, 20, 40], np.uint64))      # offsets that are not monotone
    assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        stage.run(b, q, ok, b, q, np.array([0, 30, 20], np.uint64))
    assert e.value.code == _lib.RTX_ERR_INVALID
    for which in (0, 1):                                                                                      # a quality byte of 128 or more
        q2 = q.copy()
        q2[17] = 128
        with pytest.raises(rx.RtxError) as e:
            stage.run(b, q2 if which == 0 else q, ok, b, q2 if which == 1 else q, ok)
        assert e.value.code == _lib.RTX_ERR_INVALID
    for p in (P(ascii_base=35), P(min_overlap=0), P(max_diff_pct=101), P(q_cap=94)):
        with pytest.raises(rx.RtxError) as e:
            rx.Merge(0, rx.MergeParams(*p))
        assert e.value.code == _lib.RTX_ERR_INVALID
    got = stage.run(b, q, ok, b, q, ok)                                                                       # the object works on after a refusal
    want = [merge_ref(DEFAULT, b[:20], q[:20], b[:20], q[:20])] * 2
    _assert_equal(got, want, "after the refusals")

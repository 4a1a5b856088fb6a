"""The quality filter on the device (rx.Qual, rtx_qual.hip) against the plain-integer restatement of tests/qual_common.py: lengths at +-1 of the
16-byte piece of a lane and of the 256-byte step of a group, the stopping position of trunc_qual and of trunc_ee at each of those
positions, every Q, N bases on either side of a cut, bad bytes, ascii_base 64, input ranges, and batches at +-1 of the reads of a wave (4)
and of a block (16) through one object."""
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from qual_common import (BAD_QUALITY, MAX_EE, MAX_EE_RATE, ONE, SHORT_FOR_TRUNC_LEN, TOO_LONG, TOO_MANY_N, TOO_SHORT, concat, qual_many, table)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 658, 5000]
STOPS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 658]
TRUNC_QUAL, TRUNC_EE, TRUNC_EE_0 = 2, 0.9, 0.15   # (TRUNC_EE_0: the threshold that one base of Q 6 passes -- a cut at position 0)
PARAMS = rx.QualParams(trunc_len=600, trunc_qual=TRUNC_QUAL, trunc_ee=TRUNC_EE, min_len=16, max_len=520, max_ns=2, max_ee=0.5, max_ee_rate=0.002)


FILTER_ONLY = rx.QualParams(max_ee=0.5, max_ns=0)


def _assert_equal(got, want, what):
    for name, g, w in zip(("hi", "ee", "verdict"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, f"{what}: {name} differs at reads {bad[:8].tolist()}: {np.asarray(g)[bad[:8]].tolist()} != {np.asarray(w)[bad[:8]].tolist()}"


@pytest.fixture(scope="module")
def reads():
    """About 300 (bases, quals) pairs, base 33.  Good reads (Q 35 .. 41: the sum of 5000 bases stays below TRUNC_EE) of every length, then the
    same with one stop planted at every position of STOPS: a base of Q <= TRUNC_QUAL, or two bases of Q 3 (e = 0.501 each: the sum is at
    most TRUNC_EE in front of the second one and above it with it; at position 0 one base of Q 6, for TRUNC_EE_0); N bases on either side."""
    rng = random.Random(11)
    out = []

    def good(n):
        bases = np.array([rng.choice([1, 2, 4, 8]) for _ in range(n)], np.uint8)
        quals = np.array([33 + rng.randint(35, 41) for _ in range(n)], np.uint8)
        return bases, quals

    for n in LENGTHS:                                   # nowhere
        out += [good(n), good(n), good(n)]
    for n in (17, 257, 258, 513, 514, 658, 700, 1024, 2049, 5000):
        for stop in STOPS:
            if stop >= n:
                continue
            b, q = good(n)                              # trunc_qual: the first base with Q <= TRUNC_QUAL is at `stop`
            q[stop] = 33 + rng.randint(0, TRUNC_QUAL)
            if stop + 3 < n:
                q[stop + 3] = 33                        # (a later one changes nothing)
            if stop >= 1:
                b[stop - 1] = 15                        # N bases on either side of the cut
            b[stop] = 15
            if stop + 1 < n:
                b[stop + 1] = 0
            out.append((b, q))
            b, q = good(n)                              # trunc_ee: the sum passes TRUNC_EE with the base at `stop`
            if stop >= 1:
                q[stop - 1] = q[stop] = 33 + 3
            else:
                q[0] = 33 + 6
            for k in range(max(0, stop - 3), min(n, stop + 2)):
                b[k] = (15, 5, 0)[k % 3]                # three N bases in front of the cut, two behind
            out.append((b, q))
    b, q = good(94 * 3)                                 # every Q of 0 .. 93
    q[:] = 33 + np.tile(np.arange(93, -1, -1), 3)
    out.append((b, q))
    out.append((b[::-1].copy(), q[::-1].copy()))
    for byte in (32, 127, 0, 33 + 94):                  # below the base and above base + 93
        for n, pos in ((1, 0), (17, 16), (300, 299), (700, 650), (5000, 4999)):
            b, q = good(n)
            q[pos] = byte
            out.append((b, q))
    return out


def test_the_expectation_covers_what_it_should(reads):
    hi, ee, verdict = qual_many(PARAMS, [r for r, _ in reads], [q for _, q in reads])
    lens = np.array([len(r) for r, _ in reads])
    assert 250 <= len(reads) <= 350
    seen = 0
    for v in verdict:
        seen |= int(v)
    assert seen == 127                                                          # every verdict bit
    assert ((verdict == 0) & (hi < np.minimum(lens, 600))).any()                # reads that pass and were cut short
    hi2, _, verdict2 = qual_many(FILTER_ONLY, [r for r, _ in reads], [q for _, q in reads])
    assert ((verdict2 == 0) & (hi2 == lens) & (lens > 0)).any() and (verdict2 != 0).any()   # untouched reads (PARAMS cuts or discards by trunc_len)
    assert (verdict == BAD_QUALITY).sum() == 20 and not ((verdict & BAD_QUALITY != 0) & (verdict != BAD_QUALITY)).any()
    only_q = qual_many(rx.QualParams(trunc_qual=TRUNC_QUAL), [r for r, _ in reads], [q for _, q in reads])[0]
    only_e = qual_many(rx.QualParams(trunc_ee=TRUNC_EE), [r for r, _ in reads], [q for _, q in reads])[0]
    only_0 = qual_many(rx.QualParams(trunc_ee=TRUNC_EE_0), [r for r, _ in reads], [q for _, q in reads])[0]
    for stop in STOPS:                                                          # both cuts land on every position
        assert (only_q == stop).any() and (((only_e if stop else only_0) == stop) & (only_q != stop)).any(), stop
    assert (only_q == lens).any() and (only_e == lens).any()                    # ... and nowhere


@pytest.mark.parametrize("p", [PARAMS, rx.QualParams(), rx.QualParams(trunc_qual=TRUNC_QUAL), rx.QualParams(trunc_ee=TRUNC_EE), rx.QualParams(trunc_ee=TRUNC_EE_0), FILTER_ONLY,
                               rx.QualParams(trunc_len=256, min_len=256, max_ee_rate=0.0005)], ids=["all", "off", "truncq", "truncee", "truncee0", "maxee", "trunclen"])
def test_device_equals_the_restatement(reads, p):
    bases, off = concat([r for r, _ in reads])
    quals, _ = concat([q for _, q in reads])
    stage = rx.Qual(0, p)
    want = qual_many(p, [r for r, _ in reads], [q for _, q in reads])
    _assert_equal(stage.run(bases, quals, off), want, "whole reads")
    assert stage.kernel_ms() > 0 and stage.stage_seconds()[2] > 0
    rev = reads[::-1]                                                            # the batch reversed, through the same object
    rb, ro = concat([r for r, _ in rev])
    rq, _ = concat([q for _, q in rev])
    _assert_equal(stage.run(rb, rq, ro), tuple(w[::-1] for w in want), "reversed")


def test_batches_of_every_size_through_one_object(reads):
    stage = rx.Qual(0, PARAMS)
    rng = random.Random(2)
    for n in (257, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 0):
        part = [reads[rng.randrange(len(reads))] for _ in range(n)]
        bases, off = concat([r for r, _ in part])
        quals, _ = concat([q for _, q in part])
        got = stage.run(bases, quals, off)
        assert all(len(g) == n for g in got)
        _assert_equal(got, qual_many(PARAMS, [r for r, _ in part], [q for _, q in part]), f"batch of {n}")


def test_input_ranges(reads):
    rng = random.Random(3)
    rs, qs = [r for r, _ in reads], [q for _, q in reads]
    lo = np.array([rng.randint(0, len(r)) if i % 3 else min(len(r), 1 + i % 40) for i, r in enumerate(rs)], np.uint32)
    hi = np.array([rng.randint(int(a), len(r)) if i % 5 else int(a) for i, (a, r) in enumerate(zip(lo, rs))], np.uint32)   # every fifth range is empty
    assert (lo > 0).sum() > 200 and (hi == lo).sum() >= 60
    bases, off = concat(rs)
    quals, _ = concat(qs)
    for p in (PARAMS, rx.QualParams(trunc_qual=TRUNC_QUAL, trunc_ee=0.3, max_ns=1)):
        want = qual_many(p, rs, qs, lo, hi)
        assert (want[0] >= lo).all() and (want[0] <= hi).all()
        _assert_equal(rx.Qual(0, p).run(bases, quals, off, lo, hi), want, "ranges")


def test_ascii_base_64(reads):
    part = [(r, (q.astype(np.int32) + 31).astype(np.uint8)) for r, q in reads if len(q) and q.min() >= 33 and q.max() <= 33 + 62]
    assert len(part) > 200
    p64 = rx.QualParams(ascii_base=64, trunc_qual=TRUNC_QUAL, trunc_ee=TRUNC_EE, max_ee=1.0)
    bases, off = concat([r for r, _ in part])
    quals, _ = concat([q for _, q in part])
    want = qual_many(p64, [r for r, _ in part], [q for _, q in part])
    p33 = rx.QualParams(trunc_qual=TRUNC_QUAL, trunc_ee=TRUNC_EE, max_ee=1.0)
    assert [tuple(int(x) for x in w) for w in zip(*want)] == [tuple(int(x) for x in w) for w in zip(*qual_many(p33, [r for r, _ in part], [(q - 31).astype(np.uint8) for _, q in part]))]
    _assert_equal(rx.Qual(0, p64).run(bases, quals, off), want, "base 64")
    low = [(r, q) for r, q in reads if len(q) and q.min() < 64][:40]             # bytes below base 64
    b2, o2 = concat([r for r, _ in low])
    q2, _ = concat([q for _, q in low])
    got = rx.Qual(0, p64).run(b2, q2, o2)
    assert (got[2] == BAD_QUALITY).all() and (got[0] == 0).all() and (got[1] == 0).all()


def test_invalid_arguments():
    stage = rx.Qual(0, PARAMS)
    bases, quals = np.full(16, 1, np.uint8), np.full(16, 70, np.uint8)
    cases = [
        dict(base_off=np.array([0, 8, 4, 16], np.uint64)),                                                              # base_off not monotone
        dict(base_off=np.array([0, 8, 16], np.uint64), lo=np.array([0, 9], np.uint32), hi=np.array([8, 9], np.uint32)),  # a range outside its read
        dict(base_off=np.array([0, 8, 16], np.uint64), lo=np.array([5, 0], np.uint32), hi=np.array([4, 8], np.uint32)),
    ]
    for kw in cases:
        with pytest.raises(rx.RtxError) as e:
            stage.run(bases, quals, **kw)
        assert e.value.code == _lib.RTX_ERR_INVALID
    q = quals.copy()
    q[9] = 128                                                                                                           # a quality byte >= 128
    with pytest.raises(rx.RtxError) as e:
        stage.run(bases, q, np.array([0, 8, 16], np.uint64))
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert [int(x) for x in stage.run(bases, q, np.array([0, 8, 16], np.uint64), np.array([0, 2], np.uint32), np.array([8, 2], np.uint32))[2]] == [TOO_SHORT | SHORT_FOR_TRUNC_LEN] * 2
    n = rx.QUAL_MAX_READ + 1                                                                                             # an over-long read
    with pytest.raises(rx.RtxError) as e:
        stage.run(np.full(n, 1, np.uint8), np.full(n, 70, np.uint8), np.array([0, n], np.uint64))
    assert e.value.code == _lib.RTX_ERR_INVALID
    for p in (rx.QualParams(ascii_base=35), rx.QualParams(trunc_qual=94), rx.QualParams(max_ee=float("nan"))):
        with pytest.raises(rx.RtxError) as e:
            rx.Qual(0, p)
        assert e.value.code == _lib.RTX_ERR_INVALID
    # the longest read there is, all Q 0: 2^20 * 2^40
    n = rx.QUAL_MAX_READ
    hi, ee, v = rx.Qual(0, rx.QualParams(max_ee=1e9)).run(np.full(n, 1, np.uint8), np.full(n, 33, np.uint8), np.array([0, n], np.uint64))
    assert (int(hi[0]), int(ee[0]), int(v[0])) == (n, n << 40, 0)

"""The quality filter without a device: the error table, rtx_qual_read (the host function) and emul_qual_read (the device's steps and pieces on
x86) against the plain-integer restatement of tests/qual_common.py, thresholds that a read meets exactly, and every rejected parameter."""
import ctypes as C
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from qual_common import (BAD_QUALITY, MAX_EE, MAX_EE_RATE, ONE, SHORT_FOR_TRUNC_LEN, TOO_LONG, TOO_MANY_N, TOO_SHORT, qual_ref, table, threshold)

LENGTHS = [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 658]


def _read(rng, n, base=33, qlo=2, qhi=41, n_rate=0.03):
    bases = np.array([rng.choice([1, 2, 4, 8]) if rng.random() >= n_rate else rng.choice([15, 5, 0, 3]) for _ in range(n)], np.uint8)
    quals = np.array([base + rng.randint(qlo, qhi) for _ in range(n)], np.uint8)
    return bases, quals


def _emul(emul, p, bases, quals, lo=0, hi_in=None):
    hi_in = len(bases) if hi_in is None else hi_in
    off = lambda t: (1 << 64) - 1 if t is None else t
    cfg32 = (C.c_int32 * 6)(p.ascii_base, p.trunc_len, max(p.trunc_qual, -1), p.min_len, p.max_len, max(p.max_ns, -1))
    cfg64 = (C.c_uint64 * 3)(off(threshold(p.trunc_ee)), off(threshold(p.max_ee)), off(threshold(p.max_ee_rate)))
    tab = (C.c_uint64 * 94)(*table())
    x = np.ascontiguousarray(quals[lo:hi_in] | np.where(np.isin(bases[lo:hi_in], [1, 2, 4, 8]), 0, 0x80).astype(np.uint8))
    kept, ee, v = C.c_uint32(), C.c_uint64(), C.c_uint32()
    emul.emul_qual_read.restype = None
    emul.emul_qual_read(cfg32, cfg64, tab, x.ctypes.data_as(_lib.u8p) if len(x) else None, C.c_uint32(len(x)), C.byref(kept), C.byref(ee), C.byref(v))
    return lo + kept.value, ee.value, v.value


def _both(emul, p, bases, quals, lo=0, hi_in=None):
    want = qual_ref(p, bases, quals, lo, hi_in)
    assert rx.qual_read(p, bases, quals, lo, hi_in) == want, (p, len(bases), lo, hi_in)
    assert _emul(emul, p, bases, quals, lo, hi_in) == want, (p, len(bases), lo, hi_in)
    return want


def test_the_error_table():
    e = table()
    assert len(e) == 94 and e[0] == 2 ** 40 and e[93] == 551
    assert all(a > b for a, b in zip(e, e[1:]))
    for q in range(94):
        assert abs(e[q] - 10 ** (-q / 10) * 2 ** 40) <= 1, q


PARAMS = [
    rx.QualParams(),
    rx.QualParams(trunc_len=100),
    rx.QualParams(trunc_qual=2),
    rx.QualParams(trunc_qual=20),
    rx.QualParams(trunc_ee=0.5),
    rx.QualParams(min_len=200),
    rx.QualParams(max_len=300),
    rx.QualParams(max_ns=0),
    rx.QualParams(max_ns=5),
    rx.QualParams(max_ee=1.0),
    rx.QualParams(max_ee_rate=0.004),
    rx.QualParams(trunc_len=250, trunc_qual=2, trunc_ee=3.0, min_len=50, max_len=240, max_ns=3, max_ee=2.0, max_ee_rate=0.01),
]


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_host_function_and_emulated_device_equal_the_restatement(emul, k):
    p = PARAMS[k]
    rng = random.Random(100 + k)
    seen = 0
    for n in LENGTHS:
        for qlo in (2, 3, 30, 36):   # reads that are cut early, and good ones that reach the length bounds
            bases, quals = _read(rng, n, qlo=qlo)
            seen |= _both(emul, p, bases, quals)[2]
            if n >= 4:
                lo = rng.randint(1, n // 2)
                hi = rng.randint(lo, n)
                seen |= _both(emul, p, bases, quals, lo, hi)[2]
                _both(emul, p, bases, quals, n // 2, n // 2)   # an empty range
    if k == len(PARAMS) - 1:
        assert seen == SHORT_FOR_TRUNC_LEN | TOO_SHORT | TOO_LONG | TOO_MANY_N | MAX_EE | MAX_EE_RATE   # the reads reach every reason


def test_ascii_base_64_and_bad_bytes(emul):
    rng = random.Random(7)
    p64 = rx.QualParams(ascii_base=64, trunc_qual=5, max_ee=2.0)
    for n in (1, 17, 300):
        bases, quals = _read(rng, n, base=64)
        _both(emul, p64, bases, quals)
        # the same bytes read with base 33 are Q 33 .. 72: valid, other values
        _both(emul, rx.QualParams(trunc_qual=40, max_ee=0.001), bases, quals)
    bases, quals = _read(rng, 300)
    for p in (rx.QualParams(), PARAMS[-1]):
        for pos, byte in ((0, 32), (299, 127), (150, 33 + 94), (16, 0)):
            q = quals.copy()
            q[pos] = byte
            assert _both(emul, p, bases, q) == (0, 0, BAD_QUALITY)
            if pos == 299:  # outside the input range the byte is not looked at
                assert _both(emul, p, bases, q, 10, 299)[2] != BAD_QUALITY
    # below base 64
    assert _both(emul, p64, bases, quals)[2] == BAD_QUALITY
    # behind the cut of trunc_len the byte still decides
    q = quals.copy()
    q[200] = 127
    assert _both(emul, rx.QualParams(trunc_len=100), bases, q) == (0, 0, BAD_QUALITY)


def test_every_q_and_the_stopping_positions(emul):
    bases = np.full(94, 1, np.uint8)
    quals = np.arange(33 + 93, 32, -1).astype(np.uint8)    # Q = 93 .. 0
    for tq in range(0, 94):
        hi, ee, v = _both(emul, rx.QualParams(trunc_qual=tq), bases, quals)
        assert hi == 93 - tq and ee == sum(table()[93 - i] for i in range(hi)) and v == 0
    # trunc_ee at every position of a longer read: the sum up to and including the base at `pos` is one unit above the threshold
    rng = random.Random(3)
    bases, quals = _read(rng, 600)
    run = 0
    for pos in range(600):
        run += table()[int(quals[pos]) - 33]
        if pos in (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 599):
            assert _both(emul, rx.QualParams(trunc_ee=(run - 1) / ONE), bases, quals)[0] == pos
            assert _both(emul, rx.QualParams(trunc_ee=run / ONE), bases, quals)[0] > pos


def test_thresholds_met_exactly(emul):
    rng = random.Random(5)
    bases, quals = _read(rng, 321, n_rate=0.0)
    ee = sum(table()[int(q) - 33] for q in quals)
    assert threshold(ee / ONE) == ee
    assert _both(emul, rx.QualParams(max_ee=ee / ONE), bases, quals) == (321, ee, 0)                  # ee == floor(x * 2^40) passes
    assert _both(emul, rx.QualParams(max_ee=(ee - 1) / ONE), bases, quals) == (321, ee, MAX_EE)       # one unit more fails
    # the rate: ee against r * 321
    r = ee // 321
    assert _both(emul, rx.QualParams(max_ee_rate=(r + 1) / ONE), bases, quals)[2] == 0
    assert _both(emul, rx.QualParams(max_ee_rate=r / ONE), bases, quals)[2] == (MAX_EE_RATE if ee > r * 321 else 0)
    same = np.full(321, 33 + 20, np.uint8)                                                             # ee == rate * kept exactly
    assert _both(emul, rx.QualParams(max_ee_rate=table()[20] / ONE), bases, same)[2] == 0
    assert _both(emul, rx.QualParams(max_ee_rate=(table()[20] - 1) / ONE), bases, same)[2] == MAX_EE_RATE
    # thresholds that clamp: nothing reaches 2^63, and the product with the kept length does not wrap
    for big in (1e7, 1e300, float("inf")):
        assert _both(emul, rx.QualParams(max_ee=big, max_ee_rate=big, trunc_ee=big), bases, quals) == (321, ee, 0)
    assert _both(emul, rx.QualParams(max_ee=0.0, max_ee_rate=0.0), bases, quals)[2] == MAX_EE | MAX_EE_RATE
    assert _both(emul, rx.QualParams(max_ee=0.0, max_ee_rate=0.0, trunc_ee=0.0), bases, quals) == (0, 0, 0)   # nothing kept: nothing exceeded
    # lengths: min_len and max_len are inclusive bounds, trunc_len of the exact length keeps all
    assert _both(emul, rx.QualParams(min_len=321, max_len=321, trunc_len=321), bases, quals)[2] == 0
    assert _both(emul, rx.QualParams(min_len=322), bases, quals)[2] == TOO_SHORT
    assert _both(emul, rx.QualParams(max_len=320), bases, quals)[2] == TOO_LONG
    assert _both(emul, rx.QualParams(trunc_len=322, min_len=322), bases, quals) == (321, ee, SHORT_FOR_TRUNC_LEN | TOO_SHORT)
    # N bases on either side of a cut
    b2 = bases.copy()
    b2[[10, 99, 100, 200]] = 15
    assert _both(emul, rx.QualParams(trunc_len=100, max_ns=1), b2, quals)[2] == TOO_MANY_N
    assert _both(emul, rx.QualParams(trunc_len=100, max_ns=2), b2, quals)[2] == 0
    assert _both(emul, rx.QualParams(trunc_len=99, max_ns=1), b2, quals)[2] == 0


def test_rejected_parameters_and_arguments():
    bases, quals = np.full(4, 1, np.uint8), np.full(4, 70, np.uint8)
    for p in (rx.QualParams(ascii_base=0), rx.QualParams(ascii_base=34), rx.QualParams(trunc_qual=94), rx.QualParams(trunc_ee=float("nan")),
              rx.QualParams(max_ee=float("nan")), rx.QualParams(max_ee_rate=float("nan"))):
        with pytest.raises(rx.RtxError) as e:
            rx.qual_read(p, bases, quals)
        assert e.value.code == _lib.RTX_ERR_INVALID, p
    for lo, hi in ((3, 2), (0, 5)):
        with pytest.raises(rx.RtxError) as e:
            rx.qual_read(rx.QualParams(), bases, quals, lo, hi)
        assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.qual_read(rx.QualParams(), bases, np.array([70, 70, 128, 70], np.uint8))
    assert e.value.code == _lib.RTX_ERR_INVALID
    big = np.full(rx.QUAL_MAX_READ + 1, 1, np.uint8)
    with pytest.raises(rx.RtxError) as e:
        rx.qual_read(rx.QualParams(), big, np.full(len(big), 70, np.uint8))
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert rx.qual_read(rx.QualParams(max_ee=1e9), big[:-1], np.full(len(big) - 1, 33, np.uint8)) == (rx.QUAL_MAX_READ, rx.QUAL_MAX_READ << 40, 0)   # 2^60


def test_verdict_names():
    assert rx.qual_verdict_names(0) == []
    assert rx.qual_verdict_names(MAX_EE | TOO_SHORT) == ["too_short", "max_ee"]
    assert rx.qual_verdict_names(127) == ["bad_quality", "short_for_trunc_len", "too_short", "too_long", "too_many_n", "max_ee", "max_ee_rate"]

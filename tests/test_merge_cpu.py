"""Paired-end merging without a device: rtx_merge_pair (the host function) and emul_merge_pair (the device's geometry on x86) against the
plain-Python restatement of tests/merge_common.py -- on random pairs cut from random amplicons with planted errors and on every case of the
device test --, every rejected parameter, rtx_fastq_block_end_n on texts cut at every byte, and the label pairing rule of rtx_merge_queries."""
import ctypes as C
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from merge_common import BAD_QUALITY, DEFAULT, NO_OVERLAP, P, TOO_LONG, TOO_SHORT, cases, expected, merge_ref, planted, revcomp


def _params(p):
    return rx.MergeParams(*p)


def _emul(emul, p, fb, fq, rb, rq):
    cfg = (C.c_uint32 * 5)(*p)
    out = (C.c_uint32 * 4)()
    mb, mq = (np.zeros(len(fb) + len(rb) + 1, np.uint8) for _ in range(2))
    one = np.zeros(1, np.uint8)
    arr = [np.ascontiguousarray(a, np.uint8) for a in (fb, fq, rb, rq)]
    ptrs = [(a if len(a) else one).ctypes.data_as(_lib.u8p) for a in arr]
    emul.emul_merge_pair.restype = None
    emul.emul_merge_pair(cfg, ptrs[0], ptrs[1], C.c_uint32(len(fb)), ptrs[2], ptrs[3], C.c_uint32(len(rb)), out, mb.ctypes.data_as(_lib.u8p), mq.ctypes.data_as(_lib.u8p))
    return out[0], out[1], out[2], mb[:out[3]], mq[:out[3]]


def _same(got, want, what):
    assert tuple(int(x) for x in got[:3]) == tuple(int(x) for x in want[:3]), what
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what


def _both(emul, p, pair, want=None):
    want = merge_ref(p, *pair) if want is None else want[:5]
    _same(rx.merge_pair(_params(p), *pair), want, ("host", p, len(pair[0]), len(pair[2])))
    _same(_emul(emul, p, *pair), want, ("emulator", p, len(pair[0]), len(pair[2])))
    return want


def test_random_pairs_with_planted_errors(emul):
    rng = random.Random(1)
    merged = wrong = 0
    for k in range(120):
        nf, nr = rng.randint(16, 300), rng.randint(16, 300)
        ov = rng.randint(1, min(nf, nr))
        diffs = tuple(sorted(rng.sample(range(ov), min(ov, rng.choice((0, 0, 1, 2, 5, 10, 11, 20))))))
        pair = planted(rng, nf, nr, ov, diffs=diffs, qlo=2, qhi=41)
        if k % 10 == 0:                                      # ambiguity codes and a base that is none
            for arr in (pair[0], pair[2]):
                for _ in range(3):
                    arr[rng.randrange(len(arr))] = rng.choice((0, 3, 5, 15, 10))
        p = (DEFAULT, P(min_overlap=8, max_diffs=5), P(max_diff_pct=5), P(q_cap=30, min_overlap=20))[k % 4]
        want = _both(emul, p, pair)
        merged += want[2] == 0
        wrong += want[2] == 0 and want[0] != ov
    assert 40 <= merged < 120 and wrong < merged // 4            # (of the restatement: both outcomes take a real share of the pairs)


def test_every_case_of_the_device_test(emul):
    seen = set()
    for p, cs in cases().items():
        for c, want in zip(cs, expected()[p]):
            _both(emul, p, c.pair, want)
            seen.add(want[2])
    assert seen == {0, BAD_QUALITY, TOO_LONG, TOO_SHORT, NO_OVERLAP}


def test_rejected_parameters_and_arguments():
    fb, fq = np.full(20, 1, np.uint8), np.full(20, 70, np.uint8)
    for p in (P(ascii_base=0), P(ascii_base=34), P(min_overlap=0), P(max_diff_pct=101), P(q_cap=94)):
        with pytest.raises(rx.RtxError) as e:
            rx.merge_pair(_params(p), fb, fq, fb, fq)
        assert e.value.code == _lib.RTX_ERR_INVALID, p
    q = fq.copy()
    q[3] = 128                                               # a byte that no FASTQ parse lets through
    for pair in ((fb, q, fb, fq), (fb, fq, fb, q)):
        with pytest.raises(rx.RtxError) as e:
            rx.merge_pair(_params(DEFAULT), *pair)
        assert e.value.code == _lib.RTX_ERR_INVALID
    for p in (P(max_diffs=0), P(max_diff_pct=0), P(q_cap=0), P(q_cap=93), P(min_overlap=1), P(min_overlap=5000), P(max_diffs=2 ** 32 - 1)):   # the edges that are allowed
        got = rx.merge_pair(_params(p), fb, fq, revcomp(fb), fq)
        _same(got, merge_ref(p, fb, fq, revcomp(fb), fq), p)
    assert rx.merge_verdict_names(0) == [] and rx.merge_verdict_names(8) == ["no_overlap"] and rx.merge_verdict_names(1) == ["bad_quality"]
    assert rx.MERGE_MAX_READ == 1024 and (rx.MG_BAD_QUALITY, rx.MG_TOO_LONG, rx.MG_TOO_SHORT, rx.MG_NO_OVERLAP) == (1, 2, 4, 8)
    with pytest.raises(rx.RtxError) as e:                    # checked before the device
        rx.Merge(0, _params(P(min_overlap=0)))
    assert e.value.code == _lib.RTX_ERR_INVALID


def test_fastq_block_end_n_at_every_byte():
    recs = ["@r1 x\nACGT\n+\n@@@@\n", "@r2\nAC\n+r2\n+@\n", "@r3\n\n+\n\n", "@r4\r\nACGTN\r\n+\r\n@+@+@\r\n", "@r5\nA\n+\n@"]   # quality lines that start with '@' and '+'
    text = "".join(recs)
    ends = np.cumsum([len(r) for r in recs]).tolist()
    for cut in range(len(text) + 1):
        part = text[:cut]
        whole = sum(1 for e in ends[:4] if e <= cut)         # (the last record has no final newline: it is never whole)
        for most in (0, 1, 2, 3, 4, 5, 100):
            n = min(whole, most)
            assert rx.fastq_block_end_n(part, most) == (ends[n - 1] if n else 0, n), (cut, most)
        assert rx.fastq_block_end_n(part, 2 ** 63)[0] == _lib.load().rtx_fastq_block_end(part.encode(), len(part))
    assert rx.fastq_block_end_n("", 3) == (0, 0)


def test_the_label_pairing_rule():
    """Without a device: rtx_merge_queries pairs the labels before it looks at its stage, so a NULL stage tells pairs that pair (RTX_ERR_INVALID
    for the stage) from pairs that do not (RTX_ERR_PARSE, naming the pair)."""
    rec = lambda label: (label, np.array([1, 2, 4, 8], np.uint8), np.full(4, 70, np.uint8))

    def code(fl, rl, n_extra=0):
        fwd = [rec("a"), rec(fl)]
        rev = [rec("a"), rec(rl)] + [rec("z")] * n_extra
        with pytest.raises(rx.RtxError) as e:
            rx.merge_queries(None, fwd, rev)
        return e.value.code, str(e.value)

    for fl, rl in (("r", "r"), ("r/1", "r/2"), ("r 1:N:0:1", "r 2:N:0:1"), ("r/1 first", "r/2\tsecond"), ("r", "r/2"), ("r/1", "r"), ("r/1/1", "r/1/2"), ("x/2", "x/2/2")):
        assert code(fl, rl)[0] == _lib.RTX_ERR_INVALID, (fl, rl)
    for fl, rl in (("r", "s"), ("r/2", "r/1"), ("r/1", "r/1"), ("r1 x", "r x"), ("r", "r2"), ("r/1x", "r/2x"), ("ra", "r")):
        c, msg = code(fl, rl)
        assert c == _lib.RTX_ERR_PARSE and "pair 2" in msg, (fl, rl, msg)
    c, msg = code("r", "r", n_extra=1)                       # record counts that differ
    assert c == _lib.RTX_ERR_PARSE and "2 forward and 3 reverse" in msg
    text = rx.fastq_text([rec("q/1"), ("e", np.zeros(0, np.uint8), np.zeros(0, np.uint8))])
    assert text == "@q/1\nACGT\n+\nFFFF\n@e\n\n+\n\n"
    back = rx.parse_query_fastq_str(text)
    assert [b[0] for b in back] == ["q/1", "e"] and back[0][1].tolist() == [1, 2, 4, 8]

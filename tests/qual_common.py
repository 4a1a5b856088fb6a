"""The reference of the tests of the quality filter: section "quality filter" of include/raxtax_hip.h restated with plain Python integers over
rx.qual_error_table() -- no numpy arithmetic, no floating point but the one conversion of a threshold (floor(x * 2^40), exact for a double).

Per read, input range [lo, hi_in), Q_i = qual_i - ascii_base:
  1. a byte of the range with Q_i outside 0 .. 93: verdict BAD_QUALITY alone, hi = lo, ee = 0;
  2. trunc_len: a range shorter than it is discarded (SHORT_FOR_TRUNC_LEN) and keeps its length, otherwise it is cut to that length;
  3. trunc_qual / trunc_ee within that: cut in front of the first base with Q <= trunc_qual, and in front of the first base at which the sum
     of e from lo, that base included, is above the threshold; the shorter wins;
  4. the verdict is the OR of every reason that applies to the kept bases."""
from fractions import Fraction
import math

import numpy as np

import raxtax_amd as rx

BAD_QUALITY, SHORT_FOR_TRUNC_LEN, TOO_SHORT, TOO_LONG, TOO_MANY_N, MAX_EE, MAX_EE_RATE = (1 << b for b in range(7))
ONE = 1 << 40

_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = rx.qual_error_table()
    return _TABLE


def threshold(x):
    """floor(x * 2^40), at most 2^63; None when the field is off (x < 0)."""
    if x < 0:
        return None
    if math.isinf(x):
        return 1 << 63
    return min(math.floor(Fraction(x) * ONE), 1 << 63)


def qual_ref(p, bases, quals, lo=0, hi_in=None):
    """(hi, ee, verdict) of one read for the rx.QualParams p."""
    e = table()
    hi_in = len(bases) if hi_in is None else hi_in
    q = [int(b) - p.ascii_base for b in quals[lo:hi_in]]
    n_flag = [int(b) not in (1, 2, 4, 8) for b in bases[lo:hi_in]]
    if any(x < 0 or x > 93 for x in q):
        return lo, 0, BAD_QUALITY
    verdict = 0
    end = len(q)
    if p.trunc_len:
        if end < p.trunc_len:
            verdict |= SHORT_FOR_TRUNC_LEN
        else:
            end = p.trunc_len
    kept = end
    if p.trunc_qual >= 0:
        for i in range(end):
            if q[i] <= p.trunc_qual:
                kept = min(kept, i)
                break
    t = threshold(p.trunc_ee)
    if t is not None:
        run = 0
        for i in range(end):
            run += e[q[i]]
            if run > t:
                kept = min(kept, i)
                break
    ee = sum(e[x] for x in q[:kept])
    ns = sum(n_flag[:kept])
    if p.min_len and kept < p.min_len:
        verdict |= TOO_SHORT
    if p.max_len and kept > p.max_len:
        verdict |= TOO_LONG
    if p.max_ns >= 0 and ns > p.max_ns:
        verdict |= TOO_MANY_N
    t = threshold(p.max_ee)
    if t is not None and ee > t:
        verdict |= MAX_EE
    t = threshold(p.max_ee_rate)
    if t is not None and ee > t * kept:
        verdict |= MAX_EE_RATE
    return lo + kept, ee, verdict


def qual_many(p, reads, quals, lo=None, hi=None):
    """(hi[n], ee[n], verdict[n]) as Qual.run returns them."""
    out = [qual_ref(p, r, q, 0 if lo is None else int(lo[i]), None if hi is None else int(hi[i])) for i, (r, q) in enumerate(zip(reads, quals))]
    return (np.array([o[0] for o in out], np.uint32), np.array([o[1] for o in out], np.uint64), np.array([o[2] for o in out], np.uint32))


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(0, np.uint8)])
    return flat, off


def fastq_text(records, line_end="\n", last_newline=True):
    """A FASTQ text of (label, letters, quality string) records."""
    text = "".join(f"@{l}{line_end}{s}{line_end}+{line_end}{q}{line_end}" for l, s, q in records)
    return text if last_newline else text[:len(text) - len(line_end)]


def ee_text(ee):
    """Expected errors as raxtax.qc prints them: from the integer, six decimals, truncated."""
    ee = int(ee)
    return f"{ee >> 40}.{(ee & (ONE - 1)) * 1000000 >> 40:06d}"

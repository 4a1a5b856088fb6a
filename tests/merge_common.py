"""Paired-end merging restated in plain Python (include/raxtax_hip.h, "paired-end merging"): positions one after the other, no words, no
packing, nothing of the library -- the expectation of tests/test_merge_cpu.py, tests/test_gpu_merge.py and tests/test_cli_merge_gpu.py --
and the builders of the planted pairs those tests share."""
import functools
import random
from typing import NamedTuple

import numpy as np

BAD_QUALITY, TOO_LONG, TOO_SHORT, NO_OVERLAP = 1, 2, 4, 8
MAX_READ, COST = 1024, 5
VERDICT_NAMES = {0: "merged", 1: "bad_quality", 2: "too_long", 4: "too_short", 8: "no_overlap"}


class P(NamedTuple):
    """rtx_merge_params"""
    ascii_base: int = 33
    min_overlap: int = 16
    max_diffs: int = 10
    max_diff_pct: int = 100
    q_cap: int = 41


COMP = [((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3) for c in range(16)]


def revcomp(codes):
    return np.array([COMP[int(c)] if c <= 15 else 0 for c in codes[::-1]], np.uint8)


def merge_full(p: P, fb, fq, rb, rq):
    """(overlap, diffs, verdict, merged bases, merged quality bytes, candidates that share the best score)"""
    none = np.zeros(0, np.uint8)
    nf, nr = len(fb), len(rb)
    for byte in list(fq) + list(rq):
        if not 0 <= int(byte) - p.ascii_base <= 93:
            return 0, 0, BAD_QUALITY, none, none, 0
    if nf > MAX_READ or nr > MAX_READ:
        return 0, 0, TOO_LONG, none, none, 0
    if nf < p.min_overlap or nr < p.min_overlap:
        return 0, 0, TOO_SHORT, none, none, 0
    f = np.array([int(c) if c <= 15 else 0 for c in fb], np.uint8)
    r = revcomp(rb)
    qf = [int(b) - p.ascii_base for b in fq]
    qr = [int(b) - p.ascii_base for b in rq[::-1]]
    best, ties = None, 0
    for ov in range(p.min_overlap, min(nf, nr) + 1):
        d = int(np.count_nonzero((f[nf - ov:] & r[:ov]) == 0))          # positions where the two codes share no base
        score = ov - COST * d
        if d <= p.max_diffs and 100 * d <= p.max_diff_pct * ov and score >= p.min_overlap:
            if best is not None and score == best[0]:
                ties += 1
            elif best is None or score > best[0]:
                ties = 1
            if best is None or (score, ov) > (best[0], best[1]):
                best = (score, ov, d)
    if best is None:
        return 0, 0, NO_OVERLAP, none, none, 0
    _, ov, d = best
    codes, quals = [], []
    for pos in range(nf + nr - ov):
        i = pos - (nf - ov)
        if i < 0:
            c, q = int(f[pos]), qf[pos]
        elif pos >= nf:
            c, q = int(r[i]), qr[i]
        else:
            a, qa, b, qb = int(f[pos]), qf[pos], int(r[i]), qr[i]
            if a == b and a != 0:
                c, q = a, max(max(qa, qb), min(qa + qb, p.q_cap))
            elif a & b:
                c, q = a & b, max(qa, qb)
            else:
                c, q = (b if qb > qa else a), max(abs(qa - qb), 2)
        codes.append(c)
        quals.append(p.ascii_base + q)
    return ov, d, 0, np.array(codes, np.uint8), np.array(quals, np.uint8), ties


def merge_ref(p: P, fb, fq, rb, rq):
    return merge_full(p, fb, fq, rb, rq)[:5]


# ---- builders ------------------------------------------------------------------------------------------------------------------------------
def rand_bases(rng, n):
    return np.array([rng.choice((1, 2, 4, 8)) for _ in range(n)], np.uint8)


def rand_quals(rng, n, base=33, lo=20, hi=41):
    return np.array([base + rng.randint(lo, hi) for _ in range(n)], np.uint8)


def other_base(rng, c):
    return rng.choice([x for x in (1, 2, 4, 8) if x & int(c) == 0] or [0])


def planted(rng, nf, nr, ov, diffs=(), base=33, amplicon=None, qlo=20, qhi=41):
    """A pair cut from a random amplicon of nf + nr - ov bases (or the one given) whose true overlap is ov, with a diff planted at every overlap
    position of `diffs` (the reverse mate is changed).  Returns [fb, fq, rb, rq]."""
    amp = rand_bases(rng, nf + nr - ov) if amplicon is None else np.asarray(amplicon, np.uint8)
    assert len(amp) == nf + nr - ov
    fb = amp[:nf].copy()
    rprime = amp[len(amp) - nr:].copy()
    for i in diffs:
        rprime[i] = other_base(rng, fb[nf - ov + i])
    return [fb, rand_quals(rng, nf, base, qlo, qhi), revcomp(rprime), rand_quals(rng, nr, base, qlo, qhi)]


LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 79, 80, 81, 250, 251, 300, 1023, 1024, 1025]
QS = [0, 1, 2, 20, 21, 40, 41, 93]
DEFAULT, PCT, SCORE1 = P(), P(max_diffs=20, max_diff_pct=10), P(min_overlap=1)
CONS, CONS_CAP93, CONS_CAP0, BASE64 = P(max_diffs=64), P(max_diffs=64, q_cap=93), P(max_diffs=64, q_cap=0), P(ascii_base=64)


class Case(NamedTuple):
    tag: str
    pair: list          # fb, fq, rb, rq
    planted: tuple      # (ov, d) the builder meant, or None


@functools.lru_cache(maxsize=None)
def cases():
    """{params: [Case]}: every class of tests/test_gpu_merge.py's docstring; test_the_expectation_covers_what_it_should asserts that they are there."""
    rng = random.Random(20)
    out = {k: [] for k in (DEFAULT, PCT, SCORE1, CONS, CONS_CAP93, CONS_CAP0, BASE64)}

    def add(p, tag, pair, plant=None):
        out[p].append(Case(tag, pair, plant))

    # mate lengths: equal mates overlapping entirely and at min_overlap, then unequal ones in both directions
    for n in LENGTHS:
        add(DEFAULT, "len", planted(rng, n, n, n), (n, 0))
        if n >= 16:
            add(DEFAULT, "len", planted(rng, n, n, 16), (16, 0))
    for nf, nr in ((250, 300), (300, 250), (1024, 80), (80, 1024), (1025, 250), (250, 1025), (17, 1024), (1023, 33), (0, 250), (250, 0), (15, 300), (300, 15),
                   (1024, 1023), (81, 79), (33, 31), (1, 0)):
        m = min(nf, nr)
        for ov in sorted({m, max(m - 1, 0), min(16, m)}):
            add(DEFAULT, "len2", planted(rng, nf, nr, ov), (ov, 0))
    # true overlaps: around min_overlap, around one stride of candidates, every (nf - ov) mod 16
    for ov in (15, 16, 17, 79, 80, 81, 249, 250):
        add(DEFAULT, "ov", planted(rng, 250, 251, ov), (ov, 0))
    for ov in range(100, 116):
        add(DEFAULT, "ovmod", planted(rng, 250, 240, ov, diffs=(3, ov - 2)), (ov, 2))
    # diffs: exactly max_diffs and one more; the score exactly min_overlap and one below
    ten = tuple(range(5, 95, 9))
    add(DEFAULT, "maxdiffs", planted(rng, 250, 250, 100, diffs=ten), (100, 10))
    add(DEFAULT, "maxdiffs+1", planted(rng, 250, 250, 100, diffs=ten + (97,)), (100, 11))
    add(DEFAULT, "score=min", planted(rng, 200, 200, 66, diffs=tuple(range(2, 62, 6))), (66, 10))
    add(DEFAULT, "score=min-1", planted(rng, 200, 200, 65, diffs=tuple(range(2, 62, 6))), (65, 10))
    add(PCT, "pct=", planted(rng, 250, 250, 100, diffs=ten), (100, 10))
    add(PCT, "pct=", planted(rng, 250, 250, 110, diffs=ten + (100,)), (110, 11))
    add(PCT, "pct+1", planted(rng, 250, 250, 109, diffs=ten + (100,)), (109, 11))
    add(PCT, "pct+1", planted(rng, 250, 250, 99, diffs=ten), (99, 10))
    # a diff at the first and the last position, on both sides of a word boundary of R' (15 | 16) and of F (nf - ov + i = 160: i = 9 | 10),
    # and in the last nibble of a partly filled word (ov = 100: i = 99)
    for i in (0, 99, 15, 16, 9, 10, 95, 96):
        add(DEFAULT, "diffpos", planted(rng, 250, 250, 100, diffs=(i,)), (100, 1))
    add(DEFAULT, "diffpos", planted(rng, 250, 250, 100, diffs=(0, 9, 10, 15, 16, 95, 96, 99)), (100, 8))
    for ov in (22, 31, 33, 45, 50, 59):                    # the tail mask at other fill levels, the diff in the last nibble
        add(DEFAULT, "tail", planted(rng, 120, 130, ov, diffs=(ov - 1,)), (ov, 1))
    # ties: periodic amplicons whose reverse mate disagrees at 40, 45, 50, 55 -- the candidates 40, 45 .. 60 of (A)^k, 40 and 60 of (ACGT)^k score 40
    for unit, tag in (((1,), "tieA"), ((1, 2, 4, 8), "tieACGT")):
        amp = np.array(unit * 60, np.uint8)[:60]
        fb, rp = amp.copy(), amp.copy()
        for i in (40, 45, 50, 55):
            rp[i] = COMP[int(rp[i])] if unit == (1,) else 0
        add(DEFAULT, tag, [fb, rand_quals(rng, 60), revcomp(rp), rand_quals(rng, 60)], (60, 4))
        add(DEFAULT, tag + "0", [amp.copy(), rand_quals(rng, 60), revcomp(amp), rand_quals(rng, 60)], (60, 0))
        big = np.array(unit * 1024, np.uint8)[:1024]
        add(DEFAULT, tag + "0", [big.copy(), rand_quals(rng, 1024), revcomp(big), rand_quals(rng, 1024)], (1024, 0))
    # consensus: every (qa, qb) on an agreement (i = 200 ..) and on a diff (i = 100 ..), IUPAC codes that intersect, code 0, N at the overlap's edges
    for p in (CONS, CONS_CAP93, CONS_CAP0):
        pair = planted(rng, 420, 410, 400, diffs=tuple(range(100, 164)))
        nf, nr, ov = 420, 410, 400
        for k, (qa, qb) in enumerate((a, b) for a in QS for b in QS):
            for i in (100 + k, 200 + k):
                pair[1][nf - ov + i] = 33 + qa
                pair[3][nr - 1 - i] = 33 + qb
        fb, rb = pair[0], pair[2]

        def set_pair(i, a, b):                               # F[nf - ov + i] = a against R'[i] = b
            fb[nf - ov + i] = a
            rb[nr - 1 - i] = COMP[b]
        set_pair(300, 5, 1)                                  # R against A: A
        set_pair(301, 15, 15)                                # N against N: an agreement
        set_pair(302, 7, 14)                                 # V against B: S
        set_pair(303, 15, 2)
        set_pair(304, 3, 3)                                  # M against M: an agreement on an ambiguity code
        set_pair(0, 15, int(COMP[int(rb[nr - 1])]))          # N inside, at either edge of the overlap
        set_pair(ov - 1, int(fb[nf - 1]), 15)
        fb[nf - ov - 1] = 15                                 # N outside, next to either edge
        rb[nr - 1 - ov] = 15
        add(p, "consensus", pair, (400, 64))
        zero = planted(rng, 300, 300, 200)
        for i, (a, b) in enumerate(((0, 0), (0, 1), (2, 0), (0, 15), (16, 1), (200, 200))):   # code 0, and bytes that are no code
            zero[0][100 + 20 * i] = a
            zero[2][300 - 1 - 20 * i] = COMP[b] if b <= 15 else b
            zero[1][100 + 20 * i], zero[3][300 - 1 - 20 * i] = 33 + (30, 10, 25)[i % 3], 33 + (10, 30, 25)[i % 3]
        add(p, "zero", zero, (200, 6))
    # bad bytes in either mate: inside and outside the overlap, at position 0 and the last one
    for byte in (32, 127, 33 + 94):
        for mate, pos in ((1, 0), (1, 249), (1, 200), (1, 50), (3, 0), (3, 249), (3, 30), (3, 150)):
            pair = planted(rng, 250, 250, 100)
            pair[mate][pos] = byte
            add(DEFAULT, "bad", pair)
    for nf, nr, ov in ((250, 250, 100), (80, 33, 20)):
        add(BASE64, "base64", planted(rng, nf, nr, ov, base=64, qlo=0, qhi=41), (ov, 0))
        add(DEFAULT, "base64as33", planted(rng, nf, nr, ov, base=64, qlo=0, qhi=41), (ov, 0))     # the same bytes are Q 31 .. 72 at base 33
        low = planted(rng, nf, nr, ov, base=64)
        low[1 + 2 * (ov % 3 == 0)][7] = 63
        add(BASE64, "bad", low)
        add(BASE64, "bad", planted(rng, nf, nr, ov, base=33))                                    # bytes below base 64 everywhere
    # verdicts and their order
    add(DEFAULT, "order:bad>long", planted(rng, 1025, 250, 100))
    out[DEFAULT][-1].pair[1][1024] = 127
    add(DEFAULT, "order:bad>long", planted(rng, 250, 1500, 100))
    out[DEFAULT][-1].pair[3][1499] = 32
    add(DEFAULT, "order:bad>short", planted(rng, 5, 250, 5))
    out[DEFAULT][-1].pair[3][0] = 32
    add(DEFAULT, "order:long>short", planted(rng, 1025, 5, 5))
    add(DEFAULT, "order:long>short", planted(rng, 3, 2000, 3))
    add(DEFAULT, "long", planted(rng, 1500, 1500, 100))
    for _ in range(6):                                       # unrelated mates
        add(DEFAULT, "unrelated", [rand_bases(rng, 250), rand_quals(rng, 250), rand_bases(rng, 250), rand_quals(rng, 250)])
    # min_overlap 1: candidates from a single base on, mates of one base
    for nf, nr, ov in ((1, 1, 1), (1, 5, 1), (20, 20, 1), (20, 20, 2), (64, 64, 64), (65, 64, 63), (100, 129, 66)):
        add(SCORE1, "min1", planted(rng, nf, nr, ov), (ov, 0))
    return out


def concat(arrays):
    off = np.zeros(len(arrays) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    return (np.concatenate(arrays).astype(np.uint8) if len(arrays) and off[-1] else np.zeros(0, np.uint8)), off


@functools.lru_cache(maxsize=None)
def expected():
    """{params: [merge_full(...) of every case]}"""
    return {p: [merge_full(p, *c.pair) for c in cs] for p, cs in cases().items()}

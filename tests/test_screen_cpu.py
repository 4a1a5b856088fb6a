"""The contaminant screen without a device: rx.screen_read (the host function) and emul_screen_read (the device's pieces and steps on x86)
against the plain-Python restatement of tests/screen_common.py -- lengths and planted stretches at +-1 of the 16-position piece of a lane and
of the 256-position step of a group, breaking codes, near misses, palindromes and homopolymers, shared k-mers, a table whose chains are
long and wrap, a large set, thresholds that a read meets exactly, and every rejected argument."""
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from screen_common import (K, NONE, World, adversarial_world, canonical, emul_read, home_slot, kmer_codes, large_reads, large_world, plant, random_codes, rc_value,
                           revcomp, screen_ref)

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 270, 271, 272, 511, 512, 513, 658]
DEFAULT = rx.ScreenParams()


@pytest.fixture(scope="module")
def genome():
    """One seeded random 5 386-base "genome" and a short second sequence."""
    rng = random.Random(5386)
    return World([random_codes(rng, 5386), random_codes(rng, 300)])


def _both(emul, world, p, codes, lo=0, hi=None):
    want = screen_ref(world.ref, p, codes, lo, hi)
    assert rx.screen_read(world.obj, p, codes, lo, hi) == want, (len(codes), lo, hi)
    assert emul_read(emul, world.obj, codes, lo, hi) == want[:4], (len(codes), lo, hi)
    return want


def test_the_set_is_the_restatements(genome):
    info = genome.obj.info()
    assert info["keys"] == len(genome.ref) and info["slots"] == 16384 >= 2 * info["keys"] > 8192   # the smallest power of two >= 2 |S|
    slots, log2m = genome.obj.table()
    assert 1 << log2m == info["slots"] == len(slots)
    stored = {int(k): int(s) for k, s in slots if int(k) != NONE}
    assert stored == genome.ref
    assert all(int(s) == NONE for k, s in slots if int(k) == NONE)


def test_table_size_rule():
    rng = random.Random(1)
    for n_bases, slots in ((16, 1024), (16 + 511, 1024), (16 + 512, 2048), (16 + 1023, 2048), (16 + 1024, 4096)):
        w = World([random_codes(rng, n_bases)])
        if len(w.ref) == n_bases - 15:   # (no value twice: the rule is about |S|)
            assert w.obj.info()["slots"] == slots, n_bases


def test_lengths_and_ranges(emul, genome):
    rng = random.Random(2)
    for n in LENGTHS:
        for _ in range(2):
            codes = random_codes(rng, n)
            want = _both(emul, genome, DEFAULT, codes)
            assert want[0] == max(0, n - 15) and want[4] == 0
            if n >= 4:
                lo = rng.randint(1, n // 2)
                _both(emul, genome, DEFAULT, codes, lo, rng.randint(lo, n))
                _both(emul, genome, DEFAULT, codes, n // 2, n // 2)   # an empty range
        src = genome.seqs[0][100:100 + n]                             # a piece of the genome: every window hits
        want = _both(emul, genome, DEFAULT, src)
        assert want[:4] == ((n - 15, n - 15, 0, 0) if n >= 16 else (0, 0, NONE, NONE)) and want[4] == (n >= 17)
        assert _both(emul, genome, DEFAULT, revcomp(src))[:2] == want[:2]


@pytest.mark.parametrize("h", [1, 2, 3])
def test_planted_stretches(emul, genome, h):
    rng = random.Random(10 + h)
    p = rx.ScreenParams(min_hits=h, min_pct=0)
    for off in LENGTHS:
        g = rng.randrange(1, 5386 - 40)
        for rc in (False, True):                                      # both orientations of the contaminant
            for tail in (0, 1, 40):                                   # the stretch ends the read, or not
                codes = plant(random_codes(rng, off + K + h - 1 + tail), off, genome.seqs[0], g, K + h - 1, rc)
                want = _both(emul, genome, p, codes)
                assert want == (len(codes) - 15, h, off, 0, 1), (off, tail)
                back = _both(emul, genome, p, revcomp(codes))         # the read given the other way round
                assert back[:2] == want[:2] and back[4] == 1 and back[2] == tail
                assert _both(emul, genome, rx.ScreenParams(min_hits=h + 1, min_pct=0), codes)[4] == 0


def test_breaking_codes(emul, genome):
    rng = random.Random(20)
    h = 3
    p = rx.ScreenParams(min_hits=1, min_pct=0)
    for off in (1, 16, 250):
        stretch = genome.seqs[0][700 + off:700 + off + K + h - 1]
        base = plant(random_codes(rng, off + len(stretch) + 30), off, genome.seqs[0], 700 + off, len(stretch))
        assert _both(emul, genome, p, base)[1] == h
        for at in range(off - 1, off + len(stretch) + 1):
            for code in (15, 0, 5):
                codes = base.copy()
                codes[at] = code                                      # (outside the stretch the base differs from the genome's already)
                want = _both(emul, genome, p, codes)
                covering = sum(1 for w in range(off, off + h) if w <= at < w + K)   # the hitting windows that hold position `at`
                assert want[1] == h - covering, (off, at, code)
                assert (covering == 0) == (at in (off - 1, off + len(stretch)))
                assert want[0] == len(codes) - 15 - sum(1 for w in range(len(codes) - 15) if w <= at < w + K)


def test_near_misses(emul, genome):
    rng = random.Random(30)
    for _ in range(8):
        g = rng.randrange(0, 5386 - K)
        member = genome.seqs[0][g:g + K]
        assert _both(emul, genome, rx.ScreenParams(min_hits=1), member)[:4] == (1, 1, 0, 0)
        for j in range(K):
            for code in (1, 2, 4, 8):
                if code != member[j]:
                    near = member.copy()
                    near[j] = code
                    want = _both(emul, genome, DEFAULT, near)         # (it must not hit unless the restatement says so)
                    assert want[0] == 1 and want[1] == (1 if canonical_of(near) in genome.ref else 0)


def canonical_of(codes):
    w = 0
    for c in codes:
        w = w << 2 | {1: 0, 2: 1, 4: 2, 8: 3}[int(c)]
    return canonical(w)


def test_palindromes_and_homopolymers(emul):
    pal = [int("".join(f"{b:02b}" for b in bases), 2) for bases in ([0, 1, 2, 3] * 4, [0, 3] * 8, [2, 1] * 8, [0, 0, 0, 0, 1, 1, 2, 2, 1, 1, 2, 2, 3, 3, 3, 3])]
    assert all(w == rc_value(w) for w in pal)
    homo = [int(f"{b:02b}" * 16, 2) for b in range(4)]
    assert [canonical(w) for w in homo] == [0, 0x55555555, 0x55555555, 0]
    one = rx.ScreenParams(min_hits=1)
    for members in (pal, homo, [homo[3]], [homo[2]]):
        world = World([kmer_codes(w) for w in members])
        assert len(world.ref) == len({canonical(w) for w in members})
        for w in pal + homo:
            want = _both(emul, world, one, kmer_codes(w))
            assert want[1] == (canonical(w) in world.ref)
        # a homopolymer run of 40 bases: 25 windows of one value
        for b in range(4):
            want = _both(emul, world, one, np.full(40, 1 << b, np.uint8))
            assert want[:2] == (25, 25 if canonical(homo[b]) in world.ref else 0)
    assert NONE not in (canonical(w) for w in homo)                   # no canonical value is the empty slot's word


def test_shared_kmers_name_the_lowest_source(emul):
    rng = random.Random(40)
    seqs = [random_codes(rng, 60) for _ in range(6)]
    shared = random_codes(rng, K)
    seqs[5][10:10 + K] = shared
    seqs[2][30:30 + K] = revcomp(shared)                              # the same canonical value, the other strand
    seqs[4][0:K] = shared
    world = World(seqs)
    for q in (shared, revcomp(shared)):
        assert _both(emul, world, rx.ScreenParams(min_hits=1), q)[:4] == (1, 1, 0, 2)
    read = plant(random_codes(rng, 42), 7, np.concatenate([[1], seqs[5]]).astype(np.uint8), 1, 30)   # the first hit belongs to sequence 5 alone
    want = _both(emul, world, DEFAULT, read)
    assert want[2] == 7 and want[3] == 5 and want[1] == 15


@pytest.fixture(scope="module")
def adversarial():
    return adversarial_world()


def test_adversarial_table(emul, adversarial):
    world, keys, absent = adversarial
    info = world.obj.info()
    assert info["keys"] == 18 and info["slots"] == 1024
    assert info["max_displacement"] >= 8 and info["wrapped"] >= 1
    slots, log2m = world.obj.table()
    chain = [int(slots[s % 1024][0]) for s in range(1020, 1020 + 17)]
    assert NONE not in chain[:16] and chain[16] == NONE              # sixteen keys in a row, across the wrap, then the empty slot
    # ascending insertion: among keys of one home slot the smaller one sits nearer to it
    for home in (1020, 1022, 1023):
        at = [i for i, c in enumerate(chain[:16]) if home_slot(c, 10) == home]
        assert [chain[i] for i in at] == sorted(chain[i] for i in at)
    one = rx.ScreenParams(min_hits=1)
    for i, c in enumerate(keys):
        for q in (kmer_codes(c), revcomp(kmer_codes(c))):
            assert _both(emul, world, one, q) == (1, 1, 0, i, 1)
    for c in absent:                                                  # the lookup walks to the empty slot, across the wrap, and says no
        assert _both(emul, world, one, kmer_codes(c)) == (1, 0, NONE, NONE, 0)
        assert _both(emul, world, one, revcomp(kmer_codes(c)))[1] == 0
    # all of them in one read, separated by a breaking code
    read = np.concatenate([np.concatenate([kmer_codes(c), [15]]) for c in absent[:8] + keys + absent[8:]]).astype(np.uint8)
    assert _both(emul, world, one, read)[:4] == (len(keys) + len(absent), len(keys), 8 * 17, 0)


@pytest.fixture(scope="module")
def large():
    return large_world()


def test_large_set(emul, large):
    obj, ref, members, others = large
    info = obj.info()
    assert info["keys"] == 200_000 and info["slots"] == 1 << 19
    world = World.__new__(World)
    world.obj, world.ref = obj, ref
    one = rx.ScreenParams(min_hits=1)
    reads = large_reads(members, others)
    hits = 0
    for i, r in enumerate(reads):
        want = screen_ref(ref, one, r)
        assert rx.screen_read(obj, one, r) == want, i
        if i % 16 == 0 or i >= len(reads) - 8:
            assert emul_read(emul, obj, r) == want[:4], i
        hits += want[1]
    assert hits == 200_000 + 4096                                      # every member hit, no other value did


def threshold_cases(genome, rng):
    """(params, read, expected verdict): reads that meet a threshold exactly, and the same with one hit fewer."""
    g = genome.seqs[0]
    cases = []

    def read(hits, windows):       # `hits` hitting windows at the front, windows - hits others behind them
        codes = random_codes(rng, windows + 15)
        return plant(codes, 0, g, 1000, hits + 15) if hits else codes

    for m in (1, 2, 3, 7):
        cases += [(rx.ScreenParams(min_hits=m, min_pct=0), read(m, 40), 1), (rx.ScreenParams(min_hits=m, min_pct=0), read(m - 1, 40), 0)]
    for pct, hits, windows in ((50, 5, 10), (50, 2, 4), (25, 1, 4), (100, 6, 6), (100, 1, 1), (1, 1, 100), (33, 33, 100), (99, 99, 100), (10, 30, 300)):
        assert 100 * hits == pct * windows
        cases += [(rx.ScreenParams(min_hits=1, min_pct=pct), read(hits, windows), 1)]
        if hits > 1:
            cases += [(rx.ScreenParams(min_hits=1, min_pct=pct), read(hits - 1, windows), 0)]
    cases += [(rx.ScreenParams(min_hits=1, min_pct=100), read(5, 6), 0), (rx.ScreenParams(min_hits=1, min_pct=0), read(0, 20), 0),
              (DEFAULT, read(2, 4), 1), (DEFAULT, read(1, 1), 0), (DEFAULT, read(2, 5), 0)]
    return cases


def test_the_expectation_covers_the_threshold_equalities(genome):
    seen = set()
    for p, codes, verdict in threshold_cases(genome, random.Random(70)):
        windows, hits, first, source, v = screen_ref(genome.ref, p, codes)
        assert v == verdict, (p, windows, hits)
        if hits == p.min_hits and v:
            seen.add("hits == min_hits")
        if hits == p.min_hits - 1 and 100 * hits >= p.min_pct * windows:
            seen.add("one fewer than min_hits")
        if 100 * hits == p.min_pct * windows and hits >= p.min_hits and p.min_pct:
            seen.add("100 hits == min_pct windows")
        if 100 * (hits + 1) == p.min_pct * windows and hits >= p.min_hits:
            seen.add("one hit fewer than min_pct")
    assert seen == {"hits == min_hits", "one fewer than min_hits", "100 hits == min_pct windows", "one hit fewer than min_pct"}


def test_threshold_equalities(emul, genome):
    for p, codes, verdict in threshold_cases(genome, random.Random(70)):
        assert _both(emul, genome, p, codes)[4] == verdict
        assert _both(emul, genome, p, revcomp(codes))[4] == verdict


def test_rejected_parameters_sets_and_arguments(genome):
    codes = genome.seqs[0][:40]
    for p in (rx.ScreenParams(min_hits=0), rx.ScreenParams(min_pct=101), rx.ScreenParams(min_hits=0, min_pct=200)):
        with pytest.raises(rx.RtxError) as e:
            rx.screen_read(genome.obj, p, codes)
        assert e.value.code == _lib.RTX_ERR_INVALID, p
    assert rx.screen_read(genome.obj, rx.ScreenParams(min_hits=1, min_pct=0), codes)[4] == 1
    assert rx.screen_read(genome.obj, rx.ScreenParams(min_hits=1 << 31, min_pct=100), codes)[4] == 0
    for lo, hi in ((3, 2), (0, 41)):
        with pytest.raises(rx.RtxError) as e:
            rx.screen_read(genome.obj, DEFAULT, codes, lo, hi)
        assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.screen_read(genome.obj, DEFAULT, np.full(rx.SCREEN_MAX_READ + 1, 1, np.uint8))
    assert e.value.code == _lib.RTX_ERR_INVALID
    n = rx.SCREEN_MAX_READ                                            # the longest read there is
    assert rx.screen_read(genome.obj, DEFAULT, np.full(n, 2, np.uint8)) == (n - 15, 0, NONE, NONE, 0)
    sets = [
        (np.full(40, 1, np.uint8), np.array([0, 30, 20, 40], np.uint64)),            # base_off not monotone
        (np.full(15, 1, np.uint8), np.array([0, 15], np.uint64)),                    # no valid window: too short
        (np.array([1] * 10 + [15] + [2] * 15, np.uint8), np.array([0, 26], np.uint64)),   # ... broken by an N
        (np.full(30, 1, np.uint8), np.array([0, 15, 30], np.uint64)),                # ... two sequences of 15 bases (no window spans them)
        (np.zeros(0, np.uint8), np.array([0], np.uint64)),                           # no sequence
        (np.full(rx.SCREEN_MAX_BASES + 1, 1, np.uint8), np.array([0, rx.SCREEN_MAX_BASES + 1], np.uint64)),   # one base too many, really there
    ]
    for bases, off in sets:
        with pytest.raises(rx.RtxError) as e:
            rx.ScreenSet.from_arrays(bases, off)
        assert e.value.code == _lib.RTX_ERR_INVALID, off
    assert rx.SCREEN_K == K and rx.SCREEN_NONE == NONE and rx.SCREEN_MAX_READ == 1 << 20


def test_a_set_from_fasta_text(genome):
    letters = {1: "A", 2: "C", 4: "G", 8: "T"}
    text = "".join(f">{name} some description\n{''.join(letters[int(c)] for c in seq)}\n" for name, seq in zip(("phage", "vector"), genome.seqs))
    from_text = rx.ScreenSet(text)
    assert from_text.labels[0].startswith("phage") and len(from_text.labels) == 2
    assert from_text.info() == genome.obj.info()                      # the same keys and sources: the same fingerprint
    lower = rx.ScreenSet(text.lower().replace(">phage", ">PHAGE"))    # the query parser reads lower case
    assert lower.info()["fingerprint"] == genome.obj.info()["fingerprint"]
    other = rx.ScreenSet([genome.seqs[1], genome.seqs[0]])            # the sources differ: another fingerprint
    assert other.info()["keys"] == genome.obj.info()["keys"] and other.info()["fingerprint"] != genome.obj.info()["fingerprint"]

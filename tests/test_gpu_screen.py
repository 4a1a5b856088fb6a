"""The contaminant screen on the device (rx.Screen, rtx_screen.hip) against the plain-Python restatement of tests/screen_common.py.  The kernel
gives a group of 16 lanes to a read; a lane's PIECE is 16 consecutive window positions (it loads the 16 bytes they start in and the 16
behind them), a STEP is the 16 pieces of the group, 256 positions.  So: lengths and planted stretches at +-1 of 16 and of 256 and of the
last window of either, stretches that straddle a piece or a step, breaking codes on either side of those borders, input ranges, a table
whose chains are long and wrap, a large table, and batches at +-1 of the reads of a wave (4) and of a block (16) through one object."""
import random

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth

from screen_common import (K, NONE, World, adversarial_world, concat, kmer_codes, large_reads, large_world, plant, random_codes, revcomp, screen_many,
                           screen_ref)

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 270, 271, 272, 511, 512, 513, 658, 5000]
OFFSETS = [0, 1, 15, 16, 17, 31, 32, 33, 239, 240, 241, 255, 256, 257, 270, 271, 272, 511, 512, 513, 658, 4979]
DEFAULT = rx.ScreenParams()
PARAMS = [DEFAULT, rx.ScreenParams(min_hits=1, min_pct=0), rx.ScreenParams(min_hits=3, min_pct=1), rx.ScreenParams(min_hits=1, min_pct=100)]


def _assert_equal(got, want, what):
    for name, g, w in zip(("windows", "hits", "first", "source", "verdict"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, f"{what}: {name} differs at reads {bad[:8].tolist()}: {np.asarray(g)[bad[:8]].tolist()} != {np.asarray(w)[bad[:8]].tolist()}"


@pytest.fixture(scope="module")
def genome():
    rng = random.Random(5386)
    return World([random_codes(rng, 5386), random_codes(rng, 300)])


@pytest.fixture(scope="module")
def reads(genome):
    """About 500 reads: random ones and pieces of the genome of every length, stretches of 16 + h - 1 genome bases (h = 1, 2, 3, either
    orientation) planted at every offset of OFFSETS in reads that end with the stretch, one base behind it or far behind it, the same with a
    breaking code one before, inside and one behind the stretch, homopolymer runs, and reads that are all N."""
    rng = random.Random(12)
    g = genome.seqs[0]
    out = []
    for n in LENGTHS:
        out += [random_codes(rng, n), g[200:200 + n].copy(), revcomp(g[300:300 + n])]
    k = 0
    for off in OFFSETS:
        for h in (1, 2, 3):
            for tail in (0, 1, 300):
                k += 1
                at = rng.randrange(1, 5386 - 40)
                codes = plant(random_codes(rng, off + K + h - 1 + tail), off, g, at, K + h - 1, rc=bool(k & 1))
                out.append(codes)
                if tail == 1:
                    for where, code in ((off - 1, 15), (off + rng.randrange(K + h - 1), 0), (off + K + h - 1, 5)):
                        if 0 <= where < len(codes):
                            broken = codes.copy()
                            broken[where] = code
                            out.append(broken)
    for b in range(4):
        out.append(np.full(40 + b, 1 << b, np.uint8))
    out += [np.full(300, 15, np.uint8), np.zeros(17, np.uint8), np.array([1, 2, 4, 8] * 4 + [3], np.uint8)]
    return out


def test_the_expectation_covers_what_it_should(genome, reads):
    one = rx.ScreenParams(min_hits=1, min_pct=0)
    windows, hits, first, source, verdict = screen_many(genome.ref, one, reads)
    lens = np.array([len(r) for r in reads])
    assert 400 <= len(reads) <= 600
    for off in OFFSETS:                                                          # a first hit at every offset, with 1, 2 and 3 hits
        for h in (1, 2, 3):
            assert ((first == off) & (hits == h)).any(), (off, h)
    assert ((hits == 0) & (windows > 0)).any() and ((windows == 0) & (lens >= 16)).any() and (windows[lens < 16] == 0).all()
    assert ((hits == windows) & (windows > 100)).any()                           # whole pieces of the genome
    assert (windows < np.maximum(lens - 15, 0)).sum() > 50                       # breaking codes took windows away
    assert set(source.tolist()) == {0, NONE}
    d = screen_many(genome.ref, DEFAULT, reads)[4]
    assert 0 < d.sum() < verdict.sum()


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_device_equals_the_restatement(genome, reads, k):
    p = PARAMS[k]
    bases, off = concat(reads)
    stage = rx.Screen(0, genome.obj, p)
    want = screen_many(genome.ref, p, reads)
    _assert_equal(stage.run(bases, off), want, "whole reads")
    assert stage.kernel_ms() > 0 and stage.stage_seconds()[2] > 0
    rev = reads[::-1]                                                            # the batch reversed, through the same object
    rb, ro = concat(rev)
    _assert_equal(stage.run(rb, ro), tuple(w[::-1] for w in want), "reversed")
    flipped = [revcomp(r) for r in reads]                                        # every read given the other way round
    fb, fo = concat(flipped)
    got = stage.run(fb, fo)
    _assert_equal(got, screen_many(genome.ref, p, flipped), "reverse complements")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4])


def test_batches_of_every_size_through_one_object(genome, reads):
    stage = rx.Screen(0, genome.obj, DEFAULT)
    rng = random.Random(2)
    for n in (257, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 0):
        part = [reads[rng.randrange(len(reads))] for _ in range(n)]
        bases, off = concat(part)
        got = stage.run(bases, off)
        assert all(len(g) == n for g in got)
        _assert_equal(got, screen_many(genome.ref, DEFAULT, part), f"batch of {n}")


def test_input_ranges(genome, reads):
    rng = random.Random(3)
    lo = np.array([rng.randint(0, len(r)) if i % 3 else min(len(r), 1 + i % 40) for i, r in enumerate(reads)], np.uint32)
    hi = np.array([rng.randint(int(a), len(r)) if i % 5 else int(a) for i, (a, r) in enumerate(zip(lo, reads))], np.uint32)   # every fifth range is empty
    assert (lo > 0).sum() > 300 and (hi == lo).sum() >= 80
    bases, off = concat(reads)
    for p in (DEFAULT, PARAMS[1]):
        want = screen_many(genome.ref, p, reads, lo, hi)
        assert (want[1] > 0).sum() > 30
        _assert_equal(rx.Screen(0, genome.obj, p).run(bases, off, lo, hi), want, "ranges")


def test_the_longest_read(genome):
    n = rx.SCREEN_MAX_READ
    rng = np.random.default_rng(4)
    codes = (np.uint8(1) << rng.integers(0, 4, n).astype(np.uint8)).astype(np.uint8)
    g = genome.seqs[0]
    for at in (0, 4090, 65536 + 255, n - 300):                                   # (4090: across a step)
        codes[at:at + 300] = g[1000:1300]
    codes[70000] = 15
    batch = [codes, random_codes(random.Random(1), 20), codes[:n - 1]]
    bases, off = concat(batch)
    p = rx.ScreenParams(min_hits=1, min_pct=0)
    want = screen_many(genome.ref, p, batch)
    assert want[0][0] == n - 15 - 16 and want[1][0] >= 4 * 285 and want[2][0] == 0
    _assert_equal(rx.Screen(0, genome.obj, p).run(bases, off), want, "2^20 bases")


def test_adversarial_table():
    world, keys, absent = adversarial_world()
    one = rx.ScreenParams(min_hits=1)
    singles = [kmer_codes(c) for c in keys + absent] + [revcomp(kmer_codes(c)) for c in keys + absent]
    joined = np.concatenate([np.concatenate([kmer_codes(c), [15]]) for c in absent[:8] + keys + absent[8:]]).astype(np.uint8)
    batch = singles + [joined, revcomp(joined)]
    bases, off = concat(batch)
    want = screen_many(world.ref, one, batch)
    assert want[1][:len(keys)].tolist() == [1] * len(keys) and want[1][len(keys):len(keys) + len(absent)].sum() == 0 and want[1][-2] == len(keys)
    assert want[3][:len(keys)].tolist() == list(range(len(keys)))
    _assert_equal(rx.Screen(0, world.obj, one).run(bases, off), want, "chains across the wrap")


def test_large_table():
    obj, ref, members, others = large_world()
    one = rx.ScreenParams(min_hits=1)
    batch = large_reads(members, others)
    bases, off = concat(batch)
    want = screen_many(ref, one, batch)
    assert int(want[1].sum()) == 200_000 + 4096
    stage = rx.Screen(0, obj, one)
    _assert_equal(stage.run(bases, off), want, "200 000 keys")
    print(f"large table: {len(batch)} reads, kernel {stage.kernel_ms():.3f} ms")


def test_realistic_mix(genome):
    """2 000 reads of 150-300 bases cut from the 5 386-base genome in either orientation with 0-3 substitutions, mixed with 2 000 reads of the
    synthetic COI database: under the defaults the restatement flags every genome read and no database read, and the device says the same."""
    rng = np.random.default_rng(8)
    g = genome.seqs[0]
    batch, is_genome = [], []
    db = synth.make_db(400)
    qs = synth.make_queries(db, 2000, seed=9)
    for i in range(2000):
        n = int(rng.integers(150, 301))
        at = int(rng.integers(0, 5386 - n))
        r = g[at:at + n].copy()
        for pos in rng.integers(0, n, int(rng.integers(0, 4))):
            r[pos] = {1: 2, 2: 4, 4: 8, 8: 1}[int(r[pos])]
        batch += [revcomp(r) if i & 1 else r, qs.seq(i)]
        is_genome += [True, False]
    is_genome = np.array(is_genome)
    want = screen_many(genome.ref, DEFAULT, batch)
    assert (want[4][is_genome] == 1).all() and (want[4][~is_genome] == 0).all()
    assert (want[1][~is_genome] == 0).all() and (want[1][is_genome] >= 150 - 15 - 3 * 16).all()
    bases, off = concat(batch)
    stage = rx.Screen(0, genome.obj, DEFAULT)
    _assert_equal(stage.run(bases, off), want, "genome reads among barcodes")
    print(f"realistic mix: 4000 reads, kernel {stage.kernel_ms():.3f} ms, stage {stage.stage_seconds()}")


def test_invalid_arguments(genome):
    stage = rx.Screen(0, genome.obj, DEFAULT)
    bases = np.full(16, 1, np.uint8)
    cases = [
        dict(base_off=np.array([0, 8, 4, 16], np.uint64)),                                                              # base_off not monotone
        dict(base_off=np.array([0, 8, 16], np.uint64), lo=np.array([0, 9], np.uint32), hi=np.array([8, 9], np.uint32)),  # a range outside its read
        dict(base_off=np.array([0, 8, 16], np.uint64), lo=np.array([5, 0], np.uint32), hi=np.array([4, 8], np.uint32)),
    ]
    for kw in cases:
        with pytest.raises(rx.RtxError) as e:
            stage.run(bases, **kw)
        assert e.value.code == _lib.RTX_ERR_INVALID
    n = rx.SCREEN_MAX_READ + 1                                                                                           # an over-long read
    with pytest.raises(rx.RtxError) as e:
        stage.run(np.full(n, 1, np.uint8), np.array([0, n], np.uint64))
    assert e.value.code == _lib.RTX_ERR_INVALID
    for p in (rx.ScreenParams(min_hits=0), rx.ScreenParams(min_pct=101)):
        with pytest.raises(rx.RtxError) as e:
            rx.Screen(0, genome.obj, p)
        assert e.value.code == _lib.RTX_ERR_INVALID
    got = stage.run(bases, np.array([0, 16], np.uint64))                                                                 # the object still works
    assert [int(x[0]) for x in got] == list(screen_ref(genome.ref, DEFAULT, bases))

"""What the front stage objects share (csrc/rtx_stage.hpp, csrc/host_stage.hpp) on the device path, where the direct stage tests do not reach
with their few hundred reads:

  1. trim, demux, qual, screen: a batch of more than 8 192 reads -- the host stages it on two threads or more -- through one object, held
     against the expectation of 41 reads tiled (a read's values never depend on its batch); qual and screen once with whole reads and once
     with [lo, hi) ranges; then three empty reads through the same object: no piece, nothing to upload;
  2. derep, chimera: the packed upload they share, three batches through one object each: every read empty, an odd number of bases in all,
     and a byte above 15 (the batch travels unpacked).

Every expectation comes from the restatements of tests/*_common.py (rx.chimera_read and a dict of first indices for the last two) on the small
batch, computed once per module.  No tolerance anywhere.  (tests/test_gpu_derep.py::test_raw_bytes runs the unpacked path on a fresh object;
here it follows a packed batch on the same one.)"""
import random

import numpy as np
import pytest

import chimera_common as cc
import demux_common as dx
import raxtax_amd as rx
from qual_common import qual_many
from raxtax_amd import _lib, synth
from screen_common import K, World, plant, random_codes, screen_many
from trim_common import trim_many

pytestmark = pytest.mark.gpu

SMALL, TIMES = 41, 200    # 8 200 reads: more than two grains of 4 096
EMPTY = np.zeros(0, np.uint8)


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    flat = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [EMPTY])
    return flat, off


def tiled(flat, off):
    """The batch TIMES times over: (bases, base_off)."""
    total = off[-1]
    offs = (off[:-1][None, :] + (np.arange(TIMES, dtype=np.uint64) * total)[:, None]).reshape(-1)
    return np.tile(flat, TIMES), np.concatenate([offs, np.array([total * np.uint64(TIMES)], np.uint64)])


def assert_equal(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: column {k} differs at reads {bad[:8].tolist()}: {g[bad[:8]].tolist()} != {w[bad[:8]].tolist()}"


def tile_columns(want):
    return tuple(np.tile(np.asarray(w), TIMES) for w in want)


def ranges_of(reads, seed):
    """[lo, hi) inside every read: every fifth range empty, every seventh the whole read, one that ends on the last byte of the batch."""
    rng = random.Random(seed)
    lo = np.array([rng.randint(0, len(r)) if i % 7 else 0 for i, r in enumerate(reads)], np.uint32)
    hi = np.array([int(a) if i % 5 == 0 and i % 7 else (len(r) if i % 7 == 0 else rng.randint(int(a), len(r))) for i, (a, r) in enumerate(zip(lo, reads))], np.uint32)
    hi[-1] = len(reads[-1])
    assert (hi == lo).sum() >= 5 and (lo > 0).sum() >= 20 and len(reads[-1]) > 0
    return lo, hi


def seq(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the stages that stage per read
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trim_large_batch_and_empty_reads():
    rng = np.random.default_rng(141)
    f20, r20, f33 = seq(rng, 20), seq(rng, 20), seq(rng, 33)
    pats = [rx.TrimPrimer(f20, rx.TRIM_5P, 2), rx.TrimPrimer(f33, rx.TRIM_5P, 3), rx.TrimPrimer(r20, rx.TRIM_3P, 2)]
    reads = [np.concatenate([f20, seq(rng, 300), r20]), EMPTY, seq(rng, 1), f20.copy(), np.concatenate([f20, r20]), np.concatenate([f33, seq(rng, 15)])]
    while len(reads) < SMALL:
        k = len(reads)
        a, b = (f20 if k % 2 else f33).copy(), r20.copy()
        a[int(rng.integers(0, len(a)))] = int(rng.choice([1, 2, 4, 8, 15, 0x20]))
        reads.append(np.concatenate([a] * (k % 5 != 0) + [seq(rng, int(rng.integers(15, 400)))] + [b] * (k % 3 != 0)))
    want = trim_many(pats, reads)
    assert ((want[2] & 0xFF) != 0xFF).sum() >= 20 and (((want[2] >> 16) & 0xFF) != 0xFF).sum() >= 20
    stage = rx.Trim(0, pats)
    assert_equal(stage.run(*tiled(*concat(reads))), tile_columns(want), "trim, 8 200 reads")
    assert stage.kernel_ms() > 0
    assert_equal(stage.run(*concat([EMPTY] * 3)), trim_many(pats, [EMPTY] * 3), "trim, three empty reads")
    assert_equal(stage.run(*concat(reads)), want, "trim, the small batch behind them")


def test_demux_large_batch_and_empty_reads():
    lists, shared_reads = dx.shared()
    tags, pairs = lists.lists["l96"]
    reads = shared_reads[:SMALL]
    mm, max_offset = 3, 15
    want = dx.demux_ref(tags, pairs, mm, max_offset, reads)[:5]
    assert (want[0] != dx.NONE).sum() >= 10 and len(set((want[4] & 0xFF).tolist())) >= 3
    stage = rx.Demux(0, tags, pairs, rx.DemuxParams(mm, max_offset))
    assert_equal(stage.run(*tiled(*concat(reads))), tile_columns(want), "demux, 8 200 reads")
    assert stage.kernel_ms() > 0
    assert_equal(stage.run(*concat([EMPTY] * 3)), dx.demux_ref(tags, pairs, mm, max_offset, [EMPTY] * 3)[:5], "demux, three empty reads")
    assert_equal(stage.run(*concat(reads)), want, "demux, the small batch behind them")


def test_qual_large_batch_ranges_and_empty_reads():
    rng = random.Random(142)
    p = rx.QualParams(trunc_len=400, trunc_qual=2, trunc_ee=0.9, min_len=16, max_len=380, max_ns=2, max_ee=0.5, max_ee_rate=0.002)
    pairs = []
    for n in [0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513] + [rng.randint(20, 658) for _ in range(SMALL - 11)]:
        b = np.array([rng.choice([1, 2, 4, 8]) for _ in range(n)], np.uint8)
        q = np.array([33 + rng.randint(30, 41) for _ in range(n)], np.uint8)
        k = len(pairs)
        if n > 20 and k % 3 == 0:
            q[rng.randrange(n)] = 33 + rng.randint(0, 2)          # a cut of trunc_qual
        if n > 20 and k % 4 == 1:
            at = rng.randrange(1, n)
            q[at - 1] = q[at] = 33 + 3                            # a cut of trunc_ee
            b[max(0, at - 3):at] = 15
        if n > 20 and k % 13 == 5:
            q[n - 1] = 32                                         # a byte below the base
        pairs.append((b, q))
    reads, quals = [b for b, _ in pairs], [q for _, q in pairs]
    want = qual_many(p, reads, quals)
    assert len(set(want[2].tolist())) >= 4 and (want[0] < np.array([len(r) for r in reads])).sum() >= 10
    lo, hi = ranges_of(reads, 143)
    want_r = qual_many(p, reads, quals, lo, hi)
    assert any(not np.array_equal(a, b) for a, b in zip(want, want_r))
    (bases, off), (qb, _) = concat(reads), concat(quals)
    big_b, big_off = tiled(bases, off)
    stage = rx.Qual(0, p)
    assert_equal(stage.run(big_b, np.tile(qb, TIMES), big_off), tile_columns(want), "qual, 8 200 reads")
    assert stage.kernel_ms() > 0 and stage.stage_seconds()[2] >= stage.stage_seconds()[0] > 0
    assert_equal(stage.run(big_b, np.tile(qb, TIMES), big_off, np.tile(lo, TIMES), np.tile(hi, TIMES)), tile_columns(want_r), "qual, 8 200 ranges")
    assert_equal(stage.run(EMPTY, EMPTY, np.zeros(4, np.uint64)), qual_many(p, [EMPTY] * 3, [EMPTY] * 3), "qual, three empty reads")
    assert stage.stage_seconds()[2] > 0
    zero = np.zeros(3, np.uint32)
    assert_equal(stage.run(EMPTY, EMPTY, np.zeros(4, np.uint64), zero, zero), qual_many(p, [EMPTY] * 3, [EMPTY] * 3), "qual, three empty ranges")
    assert_equal(stage.run(bases, qb, off, lo, hi), want_r, "qual, the small batch behind them")


def test_screen_large_batch_ranges_and_empty_reads():
    rng = random.Random(144)
    world = World([random_codes(rng, 2000), random_codes(rng, 300)])
    g = world.seqs[0]
    reads = [EMPTY, random_codes(rng, 15), g[100:116].copy(), g[200:217].copy(), random_codes(rng, 300), np.full(40, 15, np.uint8)]
    while len(reads) < SMALL:
        k = len(reads)
        at_read, n = rng.choice([0, 1, 15, 16, 17, 239, 240, 241, 255, 256, 257]), K + rng.randrange(3)
        codes = plant(random_codes(rng, at_read + n + rng.choice([0, 1, 300])), at_read, g, rng.randrange(1, 2000 - 40), n, rc=bool(k & 1))
        if k % 6 == 0:
            codes[rng.randrange(len(codes))] = 15
        reads.append(codes)
    p = rx.ScreenParams(min_hits=1, min_pct=0)
    want = screen_many(world.ref, p, reads)
    assert (want[1] > 0).sum() >= 20 and (want[1] == 0).sum() >= 4
    lo, hi = ranges_of(reads, 145)
    want_r = screen_many(world.ref, p, reads, lo, hi)
    assert (want_r[1] > 0).sum() >= 5 and not np.array_equal(want[1], want_r[1])
    bases, off = concat(reads)
    big_b, big_off = tiled(bases, off)
    stage = rx.Screen(0, world.obj, p)
    assert_equal(stage.run(big_b, big_off), tile_columns(want), "screen, 8 200 reads")
    assert stage.kernel_ms() > 0 and stage.stage_seconds()[2] >= stage.stage_seconds()[0] > 0
    assert_equal(stage.run(big_b, big_off, np.tile(lo, TIMES), np.tile(hi, TIMES)), tile_columns(want_r), "screen, 8 200 ranges")
    assert_equal(stage.run(EMPTY, np.zeros(4, np.uint64)), screen_many(world.ref, p, [EMPTY] * 3), "screen, three empty reads")
    assert stage.stage_seconds()[2] > 0
    zero = np.zeros(3, np.uint32)
    assert_equal(stage.run(EMPTY, np.zeros(4, np.uint64), zero, zero), screen_many(world.ref, p, [EMPTY] * 3), "screen, three empty ranges")
    assert_equal(stage.run(bases, off, lo, hi), want_r, "screen, the small batch behind them")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the packed upload of derep and chimera
# ---------------------------------------------------------------------------------------------------------------------------------
def packed_batches(seqs):
    """(name, reads) x 3: every read empty; an odd number of bases in all; the same with one byte above 15 (not packed)."""
    seqs = [s.copy() for s in seqs]
    if sum(len(s) for s in seqs) % 2 == 0:
        seqs[0] = seqs[0][:-1]
    raw = [s.copy() for s in seqs]
    raw[1][len(raw[1]) // 2] = 0x20
    bases = concat(raw)[0]
    assert len(bases) % 2 == 1 and _lib.load().rtx_pack_bases(_lib.ptr(bases, _lib.u8p), len(bases), _lib.ptr(np.zeros(len(bases), np.uint8), _lib.u8p)) == 0
    return [("every read empty", [EMPTY] * 3), ("an odd number of bases", seqs), ("a byte above 15", raw), ("an odd number of bases, again", seqs)]


def test_derep_packed_upload_through_one_object():
    rng = np.random.default_rng(146)
    distinct = [seq(rng, n) for n in (1, 7, 8, 9, 63, 64, 65, 300, 301)]
    seqs = [distinct[i] for i in rng.integers(0, len(distinct), 30)] + [EMPTY, distinct[3], EMPTY]
    batches = packed_batches(seqs)
    d = rx.Derep()
    for name, batch in batches:
        seen, want = {}, np.zeros(len(batch), np.uint32)
        for q, s in enumerate(batch):
            want[q] = seen.setdefault(bytes(s), q)
        rep = d.run(*concat(batch))
        assert np.array_equal(rep, want), (name, rep.tolist(), want.tolist())
        assert d.n_unique == len(seen), (name, d.n_unique, len(seen))
        uniq, slot, size = rx.derep_plan(rep)
        assert uniq.tolist() == sorted(seen.values()) and int(size.sum()) == len(batch) and np.array_equal(uniq[slot], want), name


def test_chimera_packed_upload_through_one_object():
    db = synth.make_db(300)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    ref_bases, ref_off = cc.tree_order(db, tree)
    chim, _ = cc.planted_chimeras(db, n=4, seed=7)
    seqs = chim + [db.seq(5).copy(), EMPTY, db.seq(9)[:40].copy(), db.seq(11)[:7].copy()]
    params = rx.ChimeraParams()
    batches = [(name, batch, [rx.chimera_read(params, s, ref_bases, ref_off) for s in batch]) for name, batch in packed_batches(seqs)]
    assert all(sum(int(w["flag"]) for w in want) >= 3 for name, _, want in batches if "empty" not in name)   # (the planted chimeras are found: more than empty records are compared)
    stage = rx.Chimera(rx.Index(tree), params)
    for name, batch, want in batches:
        got = stage.run(*concat(batch))
        assert len(got) == len(batch)
        for i, s in enumerate(batch):
            assert cc.as_tuple(got[i]) == cc.as_tuple(want[i]), (name, i, len(s), cc.as_tuple(got[i]), cc.as_tuple(want[i]))
    assert stage.kernel_ms() > 0

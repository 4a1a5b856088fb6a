"""The distinct reads of a run on the device (rtx_tally.hip).  The expected table everywhere is a Python dict over bytes(seq)
(tally_common.expected_table), which test_tally_cpu.py holds against rx.tally_reads on a hand-written example; here the device is held
against both.  No tolerance anywhere."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from tally_common import concat, edge_reads, expected_table

pytestmark = pytest.mark.gpu

SILENT = 37          # a sequence that is only ever seen with weight 0
LATE2, LATE3 = 38, 39  # sequences that first appear in the second and in the third add


@pytest.fixture(scope="module")
def edges():
    """(seqs, weight, cuts): the 330 edge reads in three adds.  Sequence 38 first appears in the second add, 39 in the third; every read of
    sequence 37 has weight 0, and so have a few reads of sequences that count elsewhere."""
    distinct, picks = edge_reads()
    rng = np.random.default_rng(42)
    rest = [p for p in picks if p not in (LATE2, LATE3)]
    n2, n3 = picks.count(LATE2), picks.count(LATE3)
    adds = [rest[:110], rest[110:215], rest[215:]]
    for _ in range(n2):
        k = 1 + int(rng.integers(0, 2))
        adds[k].insert(int(rng.integers(0, len(adds[k]) + 1)), LATE2)
    if LATE2 not in adds[1]:
        adds[1].insert(50, LATE2)
        adds[2].remove(LATE2)
    for _ in range(n3):
        adds[2].insert(int(rng.integers(0, len(adds[2]) + 1)), LATE3)
    order = adds[0] + adds[1] + adds[2]
    assert len(order) == 330 and n2 >= 2 and n3 >= 1
    cuts = [0, len(adds[0]), len(adds[0]) + len(adds[1]), 330]
    seqs = [distinct[i] for i in order]
    weight = np.ones(330, np.uint32)
    weight[[i for i, p in enumerate(order) if p == SILENT]] = 0
    weight[[5, 120, 121, 300]] = 0
    assert order[5] != SILENT and order.count(order[5]) > 1
    # copies within an add and copies across adds
    first, second = set(adds[0]), set(adds[1])
    assert any(adds[0].count(p) > 1 for p in first) and first & second and first & set(adds[2])
    return seqs, weight, cuts


def add_all(t, seqs, cuts, sample=None, weight=None):
    for a, b in zip(cuts[:-1], cuts[1:]):
        t.add(*concat(seqs[a:b]), None if sample is None else sample[a:b], None if weight is None else weight[a:b])


def assert_table(table, want, reads=None, overflow=0):
    got = table.as_dict()
    assert got.keys() == want.keys(), (len(got), len(want))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, [(len(k), got[k], want[k]) for k in bad[:5]]
    assert table.totals == {"reads": sum(map(sum, want.values())) + overflow if reads is None else reads, "entries": len(want), "overflow_reads": overflow}
    # rows: size descending, then bytes ascending
    keys = [(-sum(want[bytes(s)]), bytes(s)) for s in table.seqs]
    assert keys == sorted(keys)


def assert_equal_tables(a, b):
    assert [bytes(s) for s in a.seqs] == [bytes(s) for s in b.seqs]
    assert np.array_equal(a.counts, b.counts) and a.totals == b.totals


def test_three_adds(edges):
    seqs, weight, cuts = edges
    want = expected_table(seqs, None, weight)
    assert len(want) == 38                                             # 40, but for the empty sequence and the silent one
    counting = [bytes(s) if w else b"" for s, w in zip(seqs, weight)]
    assert any(k and k not in counting[:cuts[1]] for k in counting[cuts[1]:cuts[2]])       # a sequence that first appears in the second add ...
    assert any(k and k not in counting[:cuts[2]] for k in counting[cuts[2]:])              # ... and one in the third
    silent = {bytes(s) for s, w in zip(seqs, weight) if w == 0 and len(s)} - want.keys()
    assert len(silent) == 1                                            # seen, never counted: no entry
    t = rx.Tally()
    add_all(t, seqs, cuts, weight=weight)
    table = t.read()
    assert_table(table, want)
    assert_equal_tables(table, rx.tally_reads(*concat(seqs), None, weight))
    # entry ids are the order of first appearance (of the reads that count)
    by_first = [bytes(table.seqs[r]) for r in np.argsort(table.first)]
    assert sorted(table.first) == list(range(38)) and by_first == list(want)
    assert t.info()["entries"] == 38 and t.info()["counted"] == int(weight[[i for i, s in enumerate(seqs) if len(s)]].sum())
    # the object goes on counting after a read
    t.add(*concat(seqs[:7]))
    again = t.read().as_dict()
    more = expected_table(seqs[:7])
    assert all(sum(again[k]) == sum(want.get(k, (0,))) + sum(more.get(k, (0,))) for k in again) and set(again) == set(want) | set(more)


def test_forced_collisions(edges):
    seqs, weight, cuts = edges
    lib = _lib.load()
    _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_TALLY_HASH_MASK, 3))
    try:
        t = rx.Tally()
        add_all(t, seqs, cuts, weight=weight)      # every probe ends in the byte compare, the chains run across the adds
        assert_table(t.read(), expected_table(seqs, None, weight))
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_TALLY_HASH_MASK, 0))
    # the mask is read at every add: the same object under the full hash lays its table out again and finds every entry
    t.add(*concat(seqs), None, weight)
    want2 = {k: (2 * v[0],) for k, v in expected_table(seqs, None, weight).items()}
    assert_table(t.read(), want2)


def test_growth(edges):
    seqs, weight, cuts = edges
    t = rx.Tally(initial_entries=4, initial_bytes=64)
    assert t.info()["entry_capacity"] == 4 and t.info()["byte_capacity"] == 64
    add_all(t, seqs, cuts, weight=weight)
    info = t.info()
    assert info["entry_capacity"] >= 38 > 4 and info["byte_capacity"] >= info["bytes"] > 64
    assert info["bytes"] == sum((len(k) + 7) // 8 * 8 for k in expected_table(seqs, None, weight))
    table = t.read()
    assert_table(table, expected_table(seqs, None, weight))
    big = rx.Tally()
    add_all(big, seqs, cuts, weight=weight)
    assert_equal_tables(table, big.read())
    assert np.array_equal(table.first, big.read().first)
    # one read at a time: the table is laid out again and again, and the arena grows under entries in use
    one = rx.Tally(initial_entries=1, initial_bytes=8)
    add_all(one, seqs[:60], list(range(61)), weight=weight[:60])
    assert_table(one.read(), expected_table(seqs[:60], None, weight[:60]))


def capped(seqs, weight, cuts, max_entries=1 << 40, max_bytes=1 << 60):
    """The rule of the caps restated: per add, the new distinct reads in read order; one is stored iff its inclusive position -- entries and
    padded bytes, on top of what is in use -- is within both caps.  (stored table, overflow_reads)"""
    stored, overflow, used_b = {}, 0, 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        pos_e = pos_b = 0
        now = {}                     # the new distinct reads of this add: stored or not
        for q in range(a, b):
            k, w = bytes(seqs[q]), int(weight[q])
            if w == 0 or not k:
                continue
            if k not in stored and k not in now:
                pos_e, pos_b = pos_e + 1, pos_b + (len(k) + 7) // 8 * 8
                now[k] = len(stored) + pos_e <= max_entries and used_b + pos_b <= max_bytes
            if k in stored or now[k]:
                pass
            else:
                overflow += w
        for q in range(a, b):        # (counted in a second pass: `stored` must not change under the scan)
            k, w = bytes(seqs[q]), int(weight[q])
            if w and k and (k in stored or now[k]):
                stored.setdefault(k, [0])[0] += w
        used_b = sum((len(k) + 7) // 8 * 8 for k in stored)
    return {k: tuple(v) for k, v in stored.items()}, overflow


def test_caps(edges):
    seqs, weight, cuts = edges
    full = expected_table(seqs, None, weight)
    appear = list(full)
    # entries: the first 10 to appear are stored, the weight of the rest overflows -- also when it is presented again in a later add
    want, overflow = capped(seqs, weight, cuts, max_entries=10)
    assert list(want) == appear[:10] and overflow == sum(full[k][0] for k in appear[10:]) and all(want[k] == full[k] for k in want)
    later = [bytes(s) for s in seqs[cuts[1]:]]
    assert any(k in later for k in appear[10:]) and any(k in later for k in appear[:10])
    t = rx.Tally(max_entries=10)
    add_all(t, seqs, cuts, weight=weight)
    table = t.read()
    assert_table(table, want, overflow=overflow)
    assert t.info()["entries"] == 10 and t.info()["entry_capacity"] <= 10
    assert [bytes(table.seqs[r]) for r in np.argsort(table.first)] == appear[:10]
    # bytes: the cap cuts in the middle of the first add's new reads, and leaves less than one word of room
    pad = [(len(k) + 7) // 8 * 8 for k in appear]
    max_bytes = sum(pad[:12]) + 7
    want, overflow = capped(seqs, weight, cuts, max_bytes=max_bytes)
    assert list(want) == appear[:12] and overflow == sum(full[k][0] for k in appear[12:])
    t = rx.Tally(max_bytes=max_bytes, initial_bytes=64)
    add_all(t, seqs, cuts, weight=weight)
    assert_table(t.read(), want, overflow=overflow)
    assert t.info()["bytes"] == sum(pad[:12]) and t.info()["byte_capacity"] <= max_bytes
    # a cap that a later, shorter read still fits under: the rule is the scan position of the add, and the restatement follows it
    max_bytes = sum(pad[:12]) + 64
    want, overflow = capped(seqs, weight, cuts, max_bytes=max_bytes)
    assert len(want) > 12 and overflow > 0
    t = rx.Tally(max_bytes=max_bytes)
    add_all(t, seqs, cuts, weight=weight)
    assert_table(t.read(), want, overflow=overflow)


def test_samples(edges):
    seqs, _, cuts = edges
    rng = np.random.default_rng(43)
    sample = rng.integers(0, 3, 330).astype(np.uint32)
    weight = rng.choice([0, 1, 5], 330).astype(np.uint32)
    sample[weight == 0] = rx.DEMUX_NONE                      # nobody looks at the sample of a read that does not count
    want = expected_table(seqs, sample, weight, 3)
    assert {c for v in want.values() for c in v} >= {0, 1, 5, 6} and all(any(v[s] for v in want.values()) for s in range(3))
    t = rx.Tally(samples=3)
    add_all(t, seqs, cuts, sample, weight)
    table = t.read()
    assert table.columns == 3
    assert_table(table, want)
    assert_equal_tables(table, rx.tally_reads(*concat(seqs), sample, weight, samples=3))


def test_order_independence(edges):
    seqs, weight, cuts = edges
    rng = np.random.default_rng(44)
    sample = rng.integers(0, 2, 330).astype(np.uint32)
    a = rx.Tally(samples=2)
    add_all(a, seqs, cuts, sample, weight)
    perm = rng.permutation(330)
    b = rx.Tally(samples=2, initial_entries=8)
    add_all(b, [seqs[i] for i in perm], [0, 1, 2, 60, 61, 257, 330], sample[perm], weight[perm])
    assert_equal_tables(a.read(), b.read())
    assert not np.array_equal(a.read().first, b.read().first)


def test_raw_bytes(edges):
    seqs, weight, cuts = edges
    seqs = [s.copy() for s in seqs]
    k = next(i for i, s in enumerate(seqs) if len(s) == 658 and weight[i])
    seqs[k][100] = 0x20    # no code of the parser: the add it is in travels as raw bytes
    t = rx.Tally()
    add_all(t, seqs, cuts, weight=weight)
    assert_table(t.read(), expected_table(seqs, None, weight))


def test_refusals(edges):
    seqs, weight, cuts = edges
    lib = _lib.load()
    with pytest.raises(rx.RtxError) as e:
        rx.Tally(device=lib.rtx_device_count())
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE
    with pytest.raises(rx.RtxError) as e:
        rx.Tally(max_entries=1 << 31)
    assert e.value.code == _lib.RTX_ERR_INVALID
    # a sample out of range: nothing is enqueued, the table is what it was
    t = rx.Tally(samples=2)
    sample = np.zeros(330, np.uint32)
    add_all(t, seqs, cuts, sample, weight)
    before, info = t.read(), t.info()
    bad = sample.copy()
    bad[next(i for i in range(329, 0, -1) if weight[i] and len(seqs[i]))] = 2
    with pytest.raises(rx.RtxError) as e:
        t.add(*concat(seqs), bad, weight)
    assert e.value.code == _lib.RTX_ERR_INVALID and "sample 2" in str(e.value)
    with pytest.raises(rx.RtxError) as e:
        t.add(*concat([s for s in seqs if len(s)][:4]), None, np.array([0xFFFFFFFF, 0xFFFFFFFF, 1, 1], np.uint32))   # a cell could wrap
    assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError):
        t.add(np.zeros(16, np.uint8), np.array([0, 8, 4, 16], np.uint64))
    assert t.info() == info
    assert_equal_tables(t.read(), before)
    # handles: the tally's device is the handle's; on every handle of a call or on none; never one object on two handles
    db = synth.make_db(300)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    queries = [(f"q{i}", db.seq(i).copy()) for i in range(8)]
    with_tally, without = rx.Index(tree, tally=rx.Tally()), rx.Index(tree)
    assert with_tally.tally is not None and without.tally is None
    if lib.rtx_device_count() > 1:
        with pytest.raises(rx.RtxError) as e:
            without.set_tally(rx.Tally(device=1))
        assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(queries, [with_tally, without], False, False, 4, lambda *a: None, False)
    assert e.value.code == _lib.RTX_ERR_INVALID and "rtx_index_set_tally" in str(e.value)
    without.set_tally(with_tally.tally)
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(queries, [with_tally, without], False, False, 4, lambda *a: None, False)
    assert e.value.code == _lib.RTX_ERR_INVALID and "share" in str(e.value)
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax(queries, rx.Index(tree, tally=rx.Tally(samples=2)), False, False, 4, lambda *a: None, False)   # samples without tags
    assert e.value.code == _lib.RTX_ERR_INVALID and "n_samples" in str(e.value)
    assert with_tally.tally.read().totals["reads"] == 0        # none of the refused calls counted anything
    without.set_tally(None)
    assert without.tally is None

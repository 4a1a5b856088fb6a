"""Sample demultiplexing on the device (rtx_demux.hip).  The expected values everywhere come from the numpy restatement of
tests/demux_common.py (loops over tags and offsets, nothing packed, no code of the library); exact integers, no tolerance.  The lists: 1, 2,
96 and 1024 tags per end, one with tags of 1, 8, 16, 17 and 32 codes (the 64-bit word boundary sits at 16), one end alone; the 257 reads
and what they hold: demux_common.Lists.reads."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from demux_common import AMBIGUOUS, NO_TAG3, NO_TAG5, NONE, OK, UNKNOWN_PAIR, concat, expected, shared

pytestmark = pytest.mark.gpu
NAMES = ("sample", "lo", "hi", "hit", "info")


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g, np.uint32), np.asarray(w, np.uint32)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:8]}: device {g[bad[:8]]}, expected {w[bad[:8]]}"


def stage(name, mm, off):
    lists, _ = shared()
    tags, pairs = lists.lists[name]
    return rx.Demux(0, tags, pairs, rx.DemuxParams(mm, off))


def test_the_expectation_holds_every_kind():
    sample, lo, hi, hit, info, d5, d3 = expected("l96", 3, 15)
    _, reads = shared()
    verdict = info & 0xFF
    length = np.array([len(r) for r in reads])
    assert set(np.unique(verdict)) == {OK, NO_TAG5, NO_TAG3, AMBIGUOUS, UNKNOWN_PAIR}
    assert ((hi == lo) & (lo > 0) & (lo < length)).any() and ((hi == lo) & (hi == length)).any()      # cuts that overlap; nothing cut of nothing
    assert length.max() == 5000 and (length == 0).any()
    for d in (d5, d3):                                                   # as many substitutions as allowed, and one more
        assert (d == 3).any() and (d == 4).any()


def test_batches_of_every_size_on_one_object():
    _, reads = shared()
    want = expected("l96", 3, 15)[:5]
    d = stage("l96", 3, 15)
    for n in (257, 1, 63, 64, 65):                                       # (the buffers of the largest batch are reused by the smaller ones)
        assert_equal(d.run(*concat(reads[:n])), [w[:n] for w in want], f"{n} reads")
    assert_equal(d.run(*concat(reads[::-1])), [w[::-1] for w in want], "the batch reversed: a read's values do not depend on its batch")
    got = d.run(*concat([]))
    assert all(len(g) == 0 for g in got)
    assert d.kernel_ms() >= 0.0


@pytest.mark.parametrize("name,mm,off", [("l1", 0, 0), ("l1", 3, 15), ("l2", 3, 1), ("l1024", 2, 3), ("l1024", 1, 15), ("mixed", 0, 0), ("mixed", 1, 15),
                                         ("mixed", 8, 1), ("only5", 3, 15), ("only3", 1, 1)])
def test_every_list(name, mm, off):
    _, reads = shared()
    assert_equal(stage(name, mm, off).run(*concat(reads)), expected(name, mm, off)[:5], f"{name} {mm} {off}")


@pytest.mark.parametrize("mm", [0, 1, 3, 8])
@pytest.mark.parametrize("off", [0, 1, 15])
def test_every_parameter(mm, off):
    _, reads = shared()
    assert_equal(stage("l96", mm, off).run(*concat(reads)), expected("l96", mm, off)[:5], f"l96 {mm} {off}")


def test_invalid_arguments():
    d = stage("l2", 0, 0)
    with pytest.raises(rx.RtxError) as e:
        d.run(np.zeros(16, np.uint8), np.array([0, 8, 4, 16], np.uint64))   # base_off not monotone
    assert e.value.code == _lib.RTX_ERR_INVALID
    lib = _lib.load()
    z32, off = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
    p32 = z32.ctypes.data_as(_lib.u32p)
    rc = lib.rtx_demux_run(d._h, (1 << 31) - 1, np.zeros(1, np.uint8).ctypes.data_as(_lib.u8p), off.ctypes.data_as(_lib.u64p), p32, p32, p32, p32, p32)
    assert rc == _lib.RTX_ERR_INVALID                                    # more than 2^31 - 2 reads: refused before anything is read
    lists, _ = shared()
    tags, pairs = lists.lists["l2"]
    for bad_tags, bad_pairs, params in (([], [], (0, 0)), ([(np.array([1, 0, 2], np.uint8), 0)], [], (0, 0)), (tags, pairs, (9, 0)), (tags, pairs, (0, 16)),
                                        (tags, [(2, 0, 0)], (0, 0)), (tags, pairs + pairs[:1], (0, 0))):
        with pytest.raises(rx.RtxError) as e:
            rx.Demux(0, bad_tags, bad_pairs, params)
        assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.Demux(99, tags, pairs, (0, 0))
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE

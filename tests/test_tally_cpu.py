"""The distinct reads of a run, the parts that run without a GPU: the host table (rx.tally_reads, the restatement of Tally.add), its
order, the merge, the two formatters and their need / cap protocol, the refusals and the constants.  Every expected table is a Python
dict over bytes(seq).  No tolerance anywhere."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from tally_common import concat, expected_table

ROOT = Path(__file__).resolve().parent.parent

A, Cc, G, T = 1, 2, 4, 8


def seq(*codes):
    return np.array(codes, np.uint8)


def test_constants_and_binding_are_the_header_s():
    text = (ROOT / "include" / "raxtax_hip.h").read_text()
    defs = dict(re.findall(r"^#define (RTX_[A-Z_]+) (\d+)\b", text, flags=re.M))
    assert int(defs["RTX_DEFAULT_TALLY_HASH_MASK"]) == _lib.RTX_DEFAULT_TALLY_HASH_MASK == 4
    assert int(defs["RTX_DEFAULT_DEREP_HASH_MASK"]) == 3
    assert int(defs["RTX_ABI_VERSION"]) == 6 and _lib.load().rtx_abi_version() == 6
    assert _lib.load().rtx_set_default_option(_lib.RTX_DEFAULT_TALLY_HASH_MASK, 0) == 0
    for name in ("rtx_tally_create", "rtx_tally_add", "rtx_tally_read", "rtx_tally_destroy", "rtx_tally_table_create", "rtx_tally_table_add", "rtx_tally_table_merge",
                 "rtx_tally_table_view", "rtx_tally_table_destroy", "rtx_tally_format_fasta", "rtx_tally_format_table", "rtx_index_set_tally", "rtx_index_tally",
                 "rtx_raxtax_last_tally"):
        assert name in _lib._SIGNATURES and re.search(rf"\b{name}\(", text), name
    # the struct of the binding has the header's fields, in its order
    body = re.search(r"typedef struct rtx_tally_params \{(.*?)\} rtx_tally_params;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == [f for f, _ in _lib.TallyParams._fields_]
    body = re.search(r"typedef struct rtx_tally_view \{(.*?)\} rtx_tally_view;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [re.sub(r"\[.*", "", f) for f in re.findall(r"(\w+(?:\[\d+\])?);", body)] == [f for f, _ in _lib.TallyView._fields_]


# a hand-written example: samples, weights 0 / 1 / 5, an empty read, RTX_DEMUX_NONE on a weight-0 read
READS = [seq(A, Cc, G), seq(A, Cc), seq(A, Cc, G), seq(), seq(T, T, T, T), seq(A, Cc), seq(G), seq(A, Cc, G), seq(15, A)]
SAMPLE = np.array([0, 1, 2, 7, rx.DEMUX_NONE, 1, 0, 0, 2], np.uint32)   # (7 on the empty read: nobody looks at it)
WEIGHT = np.array([1, 5, 1, 1, 0, 1, 5, 5, 1], np.uint32)
WANT = {bytes(seq(A, Cc, G)): (6, 0, 1), bytes(seq(A, Cc)): (0, 6, 0), bytes(seq(G)): (5, 0, 0), bytes(seq(15, A)): (0, 0, 1)}


def test_hand_written_example():
    assert expected_table(READS, SAMPLE, WEIGHT, 3) == WANT   # (the dict of the GPU tests restates the example)
    t = rx.tally_reads(*concat(READS), SAMPLE, WEIGHT, samples=3)
    assert t.as_dict() == WANT
    assert t.totals == {"reads": 19, "entries": 4, "overflow_reads": 0}
    assert t.columns == 3 and t.counts.dtype == np.uint64
    # the sequence seen only with weight 0 is no entry, nor is the empty read
    assert bytes(seq(T, T, T, T)) not in t.as_dict() and b"" not in t.as_dict()
    assert list(t.sizes) == [7, 6, 5, 1] and np.array_equal(t.sizes, t.counts.sum(axis=1))
    # rank of first appearance: ACG, AC, G, NA
    assert list(t.first) == [0, 1, 2, 3]
    # one column without samples, every weight 1
    one = rx.tally_reads(*concat(READS))
    assert one.as_dict() == {bytes(seq(A, Cc, G)): (3,), bytes(seq(A, Cc)): (2,), bytes(seq(T, T, T, T)): (1,), bytes(seq(G)): (1,), bytes(seq(15, A)): (1,)}
    assert one.totals["reads"] == 8 and one.columns == 1


def test_sort_order_size_then_bytes():
    # three of size 2: a prefix sorts before the longer sequence, a lower code before a higher one; then the singletons
    reads = [seq(G, A), seq(A, Cc, G), seq(A, Cc), seq(G, A), seq(A, Cc), seq(A, Cc, G), seq(T), seq(A), seq(T), seq(T)]
    t = rx.tally_reads(*concat(reads))
    assert [bytes(s) for s in t.seqs] == [bytes(seq(T)), bytes(seq(A, Cc)), bytes(seq(A, Cc, G)), bytes(seq(G, A)), bytes(seq(A))]
    assert list(t.sizes) == [3, 2, 2, 2, 1]
    assert list(t.first) == [3, 2, 1, 0, 4]
    # an add re-sorts
    t.add(*concat([seq(A)] * 3))
    assert [bytes(s) for s in t.seqs][0] == bytes(seq(A)) and list(t.sizes) == [4, 3, 2, 2, 2]


def test_merge_common_and_disjoint():
    a = rx.tally_reads(*concat([seq(A), seq(Cc), seq(A)]), np.array([0, 1, 1], np.uint32), samples=2)
    b = rx.tally_reads(*concat([seq(G, G), seq(A)]), np.array([1, 0], np.uint32), np.array([5, 1], np.uint32), samples=2)
    empty = rx.tally_reads(*concat([]), samples=2)
    m = rx.tally_merge([a, b, empty])
    assert m.as_dict() == {bytes(seq(A)): (2, 1), bytes(seq(Cc)): (0, 1), bytes(seq(G, G)): (0, 5)}
    assert m.totals == {"reads": 9, "entries": 3, "overflow_reads": 0}
    assert [bytes(s) for s in m.seqs] == [bytes(seq(G, G)), bytes(seq(A)), bytes(seq(Cc))]
    assert a.as_dict() == {bytes(seq(A)): (1, 1), bytes(seq(Cc)): (0, 1)}   # the sources are as they were
    with pytest.raises(rx.RtxError) as e:
        rx.tally_merge([a, rx.tally_reads(*concat([seq(A)]), samples=3)])
    assert e.value.code == _lib.RTX_ERR_INVALID and "column" in str(e.value)
    with pytest.raises(rx.RtxError):
        rx.tally_merge([a, rx.tally_reads(*concat([seq(A)]))])   # one column against two


def test_formatters_exact_text():
    t = rx.tally_reads(*concat(READS), SAMPLE, WEIGHT, samples=3)
    assert rx.tally_fasta(t) == ">uniq1;size=7\nACG\n>uniq2;size=6\nAC\n>uniq3;size=5\nG\n>uniq4;size=1\n-A\n"
    assert rx.tally_table_text(t, ["s1", "s2", "third"]) == "#uniq\ts1\ts2\tthird\nuniq1\t6\t0\t1\nuniq2\t0\t6\t0\nuniq3\t5\t0\t0\nuniq4\t0\t0\t1\n"
    # minsize drops entries, the ranks stay those of the whole table
    assert rx.tally_fasta(t, minsize=6) == ">uniq1;size=7\nACG\n>uniq2;size=6\nAC\n"
    assert rx.tally_table_text(t, ["s1", "s2", "third"], minsize=2) == "#uniq\ts1\ts2\tthird\nuniq1\t6\t0\t1\nuniq2\t0\t6\t0\nuniq3\t5\t0\t0\n"
    # a tie in size: the rank follows the bytes
    tie = rx.tally_reads(*concat([seq(T), seq(A, Cc), seq(A)]))
    assert rx.tally_fasta(tie, minsize=1) == ">uniq1;size=1\nA\n>uniq2;size=1\nAC\n>uniq3;size=1\nT\n"
    assert rx.tally_fasta(rx.tally_reads(*concat([]))) == ""
    assert rx.tally_table_text(rx.tally_reads(*concat([])), ["all"]) == "#uniq\tall\n"
    with pytest.raises(ValueError):
        rx.tally_table_text(t, ["s1", "s2"])


def test_need_and_cap_protocol():
    lib = _lib.load()
    t = rx.tally_reads(*concat(READS), SAMPLE, WEIGHT, samples=3)
    want = rx.tally_fasta(t).encode()
    names = (C.c_char_p * 3)(b"s1", b"s2", b"third")
    want_table = rx.tally_table_text(t, ["s1", "s2", "third"]).encode()
    for fn, args, text in ((lib.rtx_tally_format_fasta, (1,), want), (lib.rtx_tally_format_table, (names, 1), want_table)):
        need = fn(t._h, *args, None, 0)
        assert need == len(text)
        buf = C.create_string_buffer(b"\xff" * (need + 8), need + 8)
        short = fn(t._h, *args, buf, need - 1)
        assert short == -need - 1024 and buf.raw == b"\xff" * (need + 8)   # -(bytes needed) - RTX_NEED_BASE, nothing written
        assert fn(t._h, *args, buf, need) == need
        assert buf.raw[:need] == text and buf.raw[need:] == b"\xff" * 8     # exactly `need` bytes, no terminator
    assert lib.rtx_tally_format_fasta(None, 1, None, 0) == _lib.RTX_ERR_INVALID
    assert lib.rtx_tally_format_table(t._h, None, 1, None, 0) == _lib.RTX_ERR_INVALID


def test_sample_out_of_range_is_refused():
    reads = [seq(A), seq(Cc), seq(G)]
    t = rx.tally_reads(*concat(reads), np.array([0, 1, 1], np.uint32), samples=2)
    before = t.as_dict()
    with pytest.raises(rx.RtxError) as e:
        t.add(*concat(reads), np.array([0, 2, 1], np.uint32))
    assert e.value.code == _lib.RTX_ERR_INVALID and "sample 2" in str(e.value)
    assert t.as_dict() == before and t.totals["reads"] == 3   # nothing of the refused chunk was counted
    with pytest.raises(rx.RtxError):
        rx.tally_reads(*concat(reads), np.array([0, 1, 0], np.uint32))   # one column: only sample 0
    # ... but on a read that does not count any value goes
    t.add(*concat(reads + [seq()]), np.array([0, 9, 1, 9], np.uint32), np.array([1, 0, 1, 1], np.uint32))
    assert t.totals["reads"] == 5
    with pytest.raises(rx.RtxError):
        t.add(np.zeros(4, np.uint8), np.array([0, 3, 2, 4], np.uint64))   # offsets not monotone
    with pytest.raises(ValueError):
        t.add(*concat(reads), np.array([0, 1], np.uint32))


def test_create_without_a_device_is_loud():
    lib = _lib.load()
    if lib.rtx_device_count() != 0:   # (with a GPU the object exists; what it computes: test_gpu_tally.py)
        rx.Tally(device=0)
        return
    h = C.c_void_p()
    assert lib.rtx_tally_create(0, None, C.byref(h)) == _lib.RTX_ERR_NO_DEVICE and not h.value
    with pytest.raises(rx.RtxError) as e:
        rx.Tally()
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE
    p = _lib.TallyParams(0, 1 << 31, 0, 0, 0)   # the parameters are checked first
    assert lib.rtx_tally_create(0, C.byref(p), C.byref(h)) == _lib.RTX_ERR_INVALID
    assert rx.raxtax_last_tally()[:3] == (0, 0, 0)

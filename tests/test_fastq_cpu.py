"""FASTQ ingest on the host (rtx_queries_parse_fastq, rtx_fastq_block_end, rtx_queries_parse_fastq_block, rtx_queries_quals): the four-line
record form, the block-wise parse against the whole-file parse for every cut position, the FASTA parse of the same records, and every
parse error of include/raxtax_hip.h."""
import ctypes as C

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

from qual_common import fastq_text

# a quality line that starts with '@', one that starts with '+', lower case, IUPAC codes, a read without bases
RECORDS = [
    ("r0 first", "ACGTACGTAC", "@IIIIIIII#"),
    ("r1", "acgtnNRYKM", "+~!5555555"),
    ("r2;tax=x", "A", "@"),
    ("r3", "", ""),
    ("r4", "GGGGCCCCTTTTAAAA", "@@@@++++@+@+IIII"),
    ("r5 last", "TTGCA", "+@+@!"),
]


def _handle_records(lib, h):
    n = lib.rtx_queries_len(h)
    pb, po, pq = _lib.u8p(), _lib.u64p(), _lib.u8p()
    _lib.check(lib.rtx_queries_data(h, C.byref(pb), C.byref(po)))
    _lib.check(lib.rtx_queries_quals(h, C.byref(pq)))
    assert pq, "a FASTQ parse holds qualities"
    off = [int(po[i]) for i in range(n + 1)]
    out = []
    for i in range(n):
        out.append((lib.rtx_queries_label(h, i).decode(), bytes(pb[off[i]:off[i + 1]]), bytes(pq[off[i]:off[i + 1]])))
    return out


def _whole(text, skip=()):
    return [(l, b.tobytes(), q.tobytes()) for l, b, q in rx.parse_query_fastq_str(text, skip)]


def _blocks(data, first_len, skip=()):
    """The records of `data` read as the CLI reads a file: a first read of first_len bytes, then the rest; every block is cut at
    rtx_fastq_block_end and its tail carried over."""
    lib = _lib.load()
    skip_arr = (C.c_char_p * max(len(skip), 1))(*[s.encode() for s in skip])
    got, carry, first = [], b"", True
    for piece, last in ((data[:first_len], False), (data[first_len:], True)):
        buf = carry + piece
        flags = 0 if first else _lib_flags()[1]
        if last:
            end = len(buf)
        else:
            end = lib.rtx_fastq_block_end(buf, len(buf))
            flags |= _lib_flags()[0]
        carry = buf[end:]
        if end == 0:
            continue
        h = C.c_void_p()
        _lib.check(lib.rtx_queries_parse_fastq_block(buf, end, skip_arr, len(skip), 33, flags, C.byref(h)))
        try:
            got += _handle_records(lib, h)
        finally:
            lib.rtx_queries_destroy(h)
        first = False
    return got


def _lib_flags():
    return 1, 2   # RTX_FASTA_MORE_FOLLOWS, RTX_FASTA_NOT_FIRST


@pytest.mark.parametrize("line_end,last_newline", [("\n", True), ("\r\n", True), ("\n", False), ("\r\n", False)])
def test_block_wise_parse_equals_the_whole_file_parse_at_every_cut(line_end, last_newline):
    text = fastq_text(RECORDS, line_end, last_newline)
    data = text.encode()
    want = _whole(text)
    assert [w[0] for w in want] == [r[0] for r in RECORDS]
    assert [w[2].decode() for w in want] == [r[2] for r in RECORDS]
    for cut in range(len(data) + 1):
        assert _blocks(data, cut) == want, cut


def test_block_end_counts_groups_of_four_lines():
    lib = _lib.load()
    data = fastq_text(RECORDS).encode()
    one = fastq_text(RECORDS[:1]).encode()
    assert lib.rtx_fastq_block_end(data, len(data)) == len(data)
    assert lib.rtx_fastq_block_end(data, len(data) - 1) == len(fastq_text(RECORDS[:-1]).encode())
    assert lib.rtx_fastq_block_end(one, len(one) - 1) == 0
    # "\n@" inside a record is no record start: the quality line of r0 starts with '@'
    assert lib.rtx_fastq_block_end(data, len(one) + 3) == len(one)


def test_bases_and_labels_equal_the_fasta_parse_of_the_same_records():
    recs = [r for r in RECORDS if r[1]]   # (a FASTA record without bases is dropped by the FASTA rules)
    fq = rx.parse_query_fastq_str(fastq_text(recs))
    fa = rx.parse_query_fasta_str("".join(f">{l}\n{s}\n" for l, s, _ in recs))
    assert [x[0] for x in fq] == [x[0] for x in fa]
    for a, b in zip(fq, fa):
        assert np.array_equal(a[1], b[1])
        assert a[2].dtype == np.uint8 and len(a[2]) == len(a[1])


def test_skip_labels_are_dropped():
    text = fastq_text(RECORDS)
    skip = ["r1", "r5 last"]
    want = [w for w in _whole(text) if w[0] not in skip]
    assert _whole(text, skip) == want
    assert len(want) == len(RECORDS) - 2
    assert _blocks(text.encode(), 40, skip) == want


def test_ascii_base_64_is_accepted_and_others_are_not():
    text = fastq_text([("a", "ACGT", "hhhh")])
    assert rx.parse_query_fastq_str(text, ascii_base=64)[0][2].tobytes() == b"hhhh"
    with pytest.raises(rx.RtxError) as e:
        rx.parse_query_fastq_str(text, ascii_base=50)
    assert e.value.code == _lib.RTX_ERR_INVALID


@pytest.mark.parametrize("text,what", [
    ("@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n", "record 2"),          # a first line that does not start with '@'
    ("@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n", "record 2"),        # a third line that does not start with '+'
    ("@a\nACGT\n+\nIII\n", "record 1"),                             # a quality string of another length
    ("@a\nACGT\n+\nIIIII\n", "record 1"),
    ("@a\nACGT\n+\nII I\n", "record 1"),                            # a quality byte outside 33 .. 126
    ("@a\nACGT\n+\nII\x7fI\n", "record 1"),
    ("@a\nACGT\n+\nIIII\n@b\nAC\n+\n", "record 2"),                 # a record that is cut short
    ("@a\nACGT\n+\nIIII\n@b\n", "record 2"),
    ("@a\nAC!T\n+\nIIII\n", "record 1"),                            # a character that is no base
])
def test_parse_errors(text, what):
    with pytest.raises(rx.RtxError) as e:
        rx.parse_query_fastq_str(text)
    assert e.value.code == _lib.RTX_ERR_PARSE
    assert what in str(e.value)


def test_empty_text_is_a_parse_error():
    for text in ("", "\n\n"):
        with pytest.raises(rx.RtxError) as e:
            rx.parse_query_fastq_str(text)
        assert e.value.code == _lib.RTX_ERR_PARSE


def test_quals_is_null_for_a_fasta_parse():
    lib = _lib.load()
    data = b">a\nACGT\n"
    h = C.c_void_p()
    _lib.check(lib.rtx_queries_parse_fasta(data, len(data), (C.c_char_p * 1)(), 0, C.byref(h)))
    try:
        pq = _lib.u8p()
        _lib.check(lib.rtx_queries_quals(h, C.byref(pq)))
        assert not pq
    finally:
        lib.rtx_queries_destroy(h)
    assert all(len(r) == 2 for r in rx.parse_query_fasta_str(data.decode()))


def test_blank_lines_behind_the_last_record_are_tolerated():
    text = fastq_text(RECORDS)
    assert _whole(text + "\n\n \n") == _whole(text)

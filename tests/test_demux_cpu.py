"""Sample demultiplexing (rtx_demux.hip) without a GPU: the additions to the C ABI, the host function rtx_demux_read and the device's
staging and per-read function (rtx_math.hpp: trim_stage_row, demux_tag_init, demux_read) run through the x86 emulator -- both against the
numpy restatement of tests/demux_common.py on the reads and lists the GPU tests use -- the sample sheet parser, and the checks of
rtx_demux_create that need no device.  No tolerance anywhere."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from demux_common import AMBIGUOUS, NO_TAG, NO_TAG3, NO_TAG5, NONE, OK, UNKNOWN_PAIR, concat, demux_ref, expected, shared

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sample", "lo", "hi", "hit", "info")
CONFIGS = [("l96", 3, 15), ("l96", 0, 0), ("l1", 0, 0), ("l2", 3, 1), ("l1024", 2, 3), ("mixed", 0, 0), ("mixed", 1, 15), ("only5", 3, 15), ("only3", 1, 1)]


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g, np.uint32), np.asarray(w, np.uint32)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:8]}: got {g[bad[:8]]}, expected {w[bad[:8]]}"


def emul_run(emul, tags, pairs, max_mismatches, max_offset, reads):
    codes, code_off = concat([c for c, _ in tags])
    code_off = code_off.astype(np.uint32)
    end = np.array([e for _, e in tags], np.uint32)
    flat_pairs = np.array([[NO_TAG if a is None else a, NO_TAG if b is None else b, s] for a, b, s in pairs], np.uint32).reshape(-1)
    bases, off = concat(reads)
    bases = np.concatenate([bases, np.zeros(1, np.uint8)])
    out = np.zeros(5 * len(reads), np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    emul.emul_demux_reads.restype = None
    emul.emul_demux_reads(C.c_uint32(len(tags)), vp(codes), vp(code_off), vp(end), C.c_uint32(len(pairs)), vp(flat_pairs), C.c_uint32(max_mismatches),
                          C.c_uint32(max_offset), C.c_uint64(len(reads)), vp(bases), vp(off), vp(out))
    return out.reshape(5, len(reads))


def test_the_expectation_holds_every_kind():
    sample, lo, hi, hit, info, d5, d3 = expected("l96", 3, 15)
    lists, reads = shared()
    verdict = info & 0xFF
    assert set(np.unique(verdict)) == {OK, NO_TAG5, NO_TAG3, AMBIGUOUS, UNKNOWN_PAIR}
    assert ((sample != NONE) == (verdict == OK)).all() and set(np.unique(sample[verdict == OK])) == {0, 1, 2, 3, 4}
    length = np.array([len(r) for r in reads])
    assert ((hi == lo) & (lo > 0) & (lo < length)).any() and ((hi == lo) & (hi == length)).any() and ((hi == lo) & (length == 0)).any()
    for d in (d5, d3):                                                   # as many substitutions as allowed, and one more
        assert (d == 3).any() and (d == 4).any()
    assert (((info >> 8) & 0xFF) == 3).any() and (((info >> 16) & 0xFF) == 3).any()
    assert set(np.unique(info >> 28)) >= {0, 1, 7, 15} and set(np.unique((info >> 24) & 0xF)) >= {0, 1, 7, 15}


@pytest.mark.parametrize("name,mm,off", CONFIGS)
def test_emulated_kernel_body_equals_the_restatement(emul, name, mm, off):
    lists, reads = shared()
    tags, pairs = lists.lists[name]
    assert_equal(emul_run(emul, tags, pairs, mm, off, reads), expected(name, mm, off), f"{name} {mm} {off}")


@pytest.mark.parametrize("name,mm,off", [c for c in CONFIGS if c[0] != "l1024"] + [("l1024", 2, 3)])
def test_demux_read_equals_the_restatement(name, mm, off):
    lists, reads = shared()
    tags, pairs = lists.lists[name]
    some = range(len(reads)) if name != "l1024" else range(0, len(reads), 4)
    got = np.array([rx.demux_read(tags, pairs, (mm, off), reads[i]) for i in some], np.uint32).T
    assert_equal(got, [w[list(some)] for w in expected(name, mm, off)[:5]], f"{name} {mm} {off}")


def test_demux_hit_takes_the_words_apart():
    assert rx.demux_hit(3 | NO_TAG << 16, 2 | 1 << 8 | 5 << 24) == (2, 3, 1, 5, None, 0, 0)
    assert rx.demux_hit(NO_TAG | 7 << 16, 0 | 8 << 16 | 15 << 28) == (0, None, 0, 0, 7, 8, 15)
    assert rx.demux_verdict_names() == ("ok", "no_tag5", "no_tag3", "ambiguous", "unknown_pair")


# ---------------------------------------------------------------------------------------------------------------------------------
# the sample sheet
# ---------------------------------------------------------------------------------------------------------------------------------
SHEET = """# run 12
s1\tACGT\tTTGA
s2\tACGW\tTTGA   # the 3' tag is shared
s1\tGGGG\tCCAN

s3\tGGGG\tTTGA
"""
A, Cc, G, T, W, N = 1, 2, 4, 8, 9, 15


def plain(tags):
    return [(list(map(int, t.codes)), t.end) for t in tags]


def test_sample_sheet():
    tags, pairs, names = rx.sample_sheet(SHEET)
    assert names == ["s1", "s2", "s3"]
    # rev_tag as on the oligo: the read ends with its reverse complement (TTGA -> TCAA, CCAN -> NTGG)
    assert plain(tags) == [([A, Cc, G, T], 0), ([T, Cc, A, A], 1), ([A, Cc, G, W], 0), ([G, G, G, G], 0), ([N, T, G, G], 1)]
    assert pairs == [(0, 1, 0), (2, 1, 1), (3, 4, 0), (3, 1, 2)]
    tags, pairs, names = rx.sample_sheet("a\tAC\t-\nb\tGT\n# nothing\nc\tTT\t\n")
    assert plain(tags) == [([A, Cc], 0), ([G, T], 0), ([T, T], 0)] and pairs == [(0, None, 0), (1, None, 1), (2, None, 2)] and names == ["a", "b", "c"]
    with pytest.raises(ValueError, match="twice"):
        rx.sample_sheet("a\tAC\tGG\nb\tAC\tGG\n")
    with pytest.raises(ValueError, match="line 2"):
        rx.sample_sheet("a\tAC\tGG\nb\n")
    with pytest.raises(ValueError, match="IUPAC"):
        rx.sample_sheet("a\tAXC\tGG\n")
    with pytest.raises(ValueError, match="rev_tag"):
        rx.sample_sheet("a\tAC\t-\n", both_orientations=True)


def test_sample_sheet_both_orientations():
    tags, pairs, names = rx.sample_sheet("s1\tACGT\tTTGA\ns2\tACGW\tTTGA\n", both_orientations=True)
    assert names == ["s1", "s2"]
    # per line: fwd at 5', revcomp(rev) at 3'; then rev at 5', revcomp(fwd) at 3' (ACGT is its own reverse complement, ACGW -> WCGT)
    assert plain(tags) == [([A, Cc, G, T], 0), ([T, Cc, A, A], 1), ([T, T, G, A], 0), ([A, Cc, G, T], 1), ([A, Cc, G, W], 0), ([W, Cc, G, T], 1)]
    assert pairs == [(0, 1, 0), (2, 3, 0), (4, 1, 1), (2, 5, 1)]
    # a read of s2 in either orientation is assigned to it
    read = rx.encode_iupac("ACGAGGGGGGGGTCAA")
    for r in (read, rx.api.revcomp(read)):
        assert rx.demux_read(tags, pairs, (0, 0), r)[:3] == (1, 4, 12)


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks that need no device, and the ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_create_checks_come_before_the_device():
    t5, t3 = (np.array([1, 2, 4, 8], np.uint8), 0), (np.array([8, 4, 2, 1], np.uint8), 1)
    good = ([t5, t3], [(0, 1, 0)], (1, 1))
    bad = {
        "no tags": ([], [], (0, 0)),
        "too many on one end": ([t5] * 1025, [], (0, 0)),
        "empty tag": ([(np.zeros(0, np.uint8), 0), t3], [], (0, 0)),
        "tag of 33 codes": ([(np.ones(33, np.uint8), 0)], [], (0, 0)),
        "byte 0 in a tag": ([(np.array([1, 0, 2], np.uint8), 0)], [], (0, 0)),
        "byte 16 in a tag": ([(np.array([1, 16, 2], np.uint8), 1)], [], (0, 0)),
        "unknown end": ([(t5[0], 2)], [], (0, 0)),
        "max_mismatches 9": (good[0], good[1], (9, 0)),
        "max_offset 16": (good[0], good[1], (0, 16)),
        "pair out of range": (good[0], [(0, 2, 0)], (0, 0)),
        "pair names a 3' tag as tag5": (good[0], [(1, 1, 0)], (0, 0)),
        "pair names a 5' tag as tag3": (good[0], [(0, 0, 0)], (0, 0)),
        "pair of no tags": (good[0], [(None, None, 0)], (0, 0)),
        "sample NONE": (good[0], [(0, 1, NONE)], (0, 0)),
        "pair twice": (good[0], [(0, 1, 0), (0, 1, 1)], (0, 0)),
    }
    for what, (tags, pairs, params) in bad.items():
        for call in (lambda: rx.Demux(0, tags, pairs, params), lambda: rx.demux_read(tags, pairs, params, t5[0])):
            with pytest.raises(rx.RtxError) as e:
                call()
            assert e.value.code == _lib.RTX_ERR_INVALID, what
    # the order: a bad tag is named before bad parameters, bad parameters before a bad pair
    with pytest.raises(rx.RtxError, match="tag 0"):
        rx.demux_read([(np.zeros(0, np.uint8), 0)], [(0, 5, 0)], (9, 0), t5[0])
    with pytest.raises(rx.RtxError, match="max_mismatches"):
        rx.demux_read(good[0], [(0, 5, 0)], (9, 0), t5[0])
    if _lib.load().rtx_device_count() == 0:                             # a good list reaches the device check
        with pytest.raises(rx.RtxError) as e:
            rx.Demux(0, *good)
        assert e.value.code == _lib.RTX_ERR_NO_DEVICE
    assert rx.demux_read(*good, np.array([1, 2, 4, 8, 1, 1, 8, 4, 2, 1], np.uint8)) == (0, 4, 6, 0 | 1 << 16, 0)


def test_the_abi_is_added_to_not_changed():
    lib = _lib.load()
    assert lib.rtx_abi_version() == 6
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    for name in ("rtx_demux_create", "rtx_demux_run", "rtx_demux_destroy", "rtx_demux_kernel_time", "rtx_demux_read", "rtx_index_profile_begin_samples",
                 "rtx_batch_prefetch_samples", "rtx_index_profile_read_samples", "rtx_sample_profile_merge", "rtx_sample_table_format"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib._SIGNATURES and hasattr(lib, name), name
    for macro, value in (("RTX_DEMUX_MAX_TAGS", 1024), ("RTX_DEMUX_MAX_TAG", 32), ("RTX_DEMUX_MAX_OFFSET", 15), ("RTX_DEMUX_MAX_MISMATCHES", 8),
                         ("RTX_DEMUX_NO_TAG", 0xFFFF), ("RTX_DEMUX_NONE", 0xFFFFFFFF)):
        m = re.search(rf"#define {macro}\s+(\w+)", header)
        assert m and int(m.group(1).rstrip("u"), 0) == value == getattr(_lib, macro), macro
    assert C.sizeof(_lib.DemuxTag) == 16 and C.sizeof(_lib.DemuxPair) == 12 and C.sizeof(_lib.DemuxParams) == 8


# ---------------------------------------------------------------------------------------------------------------------------------
# the taxon x sample table
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_table_text_byte_for_byte():
    lineages = ["A,a1,x", "A,a1,y", "A,a2,z", "B,b1,w"]
    rng = np.random.default_rng(5)
    tree = rx.Tree.new(lineages, [(1 << rng.integers(0, 4, 40)).astype(np.uint8) for _ in lineages])
    nodes = tree.nodes()
    n = len(nodes["parent"])
    # a node by its lineage prefix: depth levels of the lineage at node_begin (the nodes come breadth first)
    depth = np.zeros(n, int)
    for v in range(1, n):
        depth[v] = depth[nodes["parent"][v]] + 1
    node = {",".join(tree.lineages[int(nodes["begin"][v])].split(",")[:depth[v]]): v for v in range(1, n) if nodes["type"][v] != 2}
    direct = np.zeros((3, n), np.uint64)
    direct[0, node["A,a1,x"]] = 5        # sample one: two leaves under a1, one read that stops at A
    direct[0, node["A,a1,y"]] = 2
    direct[0, node["A"]] = 1
    direct[2, node["A,a2"]] = 4          # sample three: a read set that stops at a2 and at b1,w; sample two: nothing
    direct[2, node["B,b1,w"]] = 7
    totals = np.array([[10, 8, 1, 1], [0, 0, 0, 0], [12, 11, 1, 0]], np.uint64)
    text = rx.sample_table_text(tree, ["one", "two", "three"], rx.SampleProfile(80, 0, direct, totals))
    assert text == ("# cutoff=0.80\tsamples=3\n"
                    "# queries\t10\t0\t12\n"
                    "# classified\t8\t0\t11\n"
                    "# unclassified\t1\t0\t1\n"
                    "# unclassifiable\t1\t0\t0\n"
                    "depth\ttaxon\tlineage\tone\ttwo\tthree\n"
                    "1\tA\tA\t8\t0\t4\n"
                    "2\ta1\tA,a1\t7\t0\t0\n"
                    "3\tx\tA,a1,x\t5\t0\t0\n"
                    "3\ty\tA,a1,y\t2\t0\t0\n"
                    "2\ta2\tA,a2\t0\t0\t4\n"
                    "1\tB\tB\t0\t0\t7\n"
                    "2\tb1\tB,b1\t0\t0\t7\n"
                    "3\tw\tB,b1,w\t0\t0\t7\n")
    merged = rx.sample_profile_merge([rx.SampleProfile(80, 0, direct, totals)] * 2)
    assert np.array_equal(merged.direct, 2 * direct) and np.array_equal(merged.totals, 2 * totals)
    with pytest.raises(rx.RtxError) as e:
        rx.sample_profile_merge([rx.SampleProfile(80, 0, direct, totals), rx.SampleProfile(70, 0, direct, totals)])
    assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(ValueError):
        rx.sample_table_text(tree, ["one", "two"], rx.SampleProfile(80, 0, direct, totals))

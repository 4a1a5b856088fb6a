"""The OTUs of a run on the host (host_otu.cpp): rx.otu_cluster_host against the brute force of otu_common.py on every fixture the device is
held against in test_gpu_otu.py, the three formatters against hand-written text, and the errors.  No tolerance anywhere."""
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from otu_common import (BLOCK_EDGES, MANY, MAX_LEN, PLAIN, WEIGHTINGS, assert_otus, block_case, brute_force, brute_of, check_blocks, check_clusters,
                        check_complete, cluster_case, complete_case, edge_case, equal_length_force, many_blocks_case, pair_links, ranks, seq, table_of)
from tally_common import random_seq

ROOT = Path(__file__).resolve().parent.parent

def test_symbols_are_declared_bound_and_exported():
    text = (ROOT / "include" / "raxtax_hip.h").read_text()
    lib = _lib.load()
    for name in ("rtx_otu_cluster", "rtx_otu_cluster_host", "rtx_otu_view", "rtx_otu_times", "rtx_otu_destroy", "rtx_otu_format_fasta", "rtx_otu_format_table",
                 "rtx_otu_format_map"):
        assert name in _lib._SIGNATURES and re.search(rf"\b{name}\(", text) and hasattr(lib, name), name
    assert "#define RTX_DEFAULT_OTU_HASH_MASK 5" in text and _lib.RTX_DEFAULT_OTU_HASH_MASK == 5
    assert f"#define RTX_OTU_MAX_LEN {MAX_LEN}" in text and _lib.RTX_OTU_MAX_LEN == MAX_LEN
    assert lib.rtx_abi_version() == 6


def test_the_brute_force_sees_every_kind():
    """before anything is held against it: the brute force links what was planted as a link and nothing that was planted as none, and the
    pair-by-pair statement of the definition gives the same list"""
    table, want, marks = edge_case()
    rank = ranks(table)
    links = {tuple(l) for l in want["links"].tolist()}
    kinds = {}
    for name, (x, y, is_link) in marks.items():
        a, b = sorted((rank[bytes(x)], rank[bytes(y)]))
        assert ((a, b) in links) == is_link, name
        kinds.setdefault(name.split(" ")[0], set()).add(is_link)
    assert kinds["sub"] == {True} and kinds["del"] == {True} and kinds["run"] == {True} and kinds["ins"] == {True, False}
    for name in ("N base", "R base", "deleted N"):
        assert marks[name][2]
    for name in ("N R", "two subs", "one of each", "transposition", "rotation"):
        assert not marks[name][2]
    assert 150 <= len(table.seqs) <= 330 and want["long_rows"] == 3
    assert want["links"].tolist() == [list(l) for l in pair_links(table.seqs)]
    assert 1 < len(want["seed"]) < len(table.seqs)


def test_host_against_the_brute_force_on_the_edges():
    table, want, _ = edge_case()
    got = rx.otu_cluster_host(table)
    assert_otus(got, want)
    assert got.link_passes == 1 and got.rounds == 0 and got.seconds == (0, 0, 0, 0)


def test_host_against_the_brute_force_on_the_clusters():
    table, want, named = cluster_case()
    got = rx.otu_cluster_host(table)
    assert_otus(got, want)
    check_clusters(table, got, named)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_host_against_the_brute_force_on_the_complete_world(weighting):
    table, want = complete_case(weighting)
    lens = np.array([len(s) for s in table.seqs])
    a, b = want["links"][:, 0], want["links"][:, 1]
    assert len(want["links"]) == 64000                     # by the definition: 36 864 + 7 680 substitutions and 1 024 x 19 deletions
    assert int(((lens[a] == 6) & (lens[b] == 6)).sum()) == 36864 and int(((lens[a] == 5) & (lens[b] == 5)).sum()) == 7680
    assert int((lens[a] != lens[b]).sum()) == 1024 * 19
    got = rx.otu_cluster_host(table)
    assert_otus(got, want)
    check_complete(table, got, weighting)


def test_the_equal_length_restatement_against_the_brute_force():
    """on the 4 096 rows of 6 codes of the complete world, at sizes from {1, 2, 3}: 36 864 links, every field equal"""
    table, _ = complete_case("three")
    rows = table.seqs
    six = [r for r, s in enumerate(rows) if len(s) == 6]
    seqs, sizes, counts = [rows[r] for r in six], table.sizes[six], table.counts[six]
    want, got = brute_force(seqs, sizes, counts), equal_length_force(seqs, sizes, counts)
    assert len(want["links"]) == 36864 and 1 < len(want["seed"]) < 4096
    assert sorted(want) == sorted(got)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


@pytest.mark.parametrize("last", ("seed", "variant"))
@pytest.mark.parametrize("n", BLOCK_EDGES)
def test_host_against_the_brute_force_on_the_block_edges(n, last):
    table, want, planted = block_case(n, last)
    got = rx.otu_cluster_host(table)
    assert_otus(got, want)
    check_blocks(got, n, planted)
    assert any(a < 256 <= b for a, b in planted) == (n > 256 + (last == "seed"))


def test_host_against_the_restatement_on_65537_rows():
    table, want = many_blocks_case()
    assert len(table.seqs) == MANY == 256 * 256 + 1 and {len(s) for s in table.seqs} == {12} and set(np.unique(table.sizes)) == {1, 2, 3, 4}
    got = rx.otu_cluster_host(table)
    assert_otus(got, want)
    assert len(want["links"]) > 1000 and got.n_otus > MANY * 9 // 10 and got.seed[-1] > 65280
    assert np.bincount(want["seed"] >> 8, minlength=257).min() > 0      # every block of 256 rows holds a seed, the last one its only row


@pytest.fixture(scope="module")
def small():
    """ACGT x 5, TTTT x 3, ACGA x 2, ACG x 1 in two samples: uniq1 .. uniq4 in this order; ACGT, ACGA and ACG are linked with each other"""
    reads = [("ACGT", 0)] * 3 + [("ACGT", 1)] * 2 + [("TTTT", 1)] * 3 + [("ACGA", 0)] * 2 + [("ACG", 1)]
    table = table_of([seq(s) for s, _ in reads], sample=np.array([k for _, k in reads], np.uint32), samples=2)
    return table, rx.otu_cluster_host(table)


def test_formatters_against_hand_written_text(small):
    table, otus = small
    assert otus.links.tolist() == [[0, 2], [0, 3], [2, 3]] and otus.otu.tolist() == [0, 1, 0, 0]
    assert otus.seed.tolist() == [0, 1] and otus.members.tolist() == [3, 1] and otus.sizes.tolist() == [8, 3] and otus.counts.tolist() == [[5, 3], [0, 3]]
    assert rx.otu_fasta(otus) == ">otu1;size=8;seed=uniq1\nACGT\n>otu2;size=3;seed=uniq2\nTTTT\n"
    assert rx.otu_table_text(otus, ["s0", "s1"]) == "#otu\ts0\ts1\notu1\t5\t3\notu2\t0\t3\n"
    assert rx.otu_map_text(otus) == "uniq1\totu1\nuniq2\totu2\nuniq3\totu1\nuniq4\totu1\n"
    with pytest.raises(ValueError):
        rx.otu_table_text(otus, ["s0"])


def test_minsize_leaves_otus_out_and_keeps_the_numbers(small):
    table, otus = small
    assert rx.otu_fasta(otus, minsize=4) == ">otu1;size=8;seed=uniq1\nACGT\n"
    assert rx.otu_table_text(otus, ["s0", "s1"], minsize=4) == "#otu\ts0\ts1\notu1\t5\t3\n"
    assert rx.otu_fasta(otus, minsize=9) == "" and rx.otu_table_text(otus, ["s0", "s1"], minsize=9) == "#otu\ts0\ts1\n"
    # the numbers are those of the whole result: with the large OTU second, it keeps its 2
    table2 = table_of([seq("TTTT")] * 9 + [seq("ACGT")] * 5 + [seq("ACG")])
    o2 = rx.otu_cluster_host(table2)
    assert rx.otu_fasta(o2, minsize=1) == ">otu1;size=9;seed=uniq1\nTTTT\n>otu2;size=6;seed=uniq2\nACGT\n"
    assert rx.otu_fasta(o2, minsize=7) == ">otu1;size=9;seed=uniq1\nTTTT\n" and rx.otu_table_text(o2, ["all"], minsize=7) == "#otu\tall\notu1\t9\n"
    # a buffer that is too small says what it needs; another table is refused
    lib = _lib.load()
    import ctypes as C
    buf = C.create_string_buffer(4)
    need = len(rx.otu_map_text(otus))
    assert lib.rtx_otu_format_map(otus._h, buf, 4) == -need - 1024
    assert lib.rtx_otu_format_fasta(otus._h, table2._h, 1, None, 0) == _lib.RTX_ERR_INVALID


def test_ambiguity_codes_and_a_long_row():
    base = random_seq(np.random.default_rng(2), MAX_LEN + 1)
    table = table_of([base, np.delete(base, 100)], [2, 1])
    got = rx.otu_cluster_host(table)
    assert got.long_rows == 1 and len(got.links) == 0 and got.n_otus == 2
    assert_otus(got, brute_of(table))
    table = table_of([seq("ACGTACGT"), seq("ACNTACGT"), seq("ACRTACGT"), seq("ACGTNACGT"), seq("A"), seq("AC"), seq("C")], [7, 6, 5, 4, 3, 2, 1])
    got = rx.otu_cluster_host(table)
    assert_otus(got, brute_of(table))
    assert got.links.tolist() == [[0, 1], [0, 2], [0, 3], [4, 5], [4, 6], [5, 6]]     # N - R is none; a row of one code has no deletion


def test_errors_and_the_empty_table():
    table, _, _ = cluster_case()
    for fn in (rx.otu_cluster_host, rx.otu_cluster):
        with pytest.raises(rx.RtxError) as e:
            fn(table, differences=2)
        assert e.value.code == _lib.RTX_ERR_INVALID
    with pytest.raises(rx.RtxError) as e:
        rx.otu_cluster_host(table, flags=1)
    assert e.value.code == _lib.RTX_ERR_INVALID
    assert_otus(rx.otu_cluster_host(table, differences=0), rx.otu_cluster_host(table, differences=1))
    empty = rx.otu_cluster_host(table_of([]))
    assert empty.n_rows == 0 and empty.n_otus == 0 and empty.links.shape == (0, 2) and empty.counts.shape == (0, 1) and empty.long_rows == 0
    assert rx.otu_fasta(empty) == "" and rx.otu_map_text(empty) == "" and rx.otu_table_text(empty, ["all"]) == "#otu\tall\n"


def test_no_device_is_loud():
    table, _, _ = cluster_case()
    if _lib.load().rtx_device_count() == 0:   # (with a GPU the call runs: test_gpu_otu.py)
        with pytest.raises(rx.RtxError) as e:
            rx.otu_cluster(table)
        assert e.value.code == _lib.RTX_ERR_NO_DEVICE
    with pytest.raises(rx.RtxError) as e:     # a device that does not exist, anywhere
        rx.otu_cluster(table, device=4096)
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE

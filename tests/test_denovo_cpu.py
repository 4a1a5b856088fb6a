"""The de novo chimera check without a device: rtx_denovo_check_host (host_denovo.cpp) and the arithmetic the scan kernel adds to the chimera
check's (rtx_math.hpp through the x86 emulator: the prefix mask of lim and the masked checkpoint, over every lane count of a short last
tile) against the numpy restatement of the definition (tests/denovo_common.py), field by field; the worlds that test_gpu_denovo.py puts
on the device -- the live mask at the byte, word, lane and tile edges, a flag that is taken back, rounds over two tiles -- proven as
fixtures by the restatement alone; the symbols, the refusals, the texts and the command line's refusals."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import chimera_common as cc
import denovo_common as dc
import raxtax_amd as rx
from raxtax_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
ONE_TILE = (1, 7, 8, 9, 511, 512, 513, 520)   # (520: all the parents, so that the bitmap holds the entry at lim = 513 too)


def _host(seqs, weights, otus=False, **params):
    table = dc.table_of(rx, seqs, weights)
    o = rx.otu_cluster_host(table) if otus else None
    d = rx.denovo_check_host(table, o, **params)
    rs = dc.of_otus(table, o, **params)[0] if otus else dc.of_table(table, **params)
    return table, o, d, rs


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    lib = _lib.load()
    for name in ("rtx_denovo_check", "rtx_denovo_check_host", "rtx_denovo_view", "rtx_denovo_times", "rtx_denovo_destroy", "rtx_denovo_format_records",
                 "rtx_denovo_format_fasta", "rtx_denovo_format_table"):
        assert name + "(" in header and name in _lib._SIGNATURES and getattr(lib, name) is not None, name
    for text in ("#define RTX_DENOVO_NO_PARENT 3u", "#define RTX_DENOVO_DEFAULT_ABSKEW 2u", "#define RTX_DENOVO_DEFAULT_MAX_PARENTS 262144u", "rtx_denovo_params;",
                 "rtx_denovo_view_t;", "#define RTX_ABI_VERSION 6 "):
        assert text in header, text
    assert (_lib.RTX_DENOVO_NO_PARENT, _lib.RTX_DENOVO_DEFAULT_ABSKEW, _lib.RTX_DENOVO_DEFAULT_MAX_PARENTS) == (3, 2, 262144)
    for name in ("DenovoParams", "Denovo", "denovo_check", "denovo_check_host", "denovo_records_text", "denovo_fasta", "denovo_table_text"):
        assert name in rx.__all__ and hasattr(rx, name), name


def test_slice_option_is_declared_and_accepted():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    assert "#define RTX_DEFAULT_CHIMERA_SLICE 6\n" in header and _lib.RTX_DEFAULT_CHIMERA_SLICE == 6
    lib = _lib.load()
    try:
        assert lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, 2) == 0
        seqs, weights = dc.rounds_world()
        _, _, d, rs = _host(seqs, weights)                  # (the host walk has no slices: the option changes nothing)
        dc.check_equal(d, rs, "capped")
    finally:
        assert lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, 0) == 0
    assert lib.rtx_set_default_option(7, 0) == _lib.RTX_ERR_INVALID


def test_prefix_of_one_tile_on_the_host():
    seqs, weights, where = dc.prefix_world(520, ONE_TILE)
    _, _, d, rs = _host(seqs, weights, segments=4, mindelta=8)
    want = dc.check_equal(d, rs, "one tile")
    for L, (e, winner) in where.items():   # what the case was designed as, by the restatement alone
        assert rs.lim[e] == L and want[e]["parent"] == winner and 21 <= want[e]["single"] < 33, (L, want[e])   # the head's 21 windows (and a chance 8-mer), not the 33 of the copy at lim


def test_skew_edge_and_limits():
    rng = np.random.default_rng(2)
    T = dc.rand_seq(rng, 60)
    seqs = [T, np.concatenate([T[:50], dc.rand_seq(rng, 10)]), np.concatenate([dc.rand_seq(rng, 10), T[10:]]), dc.rand_seq(rng, 60)]
    # w[p] = abskew w[e] is a parent, abskew w[e] - 1 is not
    _, _, d, rs = _host(seqs, [10, 9, 5, 1], segments=4, mindelta=8)
    dc.check_equal(d, rs, "edge")
    assert rs.lim == [0, 0, 1, 3] and [int(r["status"]) for r in d.rec] == [dc.NO_PARENT, dc.NO_PARENT, cc.OK, cc.OK]
    assert cc.as_tuple(d.rec[0]) == cc.as_tuple(dc.blank(dc.NO_PARENT))
    # abskew = 1 with equal weights: only the entries in front
    _, _, d, rs = _host(seqs, [7, 7, 7, 7], segments=4, mindelta=8, abskew=1)
    dc.check_equal(d, rs, "abskew 1")
    assert rs.lim == [0, 1, 2, 3]
    # max_parents below the skew's prefix; abskew large enough that nobody has a parent
    _, _, d, rs = _host(seqs, [100, 90, 5, 1], segments=4, mindelta=8, max_parents=1)
    dc.check_equal(d, rs, "max_parents")
    assert rs.lim == [0, 0, 1, 1]
    _, _, d, rs = _host(seqs, [100, 90, 5, 1], abskew=1000)
    dc.check_equal(d, rs, "nobody")
    assert rs.lim == [0, 0, 0, 0] and d.n_checked == 0
    # abskew w[e] beyond 32 bits: compared without wrapping
    table = dc.table_of(rx, seqs[:2], [4000000000, 2])
    assert [int(x) for x in rx.denovo_check_host(table, abskew=2000000000).lim] == dc.limits([4000000000, 2], 2000000000) == [0, 1]
    assert [int(x) for x in rx.denovo_check_host(table, abskew=2000000001).lim] == dc.limits([4000000000, 2], 2000000001) == [0, 0]


def test_the_greedy_rule_takes_rounds():
    seqs, weights = dc.rounds_world()
    _, _, d, rs = _host(seqs, weights)
    want = dc.check_equal(d, rs, "rounds")
    assert [r["flag"] for r in want] == [0, 0, 1, 1, 1]
    first = [rs.record(e, np.zeros(5, bool))["flag"] for e in range(5)]
    assert first == [0, 0, 1, 0, 0]                     # with C live D is explained by C, and E by D
    rounds, scans, flagged = rs.rounds()
    assert rounds == 4 and scans == 5 + 2 + 1 + 0 and list(flagged) == [False, False, True, True, True]
    assert (d.rounds, d.scans) == (1, 5)                # the host walks the entries once


def _live(n_parents, flagged_at):
    seqs, weights, where = dc.live_world(n_parents, flagged_at)
    _, _, d, rs = _host(seqs, weights, segments=4, mindelta=8)
    want = dc.check_equal(d, rs, f"live {n_parents}")
    assert [e for e in range(rs.n) if want[e]["flag"]] == sorted(flagged_at)
    nobody = np.zeros(rs.n, bool)
    for f, (e, lower) in where.items():
        assert rs.lim[e] == n_parents and lower < f and not want[lower]["flag"]
        assert want[e]["parent"] == lower and 21 <= want[e]["single"] < 33, (f, want[e])   # the head's 21 windows (and a chance 8-mer)
        unmasked = rs.record(e, nobody)
        assert unmasked["parent"] == f and unmasked["single"] == 33, (f, unmasked)         # without the mask the query names f: the fixture sees a bit that is not cleared
    return rs, want, where


def test_live_mask_positions_on_the_host():
    """the flagged entries lie at bits 0 and 7 of the first and last byte of every word of a lane's 16 bytes, in the first and the last lane"""
    assert set(dc.LIVE_520) >= {7, 32, 39, 120, 127, 160, 280, 320, 440, 480, 512, 519} and len(dc.LIVE_520) == 27
    _live(520, dc.LIVE_520)
    assert set(dc.LIVE_8232) >= {7, 2047, 2048, 8191, 8192, 8199, 8224, 8231}
    _live(8232, dc.LIVE_8232)


def test_live_columns_against_the_emulated_checkpoint(emul):
    """the live row of the 520 world as the scan reads it: a query's total counts per parent, the final flags as the live mask, through the
    checkpoint of the scan kernel (five lanes): the count and the parent of the record; with everybody live, f and its 33 windows"""
    rs, want, where = _live(520, dc.LIVE_520)
    p16, p8 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)
    flagged = np.array([bool(r["flag"]) for r in want])
    for f, (e, lower) in where.items():
        counts = np.zeros(8192, np.uint16)
        counts[:520] = rs.totals(e)
        for live, result in (((~flagged[:520]), (want[e]["single"], lower)), (np.ones(520, bool), (33, f))):
            mask = np.zeros(8192, np.uint8)
            mask[:520] = live
            m, r = C.c_uint32(), C.c_uint32()
            assert emul.emul_denovo_checkpoint(counts.ctypes.data_as(p16), mask.ctypes.data_as(p8), 10, 520, 0, 520, C.byref(m), C.byref(r)) == 0
            assert (m.value, r.value) == result, (f, m.value, r.value, result)


def test_a_flag_that_goes_back():
    seqs, weights, at = dc.flipback_world()
    _, _, d, rs = _host(seqs, weights)
    want = dc.check_equal(d, rs, "flipback")
    nobody, c_flagged = np.zeros(6, bool), np.zeros(6, bool)
    c_flagged[at["C"]] = True
    assert rs.record(at["D"], nobody)["flag"] == 1 and rs.record(at["D"], nobody)["parent_a"] == at["C"]
    assert rs.record(at["D"], c_flagged)["flag"] == 0
    history = rs.flag_history()
    assert [int(h[at["D"]]) for h in history] == [1, 0, 0] and all(h[at["C"]] for h in history)    # D: 0 -> 1 -> 0, C flagged in every round
    assert [r["flag"] for r in want] == [0, 0, 0, 1, 0, 0] and want[at["E"]]["parent"] == at["D"]
    assert rs.record(at["E"], history[0])["parent"] == at["A"]                                       # while D is flagged E falls back to A
    assert rs.rounds()[:2] == (3, 6 + 2 + 1)


def test_rounds_over_two_tiles_on_the_host():
    seqs, weights, at = dc.two_tile_rounds_world()
    _, _, d, rs = _host(seqs, weights)
    want = dc.check_equal(d, rs, "two tiles")
    assert rs.n_par == 8232 and [rs.lim[at[k]] for k in ("C", "H", "D", "E", "X")] == [2, 8180, 8200, 8232, 8232] and len(rs.seqs[at["X"]]) > 1030
    rounds, scans, flagged = rs.rounds()
    history = rs.flag_history()
    assert [np.nonzero(h)[0].tolist() for h in history] == [[at["C"]], [at["C"], at["D"]], [at["C"], at["D"], at["E"]], [at["C"], at["D"], at["E"]]]
    assert (rounds, scans) == (4, 8240 + (8240 - 8180) + (8240 - 8232) + 0)
    assert want[at["H"]]["parent"] == at["H_head"] and want[at["X"]]["parent"] == at["X_head"] and want[at["X"]]["single"] > 690


def test_counts_at_the_class_edges():
    seqs, weights = dc.counts_world()
    for S in (16, 32):
        _, _, d, rs = _host(seqs, weights, segments=S)
        want = dc.check_equal(d, rs, f"counts S={S}")
        by_len = {len(s): r for s, r in zip(rs.seqs, want)}
        assert by_len[4097]["status"] == cc.TOO_LONG and by_len[7]["status"] == cc.NO_KMER and by_len[30]["status"] == cc.NO_KMER
        assert (by_len[4096]["single"], by_len[4096]["parent"]) == (4089, 0)        # the entry of 4097 bases is a parent
        assert (by_len[1031]["single"], by_len[1030]["single"]) == (1024, 1023) and by_len[1031]["parent"] == 0 and by_len[1031]["delta"] == 0
        assert by_len[13]["n_valid"] == 6 and by_len[13]["single"] == 6


def test_otu_mode_orders_the_seeds_by_otu_size():
    rng = np.random.default_rng(4)
    X, Y, Z = (dc.rand_seq(rng, 80) for _ in range(3))
    chim = np.concatenate([X[:40], Y[40:]])
    seqs = [Y, X] + [dc.substitute_at(X, (i,)) for i in (5, 25, 45, 65, 75)] + [Z, chim]
    weights = [20, 10, 3, 3, 3, 3, 3, 8, 2]
    table, o, d, (rs) = _host(seqs, weights, otus=True, segments=4, mindelta=8)
    rs, order = dc.of_otus(table, o, segments=4, mindelta=8)
    want = dc.check_equal(d, rs, "otus")
    assert rs.weights == [25, 20, 8, 2] and order == [1, 0, 2, 3] and [int(x) for x in d.otu] == order   # X's OTU overtakes Y's
    assert [int(x) for x in d.row] == [int(o.seed[k]) for k in order]
    assert want[3]["flag"] == 1 and {want[3]["parent_a"], want[3]["parent_b"]} == {0, 1}
    # the texts, against strings built here
    name = lambda e: "*" if e == dc.NO_REF else f"otu{order[e] + 1}"  # noqa: E731
    lines = ["#entry\tweight\tstatus\twindows\tsingle\tparent\tseg\tpos\tleft\ta\tright\tb\tdelta\tchimera"]
    for e, r in enumerate(want):
        lines.append("\t".join([name(e), str(rs.weights[e]), str(r["status"]), str(r["n_valid"]), str(r["single"]), name(r["parent"]), str(r["seg"]), str(r["pos"]),
                                str(r["left"]), name(r["parent_a"]), str(r["right"]), name(r["parent_b"]), str(r["delta"]),
                                "Y" if r["flag"] else ("N" if r["status"] == cc.OK else "?")]))
    assert rx.denovo_records_text(d) == "\n".join(lines) + "\n"
    all_fasta = rx.otu_fasta(o).splitlines()
    blocks = {all_fasta[i].split(";")[0][1:]: all_fasta[i:i + 2] for i in range(0, len(all_fasta), 2)}
    assert rx.denovo_fasta(d).splitlines() == blocks["otu1"] + blocks["otu2"] + blocks["otu3"]
    assert rx.denovo_fasta(d, minsize=9).splitlines() == blocks["otu1"] + blocks["otu2"]
    all_table = rx.otu_table_text(o, ["all"]).splitlines()
    assert rx.denovo_table_text(d, ["all"]).splitlines() == all_table[:4] and rx.denovo_table_text(d, ["all"], minsize=21).splitlines() == [all_table[0], all_table[2]]


def test_texts_without_otus():
    seqs, weights = dc.rounds_world()
    table, _, d, rs = _host(seqs, weights)
    text = rx.denovo_records_text(d).splitlines()
    assert text[3].split("\t")[:6] == ["uniq3", "100", "0", "193", str(d.rec[2]["single"]), "uniq1" if d.rec[2]["parent"] == 0 else "uniq2"] and text[3].endswith("\tY")
    assert text[1].split("\t")[2:] == ["3", "0", "0", "*", "0", "0", "0", "*", "0", "*", "0", "?"]
    assert rx.denovo_fasta(d) == "".join(rx.tally_fasta(table).splitlines(keepends=True)[:4])
    assert rx.denovo_table_text(d, ["all"]) == "".join(rx.tally_table_text(table, ["all"]).splitlines(keepends=True)[:3])
    assert rx.denovo_fasta(d, minsize=901) == "".join(rx.tally_fasta(table).splitlines(keepends=True)[:2])


def test_refusals():
    seqs, weights = dc.rounds_world()
    table = dc.table_of(rx, seqs, weights)
    for bad in (dict(segments=1), dict(segments=33), dict(abskew=0), dict(flags=1), dict(max_parents=262145)):
        for fn in (rx.denovo_check_host, rx.denovo_check):   # (refused before a device is looked for)
            with pytest.raises(rx.RtxError) as e:
                fn(table, **bad)
            assert e.value.code == -1, bad
    other = rx.otu_cluster_host(dc.table_of(rx, seqs[:3], weights[:3]))
    with pytest.raises(rx.RtxError) as e:
        rx.denovo_check_host(table, other)
    assert e.value.code == -1
    d = rx.denovo_check_host(table)
    d.otus = other                                           # a result made without OTUs, formatted with some
    with pytest.raises(rx.RtxError):
        rx.denovo_fasta(d)
    empty = rx.denovo_check_host(dc.table_of(rx, [], []))
    assert empty.n_entries == 0 and rx.denovo_fasta(empty) == "" and len(rx.denovo_records_text(empty).splitlines()) == 1


def test_planted_chimeras_are_found_by_the_definition():
    reads, templates, chimeras = dc.planted_world()
    table, o, d, _ = _host([s for s, _ in reads], [w for _, w in reads], otus=True)
    rs, order = dc.of_otus(table, o)
    want = dc.check_equal(d, rs, "planted")
    flag_of = {bytes(rs.seqs[e]): want[e]["flag"] for e in range(rs.n)}
    assert all(flag_of[bytes(c)] == 1 for c in chimeras) and not any(flag_of[bytes(t)] for t in templates)
    assert sum(flag_of.values()) == len(chimeras)


def _allow(emul, n_parents, tile, lim):
    out = np.zeros((64, 4), np.uint32)
    emul.emul_denovo_allow.restype = C.c_uint32
    L = emul.emul_denovo_allow(n_parents, tile, lim, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return L, out


def test_emul_prefix_mask_over_every_lane_count(emul):
    """Bit b of word w of lane l is the local entry ((4 w + b // 8) L + l) 8 + b % 8 (ref_slot inverted): allowed iff it lies below lim."""
    for L in range(1, 65):
        n_parents = 8192 + L * 128 - 5                      # a full tile and a last tile of L lanes
        got_L, _ = _allow(emul, n_parents, 1, 0)
        assert got_L == L
        w, b, lane = np.meshgrid(np.arange(4), np.arange(32), np.arange(64), indexing="ij")
        entry = 8192 + ((4 * w + b // 8) * L + lane) * 8 + b % 8
        for lim in sorted({0, 1, 8191, 8192, 8193, 8192 + 7, 8192 + 8, 8192 + 9, 8192 + L * 64, n_parents - 1, n_parents, 8192 + L * 128, 300000}):
            _, out = _allow(emul, n_parents, 1, lim)
            want = np.zeros((64, 4), np.uint32)
            ok = (entry < lim) & (lane < L)
            np.bitwise_or.at(want, (lane[ok], w[ok]), (1 << b[ok]).astype(np.uint32))
            assert np.array_equal(out, want), (L, lim)
        _, full = _allow(emul, n_parents, 0, 8192)          # the tile in front is full whatever the last one is
        assert (full == 0xFFFFFFFF).all()
        _, part = _allow(emul, n_parents, 0, 513)
        assert int(sum(bin(int(x)).count("1") for x in part.reshape(-1))) == 513


@pytest.mark.parametrize("planes", (10, 12))
def test_emul_masked_checkpoint(emul, planes):
    rng = np.random.default_rng(planes)
    p16, p8, p32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)

    def run(counts, live, n_parents, tile, lim):
        m, r = C.c_uint32(), C.c_uint32()
        assert emul.emul_denovo_checkpoint(counts.ctypes.data_as(p16), live.ctypes.data_as(p8), planes, n_parents, tile, lim, C.byref(m), C.byref(r)) == 0
        return m.value, r.value

    top = (1 << planes) - 1
    for L in (1, 2, 5, 63, 64):
        n_parents = 8192 + L * 128 - 3
        in_tile = n_parents - 8192
        for lim in (8192, 8193, 8192 + 9, 8192 + in_tile // 2, n_parents):
            counts = np.zeros(8192, np.uint16)
            counts[:in_tile] = rng.integers(0, 40, in_tile)
            live = (rng.random(8192) < 0.7).astype(np.uint8)
            hot = rng.integers(0, in_tile, 6)
            counts[hot] = top                                 # ties at the top, some of them outside lim or dead
            ok = (np.arange(8192) + 8192 < lim) & (live != 0)
            masked = np.where(ok, counts, 0)
            want = (int(masked.max()), 8192 + int(np.argmax(masked))) if masked.max() else (0, cc.NO_REF)
            assert run(counts, live, n_parents, 1, lim) == want, (L, lim)
        counts = np.full(8192, 3, np.uint16)
        assert run(counts, np.zeros(8192, np.uint8), n_parents, 1, n_parents) == (0, cc.NO_REF)      # nobody lives
        assert run(counts, np.ones(8192, np.uint8), n_parents, 0, 1) == (3, 0)                       # a prefix of one entry
    assert emul.emul_denovo_checkpoint(None, None, 9, 8192, 0, 1, None, None) == -1


def _cli(*args):
    return subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=120)


def test_cli_refuses_denovo_without_otus(tmp_path):
    db = tmp_path / "db.fasta"
    db.write_text(">a;tax=k:K,p:P,c:C,o:O,f:F,g:G,s:S\nACGTACGTACGTACGTACGT\n")
    common = ["-d", db, "-i", db, "-o", tmp_path / "out"]
    for extra in (["--denovo"], ["--uniques", "--denovo"], ["--uniques", "--otus", "--denovo-abskew", "3"], ["--uniques", "--otus", "--denovo-mindelta", "3"],
                  ["--uniques", "--otus", "--denovo-segments", "8"], ["--uniques", "--otus", "--denovo", "--denovo-abskew", "0"],
                  ["--uniques", "--otus", "--denovo", "--denovo-segments", "33"]):
        p = _cli(*common, *extra)
        assert p.returncode == 64, (extra, p.returncode, p.stderr)
        assert "denovo" in p.stderr, (extra, p.stderr)

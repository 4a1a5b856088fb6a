"""Denoising without a device: rtx_otu_unoise_host (host_unoise.cpp) against the numpy restatement of the definition (tests/unoise_common.py) on
every world, field by field; the distance the lanes of the pair kernel run (rtx_math.hpp through the x86 emulator) against the plain dynamic
programme, exhaustively on short strings and at random at the band's and the words' edges; every world that test_gpu_unoise.py puts on the
device proven a fixture by the restatement alone; the symbols, the refusals, the text and the command line's refusals."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
import unoise_common as uc
from raxtax_amd import _lib
from unoise_common import ABSORBED, LEFT, LONG, NONE, ZOTU

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
NO_DIST = 0xFFFFFFFF


def test_symbols_are_declared_bound_and_exported():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    lib = _lib.load()
    for name in ("rtx_otu_unoise", "rtx_otu_unoise_host", "rtx_otu_unoise_view", "rtx_otu_format_unoise"):
        assert name + "(" in header and name in _lib._SIGNATURES and getattr(lib, name) is not None, name
    for text in ("#define RTX_UNOISE_MAX_DIFFS 16\n", "#define RTX_UNOISE_ZOTU 0\n", "#define RTX_UNOISE_ABSORBED 1\n", "#define RTX_UNOISE_LEFT 2\n", "#define RTX_UNOISE_LONG 3\n",
                 "#define RTX_DEFAULT_UNOISE_SLICE ", "rtx_unoise_params;", "rtx_unoise_view_t;", "#define RTX_ABI_VERSION 6 "):
        assert text in header, text
    assert (_lib.RTX_UNOISE_ZOTU, _lib.RTX_UNOISE_ABSORBED, _lib.RTX_UNOISE_LEFT, _lib.RTX_UNOISE_LONG, _lib.RTX_UNOISE_MAX_DIFFS) == (0, 1, 2, 3, 16)
    assert f"#define RTX_DEFAULT_UNOISE_SLICE {_lib.RTX_DEFAULT_UNOISE_SLICE} " in header
    for name in ("UnoiseParams", "otu_unoise", "otu_unoise_host", "unoise_text"):
        assert name in rx.__all__ and hasattr(rx, name), name
    # the slice option is read at every call and means nothing to the host walk
    try:
        assert lib.rtx_set_default_option(_lib.RTX_DEFAULT_UNOISE_SLICE, 1) == 0
        table = uc.tiers_world()[0]
        uc.assert_unoise(rx.otu_unoise_host(table), uc.solved("tiers", table))
    finally:
        assert lib.rtx_set_default_option(_lib.RTX_DEFAULT_UNOISE_SLICE, 0) == 0


@pytest.mark.parametrize("key", [w[0] for w in uc.all_worlds()])
def test_host_against_the_restatement(key):
    _, table, params = next(w for w in uc.all_worlds() if w[0] == key)
    got = rx.otu_unoise_host(table, **params)
    uc.assert_unoise(got, uc.solved(key, table, **params))
    u = got.unoise
    assert u["tiers"] == u["launches"] == u["pairs"] == u["pairs_length"] == u["pairs_finished"] == 0 and u["seconds"] == (0, 0, 0, 0)


# ---- the distance of the lanes ---------------------------------------------------------------------------------------------------------------

def _emul_distance(emul):
    fn = emul.emul_unoise_distance
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32]
    return lambda x, y, k: fn(bytes(x), len(x), bytes(y), len(y), k)


def test_emul_distance_on_every_short_pair(emul):
    """all pairs of strings over {A, C} of up to 7 codes, k = 0 .. 7: d when d <= k, nothing otherwise"""
    dist = _emul_distance(emul)
    strings = [np.array(p, np.uint8) for n in range(8) for p in itertools.product((1, 2), repeat=n)]
    bad = []
    for x in strings:
        d = uc.lev_many(x, strings) if len(x) else np.array([len(y) for y in strings])
        for y, dy in zip(strings, d):
            for k in range(8):
                got = dist(x, y, k)
                if got != (dy if dy <= k else NO_DIST):
                    bad.append((bytes(x), bytes(y), k, got, int(dy)))
    assert not bad, bad[:5]


@pytest.mark.parametrize("m", uc.LENGTHS + (200, 500, 4096))
def test_emul_distance_at_random(emul, m):
    """a pattern of every edge length against texts 0 .. 20 edits away -- at the first code, the last code and anywhere -- and against an
    unrelated text; k over 0, 1, 2, 3, 8, 15, 16"""
    dist = _emul_distance(emul)
    rng = np.random.default_rng(m)
    for t in range(6 if m > 1000 else 40):
        x = uc.random_seq(rng, m)
        if t % 5 == 0:
            x[:] = (1 << rng.integers(0, 2, m))          # two letters only: many alignments tie
        y = x.copy()
        for _ in range(int(rng.integers(0, 21))):
            kind, where = int(rng.integers(3)), int(rng.integers(3))
            if kind == 0 and len(y):
                y = uc.sub_at(rng, y, (0, len(y) - 1, int(rng.integers(len(y))))[where])
            elif kind == 1 and len(y) > 1:
                y = uc.delete_at(y, (0, len(y) - 1, int(rng.integers(len(y))))[where])
            else:
                y = np.insert(y, (0, len(y), int(rng.integers(len(y) + 1)))[where], 1 << int(rng.integers(4)))
        if t % 7 == 3:
            y = uc.random_seq(rng, max(1, m + int(rng.integers(-5, 6))))
        d = uc.lev(x, y)
        for k in (0, 1, 2, 3, 8, 15, 16):
            want = d if d <= k and abs(len(x) - len(y)) <= k else NO_DIST
            assert dist(x, y, k) == want, (m, t, k, d)
            assert dist(y, x, k) == want, (m, t, k, d, "swapped")
    assert dist(x, y, 17) == NO_DIST                     # (a threshold the band does not cover is refused)


def test_emul_allowed_differences(emul):
    fn = emul.emul_unoise_allowed
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    rng = np.random.default_rng(3)
    for _ in range(4000):
        alpha, maxd = int(rng.integers(1, 9)), int(rng.integers(1, 17))
        we = int(rng.integers(1, 1 << int(rng.integers(1, 40))))
        wp = min((1 << 64) - 1, (we << int(rng.integers(0, 60))) + int(rng.integers(-1, 2)))
        assert fn(wp, we, alpha, maxd) == uc.allowed(wp, we, alpha, maxd), (wp, we, alpha, maxd)


# ---- the worlds are what they claim to be, by the restatement alone -------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", (1, 2, 3))
def test_skew_world(alpha):
    table, m, params = uc.skew_world(alpha)
    s = uc.solved(f"skew{alpha}", table, **params)
    w = table.sizes
    for d in (1, 2, 3):
        c, r = m[f"at{d}"], m[f"at{d}_read"]
        assert int(w[c]) == int(w[r]) << (alpha * d + 1) and s["status"][r] == ABSORBED and s["parent"][r] == c and s["dist"][r] == d
        c, r = m[f"below{d}"], m[f"below{d}_read"]
        assert int(w[c]) == (int(w[r]) << (alpha * d + 1)) - 1 and s["status"][r] == ZOTU and s["parent"][r] == NONE
    if alpha <= 2:
        c = m["cap"]
        assert int(w[c]) > 1 << (40 if alpha == 2 else 20) and uc.allowed(w[c], 100, alpha, 16) == 16 and uc.allowed(w[c], 100, alpha, 17) == 17
        assert s["status"][m["cap_read16"]] == ABSORBED and s["dist"][m["cap_read16"]] == 16 and s["status"][m["cap_read17"]] == ZOTU


def test_shift_world():
    table, m, params = uc.shift_world()
    s = uc.solved("shift", table, **params)
    assert int(table.sizes[m["heavy"]]) == 1 << 62 and 8 * 8 + 1 >= 64 and uc.allowed(1 << 62, 1, 8, 16) == 7
    assert s["status"][m["read7"]] == ABSORBED and s["dist"][m["read7"]] == 7 and s["status"][m["read8"]] == LEFT


def test_distance_world():
    table, m, cases = uc.distance_world()
    s = uc.solved("distance", table)
    seqs = table.seqs
    assert {k for _, k in cases} == {1, 2, 3, 16} and len(cases) >= 6 * 3 + 2 + 3
    for name, k in cases:
        c, near, far = m[name], m[name + "_near"], m[name + "_far"]
        assert uc.allowed(table.sizes[c], 2, 2, 16) == k, name
        assert uc.lev(seqs[near], seqs[c]) == k and uc.lev(seqs[far], seqs[c]) == k + 1, name
        assert s["status"][near] == ABSORBED and s["parent"][near] == c and s["dist"][near] == k, name
        assert s["status"][far] == LEFT and s["parent"][far] == NONE and s["dist"][far] == NONE, name
    # what the kinds claim
    for k in (1, 2, 3):
        c = seqs[m[f"ins{k}"]]
        assert len(seqs[m[f"ins{k}_near"]]) == len(c) + k and len(seqs[m[f"ins{k}_far"]]) == len(c) + k + 1       # the length test drops the far one
        assert len(seqs[m[f"dels{k}_near"]]) == len(seqs[m[f"dels{k}"]]) - k
        assert len(seqs[m[f"indel_first{k}_near"]]) == len(seqs[m[f"indel_first{k}"]]) - 1
        last = seqs[m[f"indel_last{k}_near"]]
        assert len(last) == len(seqs[m[f"indel_last{k}"]]) + 1
    c, near = seqs[m["indel_first1"]], seqs[m["indel_first1_near"]]
    assert np.array_equal(near, c[1:]) and (near != c[:-1]).sum() > 40
    c = seqs[m["homopolymer1"]]
    assert (c[40:52] == 1).all() and len({bytes(np.delete(c, i)) for i in range(40, 52)}) == 1
    c, near, far = seqs[m["ambiguous1"]], seqs[m["ambiguous1_near"]], seqs[m["ambiguous1_far"]]
    assert c[30] == 15 and near[30] == 1 and (near != c).sum() == 1 and (far != c).sum() == 2      # N against A is a mismatch: the far read is two away
    c, near = seqs[m["same_code1"]], seqs[m["same_code1_near"]]
    assert c[30] == 15 and near[30] == 15 and (near != c).sum() == 1                               # N against N is a match: one away


def test_lengths_worlds():
    table, m = uc.lengths_world()
    s = uc.solved("lengths", table)
    for n in uc.LENGTHS:
        c = m[f"len{n}"]
        assert len(table.seqs[c]) == n and s["status"][c] == ZOTU
        for r in [m[f"len{n}_sub"]] + ([m[f"len{n}_del"]] if n >= 15 else []):
            assert s["status"][r] == ABSORBED and s["parent"][r] == c and s["dist"][r] == 1, n
    table, m = uc.short_world()
    s = uc.solved("short", table)
    r = m["short"]
    assert len(table.seqs[r]) == 3 < uc.allowed(table.sizes[m["centre"]], 2, 2, 16) == 16 and s["status"][r] == ABSORBED and s["dist"][r] == 7
    table, m = uc.long_world()
    s = uc.solved("long", table)
    assert len(table.seqs[m["max"]]) == len(table.seqs[m["max_read"]]) == 4096 and s["status"][m["max"]] == ZOTU
    assert s["status"][m["max_read"]] == ABSORBED and s["parent"][m["max_read"]] == m["max"] and s["dist"][m["max_read"]] == 1
    assert len(table.seqs[m["long"]]) == 4097 and s["status"][m["long"]] == LONG == s["status"][m["long_too"]] and s["long_rows"] == 2
    copy = m["long_copy"]
    assert len(table.seqs[copy]) == 4096 and uc.lev(table.seqs[copy], table.seqs[m["long"]]) == 1 and s["lim"][copy] > m["long"]
    assert s["status"][copy] == LEFT and s["parent"][copy] == NONE
    assert s["seed"][s["otu"][m["long"]]] == m["long"] and s["members"][s["otu"][m["long"]]] == 1          # an OTU of its own


def test_ties_worlds():
    table, m = uc.ties_world()
    s = uc.solved("ties", table)
    seqs = table.seqs
    r = m["tie_read"]
    assert m["p1"] < m["p2"] and s["status"][m["p2"]] == ZOTU and uc.lev(seqs[r], seqs[m["p1"]]) == uc.lev(seqs[r], seqs[m["p2"]]) == 1
    assert s["parent"][r] == m["p1"] and s["dist"][r] == 1
    r = m["near_read"]
    assert m["q1"] < m["q2"] and s["status"][m["q2"]] == ZOTU and uc.lev(seqs[r], seqs[m["q1"]]) == 3 == uc.allowed(table.sizes[m["q1"]], 2, 2, 16)
    assert uc.lev(seqs[r], seqs[m["q2"]]) == 1 and s["parent"][r] == m["q2"] and s["dist"][r] == 1
    for n in (65, 128, 129):
        table, m, at = uc.lanes_world(n)
        s = uc.solved(f"lanes{n}", table)
        assert s["n_zotu"] == n and all(s["status"][m[f"c{i}"]] == ZOTU and m[f"c{i}"] == i for i in range(n))     # the list position is the rank
        assert set(at) == {p for p in (0, 63, 64, 65, n - 1) if p < n}
        for p in at:
            assert s["parent"][m[f"read{p}"]] == p and s["dist"][m[f"read{p}"]] == 1 and s["lim"][m[f"read{p}"]] == n


def test_the_greedy_rule():
    table, m, params = uc.greedy_world()
    s = uc.solved("greedy", table, **params)
    seqs = table.seqs
    a, b, c = m["A"], m["B"], m["C"]
    assert [int(table.sizes[r]) for r in (a, b, c)] == [1000, 100, 10]
    assert uc.lev(seqs[b], seqs[a]) == 1 and uc.lev(seqs[c], seqs[b]) == 1 and uc.lev(seqs[c], seqs[a]) == 2
    assert uc.allowed(100, 10, 2, 1) == 1 and uc.allowed(1000, 10, 2, 1) == 1 < 2                 # B would absorb C, A may not
    assert s["status"][b] == ABSORBED and s["parent"][b] == a and s["status"][c] == ZOTU
    everybody = uc.solve_table(table, everybody_live=True, **params)
    assert everybody["status"][c] == ABSORBED and everybody["parent"][c] == b


def test_small_rows():
    table, m, params = uc.small_world()
    s = uc.solved("small", table, **params)
    w = table.sizes
    r = m["small_absorbed"]
    assert w[r] < 100 and s["status"][r] == ABSORBED and s["parent"][r] == m["centre"]
    assert w[m["small_left"]] < 100 and s["status"][m["small_left"]] == LEFT
    p, c = m["small_parent"], m["small_child"]
    assert s["status"][p] == LEFT and uc.allowed(w[p], w[c], 2, 16) >= 1 == uc.lev(table.seqs[p], table.seqs[c]) and s["status"][c] == LEFT and s["lim"][c] > p
    one = uc.solved("small_minsize1", table, minsize=1)
    assert one["status"][p] == ZOTU and one["status"][c] == ABSORBED and one["parent"][c] == p and one["n_left"] == 0


def test_the_tier_cut():
    """tiers of one row, equal weights, and a weight at exactly 2^(alpha + 1) times the next: inside a tier no row has a candidate in it, and
    the row behind a tier has the tier's first row as one"""
    table, m = uc.tiers_world()
    s = uc.solved("tiers", table)
    assert [int(x) for x in table.sizes] == [80, 11, 10] and uc.tiers_of(table.sizes, 2) == [0, 2, 3]
    assert (m["parent"], m["last_of_tier"], m["first_of_next"]) == (0, 1, 2)
    assert s["status"][1] == ZOTU and s["lim"][1] == 0 and s["status"][2] == ABSORBED and s["parent"][2] == 0 and s["lim"][2] == 1
    table, m = uc.one_tier_world()
    s = uc.solved("one_tier", table)
    assert uc.tiers_of(table.sizes, 2) == [0, 20] and s["n_zotu"] == 20 and not s["lim"].any()
    table, m = uc.row_tiers_world()
    s = uc.solved("row_tiers", table)
    assert uc.tiers_of(table.sizes, 2) == list(range(9)) and s["n_absorbed"] == 7 and (s["parent"][1:] == 0).all()
    assert uc.tiers_of([5, 5, 5, 5], 2) == [0, 4] and uc.tiers_of([7], 1) == [0, 1] and uc.tiers_of([], 2) == [0]
    rng = np.random.default_rng(9)
    for alpha in range(1, 9):
        sizes = np.sort(rng.integers(1, 1 << 62, 300).astype(np.uint64) >> rng.integers(0, 62, 300).astype(np.uint64))[::-1] + np.uint64(1)
        cut = uc.tiers_of(sizes, alpha)
        lim = uc.lim_of(sizes, alpha)
        assert len(cut) - 1 <= 64 // (alpha + 1) + 1
        for a, b in zip(cut, cut[1:]):
            assert (lim[a:b] <= a).all()                                         # no row of a tier is a candidate of another
            assert b == len(sizes) or lim[b] > a                                 # ... and the cut is not early


def test_planted_world():
    table, m, variants = uc.planted_world()
    s = uc.solved("planted", table)
    assert len(table.seqs) == 400 and s["n_zotu"] == 40 and s["n_absorbed"] == 360
    assert all(s["status"][m[f"centre{i}"]] == ZOTU for i in range(40))
    for name, (centre, d) in variants.items():
        assert s["parent"][m[name]] == m[centre] and s["dist"][m[name]] == d, name


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    table = uc.tiers_world()[0]
    for bad in (dict(alpha=0), dict(alpha=9), dict(minsize=0), dict(max_diffs=17), dict(flags=1)):
        for fn in (rx.otu_unoise_host, rx.otu_unoise):   # (refused before a device is looked for)
            with pytest.raises(rx.RtxError) as e:
                fn(table, **bad)
            assert e.value.code == -1, bad
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.rtx_otu_unoise_host(table._h, None, C.byref(h)))          # params == NULL: the defaults
    default = rx.Otus(h, table)._read_unoise()
    assert (default.unoise["minsize"], default.unoise["alpha"], default.unoise["max_diffs"]) == (8, 2, 16)
    uc.assert_unoise(default, uc.solved("tiers", table))
    for fn in (rx.unoise_text, lambda o: o._read_unoise()):                  # any other rtx_otu is refused
        with pytest.raises(rx.RtxError) as e:
            fn(rx.otu_cluster_host(table))
        assert e.value.code == -1
    empty = rx.otu_unoise_host(uc.table_of_weights([np.array([1], np.uint8)], [1]), minsize=1)
    assert empty.n_otus == 1 and rx.unoise_text(empty) == "#read\tsize\tstatus\tparent\tdiffs\totu\nuniq1\t1\tzotu\t*\t*\totu1\n"


def test_the_text_of_five_rows():
    A = [1, 2, 4, 8, 1, 2, 4, 8, 1, 2]
    seqs = [A, A[:4] + [2] + A[5:], [8] * 4097, [4] * 12, [2] * 9]          # a centre, a read one substitution away, a long row, a ZOTU, a small row
    table = uc.table_of_weights([np.array(s, np.uint8) for s in seqs], [64, 8, 5, 9, 3])
    got = rx.otu_unoise_host(table)
    assert [int(x) for x in table.sizes] == [64, 9, 8, 5, 3] and [len(s) for s in table.seqs] == [10, 12, 10, 4097, 9]
    assert rx.unoise_text(got) == ("#read\tsize\tstatus\tparent\tdiffs\totu\n"
                                   "uniq1\t64\tzotu\t*\t*\totu1\n"
                                   "uniq2\t9\tzotu\t*\t*\totu2\n"
                                   "uniq3\t8\tabsorbed\tuniq1\t1\totu1\n"
                                   "uniq4\t5\tlong\t*\t*\totu3\n"
                                   "uniq5\t3\tleft\t*\t*\totu4\n")
    n = len(rx.unoise_text(got))
    lib = _lib.load()
    small = C.create_string_buffer(8)
    assert lib.rtx_otu_format_unoise(got._h, None, 0) == n and lib.rtx_otu_format_unoise(got._h, small, 8) < -n      # the protocol of rtx_tally_format_fasta


def test_the_object_goes_downstream():
    table, m, _ = uc.planted_world()
    got = rx.otu_unoise_host(table)
    s = uc.solved("planted", table)
    fasta = rx.otu_fasta(got, minsize=8).split("\n")
    assert len(fasta) == 2 * 40 + 1 and fasta[0] == f">otu1;size={int(s['sizes'][0])};seed=uniq1"
    assert rx.otu_map_text(got).splitlines()[5] == f"uniq6\totu{int(s['otu'][5]) + 1}"
    assert rx.otu_table_text(got, ["all"]).splitlines()[1] == f"otu1\t{int(s['sizes'][0])}"
    dn = rx.denovo_check_host(table, got)
    assert dn.n_entries == got.n_otus == 40 and len(rx.denovo_records_text(dn).splitlines()) == 41


def _cli(*args):
    return subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=120)


def test_cli_refusals(tmp_path):
    db = tmp_path / "db.fasta"
    db.write_text(">a;tax=k:K,p:P,c:C,o:O,f:F,g:G,s:S\nACGTACGTACGTACGTACGT\n")
    common = ["-d", db, "-i", db, "-o", tmp_path / "out"]
    for extra in (["--unoise"], ["--uniques", "--unoise"], ["--uniques", "--otus", "--unoise-minsize", 4], ["--uniques", "--otus", "--unoise-alpha", 2],
                  ["--uniques", "--otus", "--unoise-maxdiffs", 3], ["--uniques", "--otus", "--unoise", "--fastidious"], ["--uniques", "--otus", "--unoise", "--unoise-alpha", 9],
                  ["--uniques", "--otus", "--unoise", "--unoise-alpha", 0], ["--uniques", "--otus", "--unoise", "--unoise-maxdiffs", 17],
                  ["--uniques", "--otus", "--unoise", "--unoise-minsize", 0]):
        p = _cli(*common, *extra)
        assert p.returncode == 64, (extra, p.returncode, p.stderr)
        assert "unoise" in p.stderr, (extra, p.stderr)
    assert not (tmp_path / "out" / "raxtax.out").exists()

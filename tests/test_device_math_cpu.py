"""Runs the device arithmetic of raxtax_amd/csrc/rtx_math.hpp (the inline functions the HIP
kernels call) on the CPU through a small emulation harness and checks it against the oracle:
bit-sliced counters must be bit-exact, the linear-domain pmf recurrence must reproduce the
reference's log-space probability table."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from raxtax_amd import synth

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("planes,n_rows,density", [(10, 648, 0.3), (10, 1016, 0.97), (12, 4088, 0.5), (16, 8000, 0.9)])
def test_bit_planes_exact(emul, planes, n_rows, density):
    rng = np.random.default_rng(planes * 1000 + n_rows)
    bits = rng.random((n_rows, 32)) < density
    rows = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    out = np.zeros(32, dtype=np.uint32)
    emul.emul_planes_count(rows.ctypes.data_as(C.c_void_p), n_rows, planes, out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out, bits.sum(axis=0).astype(np.uint32))


ALL_PLANES = (8, 10, 11, 12, 16)     # every plane count the counting kernels are instantiated with


def _column_words(col_counts, n_rows, rng=None):
    """n_rows words whose column r is set in exactly col_counts[r] rows: the first ones, or (rng) a random choice of them."""
    bits = np.zeros((n_rows, 32), bool)
    for r, c in enumerate(col_counts):
        assert 0 <= c <= n_rows
        idx = np.arange(c) if rng is None else rng.choice(n_rows, c, replace=False)
        bits[idx, r] = True
    rows = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    return bits, np.ascontiguousarray(rows)


def _planes_count(emul, rows, planes, sched):
    out = np.zeros(32, dtype=np.uint32)
    emul.emul_planes_count_sched.restype = C.c_int
    rc = emul.emul_planes_count_sched(rows.ctypes.data_as(C.c_void_p), C.c_uint32(len(rows)), planes, sched, out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out


@pytest.mark.parametrize("sched", [32, 24])
@pytest.mark.parametrize("planes", ALL_PLANES)
def test_bit_planes_saturated_and_carry_columns(emul, planes, sched):
    """Counts where a plane adder goes wrong unnoticed by random densities: a column set in all 2^NP - 1 rows (every plane set) beside
    an empty one and one of 2^NP - 2, and columns on either side of every carry boundary (2^k - 1, 2^k for every k < NP) -- through
    the 32-row schedule of hit_count and the 24-row schedule of the pair kernel, the three unpack forms agreeing (a poisoned counter
    fails the comparison)."""
    full = (1 << planes) - 1
    n_rows = (full + 7) // 8 * 8
    cols = [full, 0, full - 1]
    for k in range(planes):
        cols += [(1 << k) - 1, 1 << k]
    assert len(cols) == 3 + 2 * planes
    for rng in (None, np.random.default_rng(planes * 100 + sched)):     # the set rows in front (every carry chain at once), then scattered
        for a in range(3, len(cols), 29):                               # 32 columns per word: the saturated three beside every chunk
            chunk = (cols[:3] + cols[a:a + 29] + [0] * 32)[:32]
            bits, rows = _column_words(chunk, n_rows, rng)
            want = bits.sum(axis=0).astype(np.uint32)
            assert list(want) == chunk
            assert np.array_equal(_planes_count(emul, rows, planes, sched), want)


@pytest.mark.parametrize("sched", [32, 24])
@pytest.mark.parametrize("planes", ALL_PLANES)
def test_bit_planes_every_row_count_residue(emul, planes, sched):
    """n_rows at every residue of 8 modulo 24 and modulo 32 (the tails of both schedules; the pair kernel pads its last group with the
    zero row), from no full group to several, every column full -- the count equals n_rows, the largest it can be."""
    top = min(255 if planes == 8 else 1 << 30, (1 << planes) - 1)
    rng = np.random.default_rng(planes)
    for n_rows in [n for n in range(0, 224, 8) if n <= top]:       # 0 .. 216: every residue of 8 mod 24 and mod 32 at least twice
        bits = rng.random((n_rows, 32)) < 0.9
        bits[:, 0] = True                                             # a column that holds every row
        rows = np.ascontiguousarray((bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
        got = _planes_count(emul, rows, planes, sched)
        assert np.array_equal(got, bits.sum(axis=0).astype(np.uint32)), n_rows
        assert got[0] == n_rows
    assert {n % 24 for n in range(0, 224, 8)} == {0, 8, 16} and {n % 32 for n in range(0, 224, 8)} == {0, 8, 16, 24}


def test_bit_planes_refuse_what_they_do_not_cover(emul):
    rows = np.zeros(8, np.uint32)
    out = np.full(32, 7, np.uint32)
    emul.emul_planes_count_sched.restype = C.c_int
    for planes, n, sched in ((9, 8, 32), (10, 7, 32), (10, 8, 16)):
        assert emul.emul_planes_count_sched(rows.ctypes.data_as(C.c_void_p), C.c_uint32(n), planes, sched, out.ctypes.data_as(C.c_void_p)) == -1
    assert (out == 7).all()


@pytest.mark.parametrize("planes", ALL_PLANES)
def test_planes_gt_against_the_counts(emul, planes):
    """planes_gt (rec_epilogue's candidates above a threshold, rtx_math.hpp) against counts > c, on columns of 0, c - 1, c, c + 1 and
    2^NP - 1, for c on either side of every carry boundary and at both ends."""
    full = (1 << planes) - 1
    cs = {0, 1, full - 1, full}
    for k in range(planes):
        cs |= {(1 << k) - 1, 1 << k}
    emul.emul_planes_gt.restype = C.c_int
    rng = np.random.default_rng(planes)
    for c in sorted(cs):
        special = [v for v in (0, c - 1, c, c + 1, full) if 0 <= v <= full]
        counts = np.array((special * 16)[:32], np.uint32)
        counts[10:] = rng.permutation(counts[10:])                  # every special value at several bit positions
        counts[-6:] = rng.integers(0, full + 1, 6)
        mask = C.c_uint32()
        assert emul.emul_planes_gt(counts.ctypes.data_as(C.c_void_p), planes, C.c_uint32(c), C.byref(mask)) == 0
        want = sum(1 << r for r in range(32) if counts[r] > c)
        assert mask.value == want, (c, counts.tolist(), hex(mask.value), hex(want))
        assert c in counts.tolist() and (c == full or c + 1 in counts.tolist())   # the values the comparison must tell apart were there


def _tile_word_counts(emul, rows, sparse, planes, sched=32):
    out = np.zeros(32, np.uint32)
    emul.emul_tile_word_counts.restype = C.c_int
    sp = np.ascontiguousarray(sparse, np.uint8)
    assert emul.emul_tile_word_counts(rows.ctypes.data_as(C.c_void_p), sp.ctypes.data_as(C.c_void_p), C.c_uint32(len(rows)), planes, sched,
                                      out.ctypes.data_as(C.c_void_p)) == 0
    return out


@pytest.mark.parametrize("planes,n_sparse", [(p, n) for p in ALL_PLANES for n in (0, 1, 127, 254, 255, 256, 300)
                                             if p > 8 or n <= 255])     # (eight planes: t <= 255, a query has no more rows)
def test_sparse_cap_and_dense_remainder_of_a_tile_word(emul, planes, n_sparse):
    """The counts of a (query, tile) word as the kernels split them: at most kSegMaxSparseRows = 255 sparse segments through byte
    counters, the rest and the dense rows through the planes, then the merge (eight planes: the byte-wise add).  A reference that
    sits in every sparse row reaches the cap exactly at 255 -- handled as 256, its byte counter wraps and carries into its
    neighbour's, which holds a count that is checked."""
    full = (1 << planes) - 1
    n_dense = min(full, 1023) - n_sparse         # reference 5 ends at the largest count of the class (1023 beyond ten planes)
    n = n_sparse + n_dense
    bits = np.zeros((n, 32), bool)
    sparse = np.zeros(n, np.uint8)
    sparse[:n_sparse] = 1
    bits[:n_sparse, 4] = True           # reference 4: in every sparse row and no dense one (0 + 255 at the cap)
    bits[:, 5] = True                   # its neighbour in the word: every row (dense + sparse = the largest count)
    bits[n_sparse:, 6] = True           # dense rows only
    bits[:min(n_sparse, 1), 7] = True   # one sparse row
    bits[::3, 9] = True
    bits[:n_sparse:2, 2] = True
    rows = np.ascontiguousarray((bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
    for sched in (32, 24):
        got = _tile_word_counts(emul, rows, sparse, planes, sched)
        assert np.array_equal(got, bits.sum(axis=0).astype(np.uint32)), (got.tolist(), bits.sum(axis=0).tolist())


@pytest.mark.parametrize("groups,n_rows,density", [(4, 1024, 0.3), (16, 1024, 0.9), (4, 128, 0.02), (16, 896, 0.5)])
def test_grouped_bit_planes_of_the_two_level_bounds(emul, groups, n_rows, density):
    """rtx_bounds2.hip: R lane groups fold different rows of the same columns, their bit-sliced partial counters are added pairwise
    (planes_add), the largest counter is read off the planes (planes_max): totals and maximum exact, the lowest counter among equals."""
    rng = np.random.default_rng(groups * 10000 + n_rows)
    bits = rng.random((n_rows, 32)) < density
    rows = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    out = np.zeros(32, dtype=np.uint32)
    emul.emul_planes_grouped.restype = C.c_uint32
    key = emul.emul_planes_grouped(rows.ctypes.data_as(C.c_void_p), C.c_uint32(n_rows), C.c_uint32(groups), out.ctypes.data_as(C.c_void_p))
    want = bits.sum(axis=0).astype(np.uint32)
    assert np.array_equal(out, want)
    assert key >> 8 == int(want.max()) and key & 0xFF == int(np.argmax(want))


def _lnfact(oracle, n):
    return np.array([oracle.lib.orc_ln_factorial(i) for i in range(n)], dtype=np.float64)


def _emul_table(emul, lf, t, sizes, fn="emul_prob_table"):
    hist = np.bincount(sizes, minlength=t + 1).astype(np.uint32)
    tz = np.zeros(t + 1)
    z, gs = C.c_double(), C.c_double()
    stats = np.zeros(4, dtype=np.uint64)
    f = getattr(emul, fn)
    f.restype = C.c_int
    rc = f(C.c_uint32(t), hist.ctypes.data_as(C.c_void_p), C.c_uint64(len(sizes)),
                              lf.ctypes.data_as(C.c_void_p), tz.ctypes.data_as(C.c_void_p), C.byref(z), C.byref(gs),
                              stats.ctypes.data_as(C.c_void_p))
    _emul_table.last_stats = stats
    return rc, tz, z.value, gs.value


def test_prob_recurrence_matches_reference_p2(emul, oracle, kats):
    k = kats["P2_hit_prob"]
    t = k["t"]
    sizes = np.arange(0, t + 1, dtype=np.uint16)
    lf = _lnfact(oracle, 2 * t + 8)
    rc, tz, z, gs = _emul_table(emul, lf, t, sizes)
    assert rc == 0
    ref = oracle.highest_hit_prob_per_reference(t, t // 2, sizes)   # any count == t -> only_last branch
    assert np.max(np.abs(tz[sizes] - ref)) < 1e-12
    # general branch: drop the full-overlap reference
    sizes2 = np.arange(0, t, dtype=np.uint16)
    rc, tz, z, gs = _emul_table(emul, lf, t, sizes2)
    ref = oracle.highest_hit_prob_per_reference(t, t // 2, sizes2)
    assert rc == 0 and z >= 1.0
    assert np.max(np.abs(tz[sizes2] - ref)) < 1e-12
    assert abs(ref.sum() - 1.0) < 1e-9


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_prob_recurrence_on_realistic_counts(emul, oracle, seed):
    db = synth.make_db(1200, fanouts=(2, 2, 3, 3, 3, 2))
    ot = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 6, seed=10 + seed, exact_frac=0.3)
    lf = _lnfact(oracle, 2048)
    for i in range(qs.n):
        for skip in (False, True):
            t, counts = ot.hit_counts(qs.seq(i), skip_exact=skip)
            rc, tz, z, gs = _emul_table(emul, lf, t, counts)
            ref = oracle.highest_hit_prob_per_reference(t, t // 2, counts)
            assert rc == 0
            assert np.max(np.abs(tz[counts] - ref)) < 1e-11, (i, skip)
            gs_ref = np.sqrt(((ref - 1.0 / len(ref)) ** 2).sum())
            assert abs(gs - gs_ref) < 1e-11


def test_prob_recurrence_long_sequences_need_scaling(emul, oracle):
    # t = 3000: ln pmf_m(0) is far below ln(DBL_MIN); exercises the 2^-512 rescaling path
    t = 3000
    rng = np.random.default_rng(5)
    sizes = np.concatenate([rng.integers(200, 700, 400), rng.integers(2500, 2950, 5), [0, 1, 2990]]).astype(np.uint16)
    lf = _lnfact(oracle, 2 * t + 8)
    rc, tz, z, gs = _emul_table(emul, lf, t, sizes)
    ref = oracle.highest_hit_prob_per_reference(t, t // 2, sizes)
    assert rc == 0
    assert np.max(np.abs(tz[sizes] - ref)) < 1e-11


def test_prob_status_cases(emul, oracle):
    lf = _lnfact(oracle, 64)
    assert _emul_table(emul, lf, 0, np.zeros(4, np.uint16))[0] == 1          # t == 0
    assert _emul_table(emul, lf, 1, np.zeros(4, np.uint16))[0] == 1          # t == 1, no full overlap
    rc, tz, z, gs = _emul_table(emul, lf, 1, np.array([0, 1, 1, 0], np.uint16))  # t == 1 with full overlap
    assert rc == 0 and z == 2.0 and tz[1] == 0.5 and tz[0] == 0.0


@pytest.mark.parametrize("seed", [0, 1])
def test_prob_lookup_tables_match_reference(emul, oracle, seed):
    """The memoised-table formulation (rtx_prob_tables.hip) against the reference's log-space table."""
    db = synth.make_db(1200, fanouts=(2, 2, 3, 3, 3, 2))
    ot = oracle.tree_new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 6, seed=20 + seed, exact_frac=0.3)
    lf = _lnfact(oracle, 2048)
    for i in range(qs.n):
        for skip in (False, True):
            t, counts = ot.hit_counts(qs.seq(i), skip_exact=skip)
            rc, tz, z, gs = _emul_table(emul, lf, t, counts, fn="emul_prob_lookup")
            ref = oracle.highest_hit_prob_per_reference(t, t // 2, counts)
            assert rc == 0
            assert np.max(np.abs(tz[counts] - ref)) < 1e-11, (i, skip)
    # P2 of the reference's tests, general branch
    t = 400
    sizes = np.arange(0, t, dtype=np.uint16)
    rc, tz, z, gs = _emul_table(emul, _lnfact(oracle, 2 * t + 8), t, sizes, fn="emul_prob_lookup")
    ref = oracle.highest_hit_prob_per_reference(t, t // 2, sizes)
    assert rc == 0 and np.max(np.abs(tz[sizes] - ref)) < 1e-12
    # degenerate inputs
    assert _emul_table(emul, lf, 0, np.zeros(4, np.uint16), fn="emul_prob_lookup")[0] == 1
    rc, tz, z, gs = _emul_table(emul, lf, 9, np.zeros(7, np.uint16), fn="emul_prob_lookup")   # no hits at all
    assert rc == 0 and abs(tz[0] - 1.0 / 7) < 1e-15


@pytest.mark.parametrize("n_refs", [1, 100, 8192, 8193, 50000, 3 * 8192])
def test_bitmap_bit_layout_is_a_bijection(emul, n_refs):
    """ref_slot (where a reference sits in its row) is a bijection onto the bits hit_count's lanes own, and the
    reference of (tile, lane, group, j) -- the order of a lane's count stores -- is its inverse."""
    stride = ((n_refs + 7) // 8 + 127) // 128 * 128
    seen = set()
    w, b = C.c_uint32(), C.c_uint32()
    emul.emul_slot_ref.restype = C.c_uint32
    for r in list(range(min(n_refs, 3000))) + list(range(max(0, n_refs - 3000), n_refs)):
        emul.emul_ref_slot(r, stride, C.byref(w), C.byref(b))
        assert w.value * 4 < stride and b.value < 32
        pos = (w.value, b.value)
        assert pos not in seen or r < 3000 and r >= n_refs - 3000
        seen.add(pos)
        tile, in_tile = divmod(w.value, 256)
        lane, word = divmod(in_tile, 4)
        g, j = word * 4 + b.value // 8, b.value % 8
        assert emul.emul_slot_ref(tile, lane, g, j, stride) == r


def test_epilogue_byte_merge_and_transpose(emul):
    rng = np.random.default_rng(9)
    for _ in range(50):
        sb = rng.integers(0, 256, 8).astype(np.uint8)
        cnt = rng.integers(0, 60000, 8).astype(np.uint16)
        st = cnt.view(np.uint32).copy()
        emul.emul_merge_bytes(sb.view(np.uint32).ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
        assert np.array_equal(st.view(np.uint16), cnt + sb)
    # the saturated cases: a byte counter of 255 on a count with low byte 0 and high bits 3 (0x300 -> 0x3FF: nothing may reach the
    # neighbour), a count of 0xFF that gets nothing beside neighbours that do, all eight at once
    for sb, cnt in (([255, 0, 255, 1, 0, 255, 255, 255], [0x300, 0xFF, 0x300, 0xFE, 0xFF, 0x300, 0, 0x300]),
                    ([0, 255, 0, 255, 0, 255, 0, 255], [0xFF, 0x300, 0x3FF, 0x300, 0xFF, 0x2FF, 0xFFFF, 0]),
                    ([255] * 8, [0x300] * 8), ([0] * 8, [0xFF] * 8), ([255] * 8, [0] * 8)):
        sb, cnt = np.array(sb, np.uint8), np.array(cnt, np.uint16)
        st = cnt.view(np.uint32).copy()
        emul.emul_merge_bytes(sb.view(np.uint32).ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p))
        assert np.array_equal(st.view(np.uint16).astype(np.uint32), cnt.astype(np.uint32) + sb), (sb.tolist(), cnt.tolist())
    # the byte form of the eight-plane epilogue (lo8 = lo + sb, word-wide): all eight references of a group at dense + sparse = 255
    # exactly, in every split -- no carry leaves a byte
    splits = [255, 0, 128, 127, 1, 254, 255, 0]                      # sparse part of references 8 .. 15; the dense part is the rest
    bits = np.zeros((510, 32), bool)                                  # rows 0 .. 254 sparse, 255 .. 509 dense
    for j, sp in enumerate(splits):
        bits[:sp, 8 + j] = True
        bits[255:255 + 255 - sp, 8 + j] = True
    bits[:255:2, 3] = True
    rows = np.ascontiguousarray((bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
    got = _tile_word_counts(emul, rows, np.arange(510) < 255, 8)
    assert (got[8:16] == 255).all() and np.array_equal(got, bits.sum(axis=0).astype(np.uint32))
    m = rng.integers(0, 2, (64, 64)).astype(np.uint64)
    rows = (m << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
    cols = np.zeros(64, np.uint64)
    emul.emul_transpose64(rows.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p))
    want = (m.T << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
    assert np.array_equal(cols, want)


def test_row_finalisation_matches_the_oracle(emul, oracle):
    """finalise_kernel's arithmetic (rtx_math.hpp: fin_row_before, fin_local_signal) on the CPU: the rows the oracle returns for real
    barcodes (lineage.rs:91-110: sorted, with their local signal), shuffled, must come back in the oracle's order with the oracle's local
    signals; rows handed over in the oracle's order must keep it (the sort of lineage.rs:91-93 is stable)."""
    from pathlib import Path

    text = (Path(__file__).resolve().parent / "golden" / "diptera_subset.fasta").read_text()
    otree = oracle.parse_reference_fasta_str(text)
    queries = oracle.parse_query_fasta_str(text)
    N = otree.num_tips
    rng = np.random.default_rng(5)
    emul.emul_finalise_rows.restype = C.c_uint32
    multi = 0
    for label, seq in queries[:150]:
        rows, _ = otree.classify(seq, skip_exact=True, raw_confidence=True)
        n = len(rows)
        D = max(len(r["conf"]) for r in rows)
        k = np.zeros((n, D), np.uint8)
        size = np.zeros((n, D), np.uint32)
        depth = np.zeros(n, np.uint32)
        for i, r in enumerate(rows):
            depth[i] = len(r["conf"])
            k[i, :depth[i]] = np.rint(np.array(r["conf"]) * 100).astype(np.uint8)
            size[i, :depth[i]] = np.rint(np.array(r["expd"]) * N).astype(np.uint32)
        for order in (np.arange(n), rng.permutation(n)):
            ks, ss, ds = np.ascontiguousarray(k[order]), np.ascontiguousarray(size[order]), np.ascontiguousarray(depth[order])
            rank = np.zeros(n, np.uint32)
            local = np.zeros(n, np.float64)
            bad = emul.emul_finalise_rows(C.c_uint32(n), C.c_uint32(D), ks.ctypes.data_as(C.c_void_p), ds.ctypes.data_as(C.c_void_p),
                                          ss.ctypes.data_as(C.c_void_p), C.c_double(N), rank.ctypes.data_as(C.c_void_p), local.ctypes.data_as(C.c_void_p))
            assert bad == 0                                           # the kernel's word-wise compare = the byte-wise statement of lineage.rs:91-93
            assert sorted(rank.tolist()) == list(range(n))            # a permutation: no two rows share a place
            back = np.empty(n, np.int64)
            back[rank] = np.arange(n)
            assert np.array_equal(ks[back], k) and np.array_equal(ds[back], depth)      # the oracle's order of confidence vectors
            want = np.array([r["local_signal"] for r in rows])
            if np.array_equal(order, np.arange(n)):
                assert np.array_equal(rank, np.arange(n))             # stable: equal vectors keep the order of the walk
                assert np.allclose(local, want, rtol=0, atol=1e-12)
            else:   # (rows with equal confidence vectors may have changed places among themselves: compare them as a set)
                key = lambda kk, dd, ll: sorted((tuple(a), int(b), round(float(c), 11)) for a, b, c in zip(kk.tolist(), dd, ll))
                assert key(ks, ds, local) == key(k, depth, want)
        multi += n > 1
    assert multi > 20

"""The chimera check without a device: rtx_chimera_read (host_chimera.cpp) and the arithmetic the kernels run (rtx_math.hpp through the x86
emulator: boundaries, the padded row lists, a checkpoint's step from candidate mask to lowest reference, the reduction over tiles) against
the numpy restatement of the definition (tests/chimera_common.py)."""
import ctypes as C

import numpy as np
import pytest

import chimera_common as cc
import raxtax_amd as rx
from raxtax_amd import synth

SEGMENTS = (2, 16, 32)


@pytest.fixture(scope="module")
def world():
    """300 references of 200 bases: a synthetic taxonomy with a few references rewritten for the designed reads."""
    db = synth.make_db(300, length=200)
    rng = np.random.default_rng(11)
    refs = db.seq_bytes.reshape(300, 200).copy()
    acgt = np.array([1, 2, 4, 8], np.uint8)
    refs[17] = refs[5]                                   # two identical references: the lower id wins
    tie_read = acgt[rng.integers(0, 4, 200)]             # a read whose head is reference 10's and whose tail is reference 11's, nothing between
    refs[10] = acgt[rng.integers(0, 4, 200)]
    refs[11] = acgt[rng.integers(0, 4, 200)]
    refs[10][:80] = tie_read[:80]
    refs[11][120:] = tie_read[120:]
    refs[20][30:60] = 1                                  # a homopolymer run in a reference ...
    homo = refs[20].copy()
    homo[100:140] = 1                                    # ... and a longer one in a read: the repeated 8-mer counts once per position
    bases = refs.reshape(-1)
    off = (np.arange(301) * 200).astype(np.uint64)
    reads = {}
    b8 = 8 * 193 // 16
    for name, bp in (("chimera_on_boundary", b8), ("chimera_off_boundary", b8 + 5), ("chimera_late", 171)):
        reads[name] = cc.substitute(rng, np.concatenate([refs[40][:bp], refs[250][bp:]]), 0.01)
    reads["plain"] = cc.substitute(rng, refs[123], 0.02)
    reads["copy_of_identical"] = refs[17].copy()
    reads["tie"] = tie_read
    reads["homopolymer"] = homo
    with_n = refs[77].copy()
    with_n[50:60] = 15
    with_n[120] = 15
    reads["n_runs"] = with_n
    reads["all_n"] = np.full(64, 15, np.uint8)
    long = np.concatenate([refs[i] for i in range(30, 51)])
    for n in (0, 7, 8, 8 + 16 - 2, 8 + 32 - 2, 23, 4096, 4097):
        reads[f"len{n}"] = long[:n].copy()
    return dict(bases=bases, off=off, reads=reads, rs=cc.Restatement(bases, off))


@pytest.mark.parametrize("S", SEGMENTS)
def test_host_mirror_equals_the_restatement(world, S):
    for name, read in world["reads"].items():
        got = rx.chimera_read(rx.ChimeraParams(S, 24), read, world["bases"], world["off"])
        want = world["rs"].record(read, S, 24)
        assert cc.as_tuple(got) == cc.as_tuple(want), (name, S, dict(zip(cc.FIELDS, cc.as_tuple(got))), want)


def test_designed_reads_are_what_they_were_designed_as(world):
    rec = lambda name, S=16: world["rs"].record(world["reads"][name], S, 24)  # noqa: E731
    for name in ("chimera_on_boundary", "chimera_off_boundary"):
        r = rec(name)
        assert r["flag"] == 1 and r["seg"] in (7, 8) and r["parent_a"] != r["parent_b"], (name, r)   # (the windows across the junction match neither parent)
    assert rec("plain")["flag"] == 0
    r = rec("copy_of_identical")
    assert r["parent"] == 5 and r["single"] == 193 and r["delta"] == 0
    r = rec("tie")      # two[s] is the same for every boundary between the two matching parts: the lowest one
    assert (r["seg"], r["parent_a"], r["parent_b"], r["left"], r["right"]) == (7, 10, 11, 73, 73), r
    r = rec("homopolymer")   # the 33 windows inside the run all count, though they are one 8-mer; the 14 across its two edges need not match
    assert r["parent"] == 20 and 193 - 14 <= r["single"] <= 193 and len(np.unique(cc.window_codes(world["reads"]["homopolymer"])[0])) < 193 - 14
    assert rec("all_n")["status"] == cc.NO_KMER and rec("len7")["status"] == cc.NO_KMER and rec("len0")["status"] == cc.NO_KMER
    assert rec("len8")["n_valid"] == 1 and rec("len4096")["status"] == cc.OK and rec("len4096")["n_valid"] == 4089
    assert rec("len4097")["status"] == cc.TOO_LONG and rec("len4097")["flag"] == 0
    assert rec("n_runs")["n_valid"] == 193 - 17 - 8


def test_params_are_checked(world):
    for S in (0, 1, 33):
        with pytest.raises(rx.RtxError) as e:
            rx.chimera_read(rx.ChimeraParams(S, 24), world["reads"]["plain"], world["bases"], world["off"])
        assert e.value.code == -1


def _layout(emul, n_pos, S):
    b, o0, o1 = (np.zeros(S + 1, np.uint32) for _ in range(3))
    p32 = C.POINTER(C.c_uint32)
    emul.emul_chimera_layout.restype = C.c_uint32
    cap = emul.emul_chimera_layout(n_pos, S, b.ctypes.data_as(p32), o0.ctypes.data_as(p32), o1.ctypes.data_as(p32))
    return cap, b.astype(np.int64), o0.astype(np.int64), o1.astype(np.int64)


@pytest.mark.parametrize("S", SEGMENTS)
def test_emul_boundaries_and_padded_lists(emul, S):
    p32 = C.POINTER(C.c_uint32)
    for n_pos in list(range(41)) + [1023, 1024, 4089]:
        cap, b, o0, o1 = _layout(emul, n_pos, S)
        want_b = np.array([s * n_pos // S for s in range(S + 1)])
        assert np.array_equal(b, want_b), (n_pos, S)
        sizes = np.diff(want_b)
        padded = (sizes + 7) // 8 * 8
        assert np.array_equal(o0, np.concatenate([[0], np.cumsum(padded)])), (n_pos, S)
        assert np.array_equal(o1, np.concatenate([[0], np.cumsum(padded[::-1])])), (n_pos, S)
        rows = int(padded.sum())
        assert cap == (rows + 63) // 64 * 64 + 192 and cap >= rows + 144     # the scan's look-ahead stays inside the zero rows
        for d, order in ((0, range(S)), (1, range(S - 1, -1, -1))):
            lst = np.zeros(cap, np.uint32)
            emul.emul_chimera_list(n_pos, S, d, cap, lst.ctypes.data_as(p32))
            want = []
            for s in order:   # every segment: its windows in position order, then the zero row up to a multiple of eight
                want += list(range(want_b[s], want_b[s + 1])) + [cc.NO_REF] * int(padded[s] - sizes[s])
            want += [cc.NO_REF] * (cap - len(want))
            assert np.array_equal(lst, np.array(want, np.uint32)), (n_pos, S, d)
    emul.emul_chimera_n_pos.restype = C.c_uint32
    assert [emul.emul_chimera_n_pos(n) for n in (0, 7, 8, 9, 4096, 4097)] == [0, 0, 1, 2, 4089, 0]


@pytest.mark.parametrize("planes", (10, 12))
def test_emul_checkpoint_candidate_to_lowest_reference(emul, planes):
    """A checkpoint on one tile: the largest counter and the LOWEST reference that holds it, in a full tile, in the partial last tile of a
    database (the counters behind its references are zero) and in a tile whose row spans fewer than 64 lanes (ref_slot's general form)."""
    rng = np.random.default_rng(planes)
    top = (1 << planes) - 1
    p16, p32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)

    def run(counts, stride_bytes, tile):
        m, r = C.c_uint32(), C.c_uint32()
        assert emul.emul_chimera_checkpoint(counts.ctypes.data_as(p16), planes, stride_bytes, tile, C.byref(m), C.byref(r)) == 0
        return m.value, r.value

    for tile, in_tile, stride in ((0, 8192, 5 * 1024), (4, 37, 5 * 1024), (4, 8192, 5 * 1024), (2, 5 * 128, 2 * 1024 + 5 * 16)):
        for case in range(24):
            counts = np.zeros(8192, np.uint16)
            counts[:in_tile] = rng.integers(0, top + 1 if case % 3 else 40, in_tile)
            if case % 4 == 1:       # the maximum several times over, also at the saturated value
                counts[rng.integers(0, in_tile, 5)] = top
            if case == 23:
                counts[:] = 0
            m, r = run(counts, stride, tile)
            assert m == int(counts.max()), (tile, in_tile, case)
            assert r == (tile * 8192 + int(np.argmax(counts)) if m else cc.NO_REF), (tile, in_tile, case, m)
        for where in (0, 7, 8, 511, 512, 4095, 4096, in_tile - 1):   # one reference alone, at the edges of bytes, groups and words
            if where < in_tile:
                counts = np.zeros(8192, np.uint16)
                counts[where] = 3
                assert run(counts, stride, tile) == (3, tile * 8192 + where)
    assert emul.emul_chimera_checkpoint(None, 9, 1024, 0, None, None) == -1


def test_emul_reduce_takes_the_lowest_reference_over_tiles(emul):
    """chimera_reduce_kernel's arithmetic: the tiles in ascending order, a later tile only with a larger count; then the record."""
    rng = np.random.default_rng(3)
    p32 = C.POINTER(C.c_uint32)
    for S in SEGMENTS:
        for ntiles in (1, 5):
            for case in range(20):
                n_pos = 193
                b = [s * n_pos // S for s in range(S + 1)]
                best = np.zeros((2, S, ntiles, 2), np.uint32)
                best[..., 0] = rng.integers(0, 4 if case % 2 else 60, (2, S, ntiles))
                best[0, S - 1, :, 0] = rng.integers(0, 2, ntiles)   # `single` small and P[1] at least 2: two[s] >= single as in every real read
                best[0, 0, 0, 0] = max(int(best[0, 0, 0, 0]), 2) if S > 2 else best[0, 0, 0, 0]
                best[1, S - 2, 0, 0] = max(int(best[1, S - 2, 0, 0]), 2)
                best[1, S - 1, :, 0] = best[0, S - 1, :, 0]          # Suf[0] and P[S] are both `single`
                ref = np.arange(ntiles)[None, None, :] * 8192 + rng.integers(0, 8192, (2, S, ntiles))
                ref[1, S - 1] = ref[0, S - 1]
                best[..., 1] = np.where(best[..., 0] == 0, cc.NO_REF, ref)
                pm = [0] + [int(best[0, k, :, 0].max()) for k in range(S)]
                pr = [cc.NO_REF] + [int(best[0, k, int(np.argmax(best[0, k, :, 0])), 1]) for k in range(S)]
                sm = [int(best[1, S - 1 - s, :, 0].max()) for s in range(S)] + [0]
                sr = [int(best[1, S - 1 - s, int(np.argmax(best[1, S - 1 - s, :, 0])), 1]) for s in range(S)] + [cc.NO_REF]
                two = [pm[s] + sm[s] for s in range(1, S)]
                seg = 1 + int(np.argmax(two))
                want = (cc.OK, 100, pm[S], pr[S] if pm[S] else cc.NO_REF, seg, b[seg], pm[seg], pr[seg] if pm[seg] else cc.NO_REF, sm[seg],
                        sr[seg] if sm[seg] else cc.NO_REF, max(two) - pm[S], int(max(two) - pm[S] >= 3))
                rec = np.zeros(12, np.uint32)
                emul.emul_chimera_reduce(200, 100, S, 3, ntiles, best.ctypes.data_as(p32), rec.ctypes.data_as(p32))
                assert tuple(int(x) for x in rec) == want, (S, ntiles, case)
    for length, nv, status in ((200, 0, cc.NO_KMER), (4097, 0, cc.TOO_LONG), (4097, 5, cc.TOO_LONG)):
        rec = np.zeros(12, np.uint32)
        emul.emul_chimera_reduce(length, nv, 16, 24, 1, np.ones((2, 16, 1, 2), np.uint32).ctypes.data_as(p32), rec.ctypes.data_as(p32))
        assert tuple(int(x) for x in rec) == (status, 0, 0, cc.NO_REF, 0, 0, 0, cc.NO_REF, 0, cc.NO_REF, 0, 0)

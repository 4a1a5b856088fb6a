"""The chimera check on the device (rtx_chimera.hip) against the numpy restatement of its definition (tests/chimera_common.py), field by
field and for equality:

  1. designed chimeras on the de Bruijn family (four tiles + 37 references): head of one planted window + tail of another, the two in
     different tiles, in one tile, one in the partial last tile, the junction on a boundary and inside a segment; reads that are one planted
     window, whose `single` and `parent` are also the classifier's peak and nearest reference (no 8-mer repeats in a de Bruijn window);
  2. edges: the plane classes (n_pos 1023 / 1024), the longest read (4096 bases) and the first that is too long, reads of 0 .. 8 bases,
     batches of 0, 1 and 65 reads, one read in two batches;
  3. a random database of 2 000 references with 300 planted chimeras and 300 plain reads: every field, and the two conditions of the
     definition's sanity check (at least 95 % of the chimeras flagged, no plain read);
  4. through rx.raxtax with and without dereplication: unflagged queries byte for byte as without the option, flagged ones as the empty read,
     the callback's records those of Chimera.run, a copy with its representative's record, raxtax_last_chimera adding up;
  5. the refusals: a strand-both handle, a reference shard, parameters out of range;
  6. slices: the reads of 3. with reads of 1 031, 4 096 and 4 097 bases, cut by RTX_DEFAULT_CHIMERA_SLICE into slices of 1, 7, 64, n - 1 and
     n reads -- slices without a ten-plane read, without a twelve-plane read, and of too-long reads alone -- byte for byte the uncapped run."""
import numpy as np
import pytest

import chimera_common as cc
import debruijn_common as dc
import raxtax_amd as rx
from raxtax_amd import _lib, synth
from raxtax_amd.sharded import ShardIndex

pytestmark = pytest.mark.gpu


def _check(stage, rs, seqs, S=16, mindelta=24, what=""):
    bases, off = cc.concat(seqs)
    got = stage.run(bases, off)
    assert len(got) == len(seqs)
    for i, s in enumerate(seqs):
        want = rs.record(s, S, mindelta)
        assert cc.as_tuple(got[i]) == cc.as_tuple(want), (what, i, len(s), dict(zip(cc.FIELDS, cc.as_tuple(got[i]))), want)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the de Bruijn family
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fam():
    f = dc.family()
    bases, off = f.flat()
    tree = rx.Tree.new_flat(f.lineages, bases, off)
    index = rx.Index(tree, nearest=True)
    return dict(fam=f, index=index, rs=cc.Restatement(bases, off), stage=rx.Chimera(index), stages={})


def _stage(fam, S):
    if S not in fam["stages"]:
        fam["stages"][S] = rx.Chimera(fam["index"], rx.ChimeraParams(S, 24))
    return fam["stages"][S]


# (start, k-mers) of the head window and of the tail window; the planted references that hold them: tile 0 (97: 1000 .. 1254; 320 ..: 5000 ..),
# tile 1 (200 ..: 2000 ..), tile 2 (240 ..: 3000 ..), the partial last tile (5: 4000 .. 4254)
_JOINS = {
    "different_tiles_on_boundary": ((1000, 128), (2000, 121)),      # n_pos = 256: b_8 = 128, the head's last window is 127
    "different_tiles_inside": ((1000, 133), (2000, 116)),
    "same_tile": ((1000, 128), (5000, 121)),
    "same_tile_inside": ((1003, 77), (5100, 172)),
    "last_tile_head": ((4000, 128), (3000, 121)),
    "last_tile_tail": ((2010, 150), (4020, 99)),
    "three_planes_classes_long": ((5000, 700), (12000, 900)),       # n_pos = 1607: twelve planes
    "short": ((1000, 9), (4000, 9)),
}


def _join(name):
    (a1, t1), (a2, t2) = _JOINS[name]
    return np.concatenate([dc.query(a1, t1), dc.query(a2, t2)])


@pytest.mark.parametrize("S", (2, 16, 32))
def test_designed_chimeras(fam, S):
    seqs = [_join(n) for n in _JOINS]
    got = _check(_stage(fam, S), fam["rs"], seqs, S, what="joins")
    if S == 16:
        f = fam["fam"]
        r = got[list(_JOINS).index("different_tiles_on_boundary")]
        assert (int(r["seg"]), int(r["pos"]), int(r["left"]), int(r["right"])) == (8, 128, 128, 121) and int(r["flag"]) == 1
        assert int(r["parent_a"]) == 97 and int(r["parent_b"]) // dc.TILE == 1
        r = got[list(_JOINS).index("last_tile_head")]
        assert int(r["parent_a"]) == f.n_full * dc.TILE + 5 and int(r["parent_b"]) // dc.TILE == 2
        r = got[list(_JOINS).index("same_tile")]
        assert int(r["parent_a"]) == 97 and int(r["parent_b"]) // dc.TILE == 0 and int(r["flag"]) == 1


_SINGLE = [(1000, 255), (2000, 255), (3000, 255), (4000, 255), (5000, 1023), (9000, 1023), (6999, 1024), (12000, 2048), (1003, 40), (20300, 400)]


def test_single_windows_agree_with_the_classifier(fam):
    """A read that is one window of the de Bruijn sequence repeats no 8-mer: positions and distinct 8-mers count alike, so `single` is the
    classifier's peak and `parent` its nearest reference -- the same bitmap through the other counting path."""
    seqs = [dc.query(a, t) for a, t in _SINGLE]
    got = _check(fam["stage"], fam["rs"], seqs, what="single windows")
    bases, off = cc.concat(seqs)
    res = fam["index"].classify(bases, off)
    for i, (a, t) in enumerate(_SINGLE):
        assert int(got[i]["n_valid"]) == t and int(got[i]["single"]) == int(res.peak[i]) and int(got[i]["parent"]) == int(res.nearest[i]), (a, t)
        assert int(got[i]["single"]) == int(fam["fam"].expected_counts(a, t).max())
        assert int(got[i]["flag"]) == 0 and int(got[i]["delta"]) == 0


def test_edges(fam):
    seq = dc.de_bruijn_4_8()
    edge = [dc.query(5000, 1023), dc.query(6999, 1024), dc.query(12000, 4089), dc.query(12000, 4090)]   # n_pos 1023 | 1024 | 4089 | 4097 bases
    assert [len(s) for s in edge] == [1030, 1031, 4096, 4097]
    tiny = [seq[1000:1000 + n].copy() for n in range(9)]
    with_n = dc.query(1000, 255)
    with_n[100:104] = 15
    got = _check(fam["stage"], fam["rs"], edge + tiny + [with_n, np.full(300, 15, np.uint8)], what="edges")
    assert [int(r["status"]) for r in got[:4]] == [cc.OK, cc.OK, cc.OK, cc.TOO_LONG] and int(got[2]["single"]) == 4089
    assert [int(r["status"]) for r in got[4:13]] == [cc.NO_KMER] * 8 + [cc.OK]
    # batches of 0, 1 and 65 reads; a read's record never depends on the rest of its batch
    assert len(fam["stage"].run(np.zeros(0, np.uint8), np.zeros(1, np.uint64))) == 0
    one = _join("different_tiles_inside")
    alone = _check(fam["stage"], fam["rs"], [one], what="alone")[0]
    batch = [dc.query(1000 + 3 * i, 60 + i) for i in range(64)]
    mixed = _check(fam["stage"], fam["rs"], batch[:40] + [one] + batch[40:], what="65 reads")
    assert cc.as_tuple(mixed[40]) == cc.as_tuple(alone)
    other = fam["stage"].run(*cc.concat([dc.query(12000, 4089), one, tiny[3]]))
    assert cc.as_tuple(other[1]) == cc.as_tuple(alone)
    assert fam["stage"].kernel_ms() > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3, 4: a random database
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rnd():
    db = synth.make_db(2000)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    chim, _ = cc.planted_chimeras(db)            # 300, rng seed 5, breakpoints 100 .. 558, 1 % substitutions
    qs = synth.make_queries(db, 300)             # 300 plain reads, 2 % substitutions
    return dict(db=db, tree=tree, rs=cc.Restatement(*cc.tree_order(db, tree)), chim=chim, plain=[qs.seq(i).copy() for i in range(300)])


def test_random_database(rnd):
    index = rx.Index(rnd["tree"])
    got = _check(rx.Chimera(index), rnd["rs"], rnd["chim"] + rnd["plain"], what="random database")
    flagged = got["flag"].astype(bool)
    print(f"chimeras flagged: {int(flagged[:300].sum())} of 300 (median delta {int(np.median(got['delta'][:300]))}); "
          f"plain reads flagged: {int(flagged[300:].sum())} of 300 (largest delta {int(got['delta'][300:].max())})")
    assert flagged[:300].sum() >= 0.95 * 300
    assert not flagged[300:].any()


@pytest.mark.parametrize("derep", (False, True))
def test_through_raxtax(rnd, derep):
    index = rx.Index(rnd["tree"], derep=derep)
    seqs = rnd["plain"][:20] + rnd["chim"][:12] + [rnd["plain"][3].copy(), rnd["chim"][5].copy(), rnd["chim"][5].copy(), rnd["plain"][7][:300].copy()]
    queries = [(f"q{i}", s) for i, s in enumerate(seqs)]
    want = rx.Chimera(index).run(*cc.concat(seqs))
    flagged = {f"q{i}" for i in range(len(seqs)) if want[i]["flag"]}
    assert 10 <= len(flagged) <= 14 and "q33" in flagged and "q34" in flagged and "q32" not in flagged

    def run(**kw):
        sent = []
        rx.raxtax(queries, index, False, False, 16, lambda label, out, tsv: sent.append((label, out, tsv)), True, **kw)
        return sent

    base = run()
    assert [m[0] for m in base] == [q[0] for q in queries]
    assert rx.raxtax_last_chimera()[:3] == (0, 0, 0)
    index.set_chimera(rx.ChimeraParams())
    assert index.chimera == rx.ChimeraParams(16, 24)
    recs = []
    sent = run(chimera=lambda label, rec: recs.append((label, cc.as_tuple(rec))))
    # unflagged: the sender calls of the run without the option, byte for byte; flagged: what the empty read produces -- no message
    assert sent == [m for m in base if m[0] not in flagged]
    assert recs == [(f"q{i}", cc.as_tuple(want[i])) for i in range(len(seqs))]
    assert recs[33][1] == recs[34][1] == recs[25][1] and recs[32][1] == recs[3][1]     # a copy carries its representative's record
    n_distinct = sum(len({s.tobytes() for s in seqs[c:c + 16]}) for c in range(0, len(seqs), 16))   # (per chunk of 16, as the dereplication works)
    assert n_distinct == len(seqs) - 1
    q, checked, fl, busy = rx.raxtax_last_chimera()
    assert (q, checked, fl) == (len(seqs), n_distinct if derep else len(seqs), len(flagged)) and busy > 0.0
    assert run() == sent                                   # without the callback: the same messages
    empty = []
    rx.raxtax([("e", np.zeros(0, np.uint8))], index, False, False, 16, lambda *m: empty.append(m), True)
    assert empty == []                                     # (the empty read: no message)
    index.set_chimera(None)
    assert index.chimera is None and run() == base


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: slices
# ---------------------------------------------------------------------------------------------------------------------------------
def _sliced_reads(rnd):
    """64 reads of 4 097 bases, 64 of 1 031 and 4 096 bases in turn, the 600 reads of the random database, and five of every kind: under a
    cap of 64 slice 0 holds too-long reads alone, slice 1 no ten-plane read, slices 2 .. 10 no twelve-plane read and the last one all
    kinds; under a cap of 7 the same holds of more slices, and some begin in the middle of a kind."""
    db = rnd["db"]
    long = [np.concatenate([db.seq_bytes[int(db.seq_off[r]):int(db.seq_off[r + 1])] for r in range(k, k + 8)]) for k in range(64)]
    assert min(len(s) for s in long) >= 4097
    too_long = [s[:4097] for s in long]
    twelve = [s[k:k + (1031 if k % 2 else 4096)] for k, s in enumerate(long)]
    ten = rnd["chim"] + rnd["plain"]
    assert max(len(s) for s in ten) <= 1030
    return too_long + twelve + ten + [long[3][5:1036], long[4][1:4098], ten[0][:500], long[5][2:4098], ten[1][:31]]


def test_slices(rnd):
    index = rx.Index(rnd["tree"])
    stage = rx.Chimera(index)
    seqs = _sliced_reads(rnd)
    n = len(seqs)
    bases, off = cc.concat(seqs)
    free = _check(stage, rnd["rs"], seqs, what="uncapped")
    status = [int(r["status"]) for r in free]
    assert status[:64] == [cc.TOO_LONG] * 64 and status[64:128] == [cc.OK] * 64 and status[-5:] == [cc.OK, cc.TOO_LONG, cc.OK, cc.OK, cc.OK]
    lib = _lib.load()
    try:
        for cap in (1, 7, 64, n - 1, n):
            _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, cap))
            got = stage.run(bases, off)
            assert got.tobytes() == free.tobytes(), cap
            assert stage.kernel_ms() > 0.0, cap
            if cap == 64:
                whole = stage.kernel_ms()
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, 0))
        # the kernel time of a run is the sum over its slices: no smaller than that of any one slice, run as a call of its own
        parts = []
        for q0 in range(0, n, 64):
            part = stage.run(*cc.concat(seqs[q0:q0 + 64]))
            assert part.tobytes() == free[q0:q0 + 64].tobytes(), q0
            parts.append(stage.kernel_ms())
        print(f"kernel ms of the run in slices of 64: {whole:.3f}; of the slices alone: {' '.join(f'{t:.3f}' for t in parts)}")
        assert all(whole >= t for t in parts) and max(parts) > 0.0
    finally:
        _lib.check(lib.rtx_set_default_option(_lib.RTX_DEFAULT_CHIMERA_SLICE, 0))
    assert stage.run(bases, off).tobytes() == free.tobytes()           # (the cap is gone)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rnd):
    with pytest.raises(rx.RtxError) as e:
        rx.Chimera(rx.Index(rnd["tree"], strand="both"))
    assert e.value.code == -1 and "RTX_OPT_STRAND" in str(e.value)
    shard = ShardIndex(rnd["tree"], 0, [0, 1000, 2000])
    with pytest.raises(rx.RtxError) as e:
        rx.Chimera(shard)
    assert e.value.code == -1 and "shard" in str(e.value)
    index = rx.Index(rnd["tree"])
    for S in (1, 33):
        with pytest.raises(rx.RtxError) as e:
            rx.Chimera(index, rx.ChimeraParams(S, 24))
        assert e.value.code == -1
        with pytest.raises(rx.RtxError):
            index.set_chimera(rx.ChimeraParams(S, 24))
    both = rx.Index(rnd["tree"], strand="both", chimera=rx.ChimeraParams())
    with pytest.raises(rx.RtxError) as e:
        rx.raxtax([("a", rnd["plain"][0])], both, False, False, 16, lambda *m: None, False)
    assert e.value.code == -1

"""The consensus taxonomy of the OTUs on the host: rtx_otu_taxonomy_host against the brute force of otutax_common.py on every crafted case and
on the random world, exactly; the refusals; the formatter; rtx_result_best_lineages on a hand-made view (the single-exact-match override and
both flags)."""
import ctypes as C

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from otutax_common import (CLASSIFIED, MAX_DEPTH, PERMUTED, UNCLASSIFIABLE, UNCLASSIFIED, Case, assert_tax, brute, cases, check_expected, permutation, random_world,
                           refusals, world)


@pytest.mark.parametrize("name", sorted(cases()))
def test_host_against_the_brute_force(name):
    case, agree, expected = cases()[name]
    otus, lin = case.arrays()
    want = brute(case.w.parent, otus, lin, agree)
    check_expected(name, want, expected)           # the case shows what it was built to show, by the brute force alone
    got = rx.otu_taxonomy_host(case.w.tree, otus, lin, agree=agree)
    assert_tax(got, want, name)
    assert got.agree_pct == agree and got.packed_waves == 0 and got.big_otus == 0 and got.seconds == (0, 0, 0, 0)
    if name in PERMUTED:                           # the ranks permuted: the same OTUs, the same result
        otus2, lin2 = case.arrays(permutation(len(otus[0])))
        assert_tax(rx.otu_taxonomy_host(case.w.parent, otus2, lin2, agree=agree), got, name + " permuted")


def test_random_world_on_the_host():
    case = random_world()
    otus, lin = case.arrays()
    assert 4000 <= len(otus[0]) <= 7000 and len(otus[2]) == 700 and 150 <= case.w.n_nodes <= 260
    want = brute(case.w.parent, otus, lin)
    assert (want["members"] > 256).sum() >= 3 and len(set(want["depth"].tolist())) >= 4 and len(set(want["seed_rel"].tolist())) == 4
    assert_tax(rx.otu_taxonomy_host(case.w.tree, otus, lin), want, "random")
    assert_tax(rx.otu_taxonomy_host(case.w.tree, otus, lin, agree=75), brute(case.w.parent, otus, lin, 75), "random at 75")


@pytest.mark.parametrize("name", sorted(refusals()))
def test_host_refuses(name):
    otus, lin, agree, parent = refusals()[name]
    with pytest.raises(rx.RtxError) as e:
        rx.otu_taxonomy_host(world().tree if parent is None else parent, tuple(otus), lin, agree=agree)
    assert e.value.code == _lib.RTX_ERR_INVALID and "rtx_otu_taxonomy_host" in str(e.value)


def test_the_largest_weights_that_fit_are_taken():
    c = Case().add(0, (1 << 64) // 100 - 1, "A,B,C").add(0, 1, "A,E,F")
    otus, lin = c.arrays()
    assert_tax(rx.otu_taxonomy_host(c.w.tree, otus, lin), brute(c.w.parent, otus, lin), "largest")


def test_text():
    c = Case()
    c.add(0, 2, "A,E,G,H", hund=[100, 95, 90, 81]).add(0, 2, "A,E,G,I", hund=[99, 90, 80, 80]).add(0, 1, "A,B,C", hund=[85, 80, 80])
    c.add(1, 1, "J,K,L").add(1, 1, "Q,R,S")
    c.add(2, 7, None, kind=UNCLASSIFIABLE)
    c.add(3, 2, "X,Y", seed=True, hund=[100, 100]).add(3, 9, "X,Y,Z", hund=[100, 100, 100])
    otus, lin = c.arrays()
    tax = rx.otu_taxonomy_host(c.w.tree, otus, lin)
    head = "#otu\tsize\tmembers\tclassified\tdepth\ttaxon\tlineage\tsupport\tmean_conf\tseed\n"
    lines = ["otu1\t5\t3\t5\t3\tG\tA,E,G\t100.00,80.00,80.00\t0.97,0.93,0.85\t<\n",     # conf: (200+198+85+2)/5 = 97, (190+180+2)/4 = 93, (180+160+2)/4 = 85; H holds 2 of 5
             "otu2\t2\t2\t2\t0\t-\t-\t-\t-\t<\n",     # the empty consensus is a proper prefix of the seed's path
             "otu3\t7\t1\t0\t0\t-\t-\t-\t-\t=\n",
             "otu4\t11\t2\t11\t3\tZ\tX,Y,Z\t100.00,100.00,81.82\t1.00,1.00,1.00\t>\n"]
    assert tax.text(c.w.tree) == head + "".join(lines)
    assert tax.text(c.w.tree, minsize=6) == head + lines[2] + lines[3]
    assert tax.text(c.w.tree, minsize=100) == head
    # the buffer protocol: one byte short answers -(need) - RTX_NEED_BASE
    lib = _lib.load()
    need = lib.rtx_otu_taxonomy_format(tax._h, c.w.tree._h, 0, None, 0)
    buf = C.create_string_buffer(need)
    assert need == len(head + "".join(lines)) and lib.rtx_otu_taxonomy_format(tax._h, c.w.tree._h, 0, buf, need - 1) == -need - 1024
    other = rx.Tree.new(["a,b"], [np.array([1, 2, 4, 8, 1, 2, 4, 8, 1], np.uint8)])
    with pytest.raises(rx.RtxError):
        tax.text(other)


def hand_made_view(w):
    """Five queries over the world's tree, rows in processing order (not query order), no byte arrays: q0 two rows, the first A,E,G,H at
    0.95 0.90 0.79 0.60; q1 unclassifiable by status; q2 one row J,K,L at 0.50 ...: unclassified at 0.8; q3 no rows; q4 one row Q,R,T,U, all 1.0"""
    lineage_of = {name: i for i, name in enumerate(w.lineages)}
    rows = [("Q,R,T,U", [1.0, 1.0, 1.0, 1.0]), ("A,E,G,H", [0.95, 0.90, 0.79, 0.60]), ("A,E,G,I", [0.95, 0.90, 0.21, 0.20]), ("J,K,L", [0.50, 0.40, 0.30])]
    keep = dict(t=np.array([30, 0, 30, 30, 30], np.uint32), status=np.array([0, 1, 0, 0, 0], np.uint8), gs=np.ones(5), begin=np.array([1, 0, 3, 0, 0], np.uint64),
                count=np.array([2, 0, 1, 0, 1], np.uint32), lin=np.array([lineage_of[n] for n, _ in rows], np.uint32), node=np.array([w.node(n) for n, _ in rows], np.uint32),
                depth=np.array([len(c) for _, c in rows], np.uint32), conf=np.zeros((4, MAX_DEPTH)), local=np.ones(4))
    for i, (_, c) in enumerate(rows):
        keep["conf"][i, :len(c)] = c
    p = _lib.ptr
    view = _lib.ResultView(5, 4, p(keep["t"], _lib.u32p), p(keep["status"], _lib.u8p), p(keep["gs"], _lib.f64p), p(keep["begin"], _lib.u64p), p(keep["count"], _lib.u32p),
                           p(keep["lin"], _lib.u32p), p(keep["node"], _lib.u32p), p(keep["depth"], _lib.u32p), p(keep["conf"], _lib.f64p), p(keep["local"], _lib.f64p), 0, None, None)
    return view, keep, lineage_of


def best(w, view, cutoff, flags, exact):
    n = 5
    kind, L, node, hund = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.full((n, MAX_DEPTH), 7, np.uint8)
    ids, off = exact if exact else (None, None)
    rc = _lib.load().rtx_result_best_lineages(w.tree._h, C.byref(view), None if ids is None else _lib.ptr(ids, _lib.u32p), None if off is None else _lib.ptr(off, _lib.u64p),
                                              cutoff, flags, _lib.ptr(kind, _lib.u8p), _lib.ptr(L, _lib.u8p), _lib.ptr(node, _lib.u32p), _lib.ptr(hund, _lib.u8p), MAX_DEPTH)
    return rc, kind, L, node, hund


def test_best_lineages_on_a_hand_made_view():
    w = world()
    view, keep, lineage_of = hand_made_view(w)
    rc, kind, L, node, hund = best(w, view, 80, 0, None)
    assert rc == 0
    assert kind.tolist() == [CLASSIFIED, UNCLASSIFIABLE, UNCLASSIFIED, UNCLASSIFIABLE, CLASSIFIED] and L.tolist() == [2, 0, 0, 0, 4]
    assert node.tolist() == [w.node("A,E"), 0, 0, 0, w.node("Q,R,T,U")]
    assert hund[0].tolist() == [95, 90] + [0] * 30 and hund[4].tolist() == [100] * 4 + [0] * 28 and not hund[1:4].any()
    rc, kind, L, node, hund = best(w, view, 79, 0, None)   # the cutoff is reached by equality
    assert L.tolist() == [3, 0, 0, 0, 4] and node[0] == w.node("A,E,G") and hund[0, :4].tolist() == [95, 90, 79, 0]
    # q0 and q2 have exactly one exact match, q4 two: the override replaces the best lineage of q0 and q2 by the reference's own, 100 on every level
    ids = np.array([lineage_of["J,K,M,N"], lineage_of["A,B,C"], lineage_of["A,B,C"], lineage_of["A,B,D"]], np.uint32)
    off = np.array([0, 1, 1, 2, 2, 4], np.uint64)
    rc, kind, L, node, hund = best(w, view, 80, 0, (ids, off))
    assert rc == 0 and kind.tolist() == [CLASSIFIED, UNCLASSIFIABLE, CLASSIFIED, UNCLASSIFIABLE, CLASSIFIED]
    assert L.tolist() == [4, 0, 3, 0, 4] and node.tolist() == [w.node("J,K,M,N"), 0, w.node("A,B,C"), 0, w.node("Q,R,T,U")]
    assert hund[0, :5].tolist() == [100] * 4 + [0] and hund[2, :4].tolist() == [100] * 3 + [0]
    plain = best(w, view, 80, 0, None)
    for flags in (_lib.RTX_SKIP_EXACT_MATCHES, _lib.RTX_RAW_CONFIDENCE, _lib.RTX_SKIP_EXACT_MATCHES | _lib.RTX_RAW_CONFIDENCE):   # either flag: no override
        got = best(w, view, 80, flags, (ids, off))
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], plain[1:]))
    for cutoff, flags in ((0, 0), (101, 0), (80, 4)):
        assert best(w, view, cutoff, flags, None)[0] == _lib.RTX_ERR_INVALID


def test_best_lineages_feed_the_taxonomy():
    """the Python path: a Result made of the hand-made view, rx.best_lineages, rx.otu_taxonomy_host"""
    w = world()
    view, keep, _ = hand_made_view(w)
    res = rx.Result(view)
    lin = rx.best_lineages(w.tree, res, cutoff=80)
    assert lin.kind.tolist() == [CLASSIFIED, UNCLASSIFIABLE, UNCLASSIFIED, UNCLASSIFIABLE, CLASSIFIED] and lin.L.tolist() == [2, 0, 0, 0, 4]
    otus = (np.array([0, 0, 0, 1, 1], np.uint32), np.array([5, 1, 1, 1, 3], np.uint64), np.array([0, 3], np.uint32))
    tax = rx.otu_taxonomy_host(w.tree, otus, lin)
    assert_tax(tax, brute(w.parent, otus, lin), "from a result")
    assert tax.depth.tolist() == [2, 4] and tax.seed_rel.tolist() == [0, 2]

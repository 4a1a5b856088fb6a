"""The taxon profile (rtx_index_profile_*, rtx_profile.hip) without a GPU: the numpy restatement that the GPU tests hold the device against
(checks.profile_expected) on a hand-worked tree with every number written out; the per-query step of the kernel (rtx_math.hpp:
profile_step) run on x86 against that restatement on random rows; the report (rtx_profile_format) byte for byte; the sum over handles
(rtx_profile_merge) and its refusals.

The tree, references in lineage order:
    0  A                          one level, directly under the root
    1  B,b1
    2  B,b2                       two references, one lineage: one Taxon leaf over ids 2 and 3
    3  B,b2
    4  C,c1,c2,c3,c4
    5  C,c1,c2,c3,c5
    6  D,d2,d3,...,d32            32 levels
"""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import checks

ROOT = Path(__file__).resolve().parent.parent
NONE = 0xFFFFFFFF
DEEP = ",".join(["D"] + [f"d{k}" for k in range(2, 33)])
LINEAGES = ["A", "B,b1", "B,b2", "B,b2", "C,c1,c2,c3,c4", "C,c1,c2,c3,c5", DEEP]


def make_tree(seed=3):
    rng = np.random.default_rng(seed)
    seqs = [(1 << rng.integers(0, 4, 80)).astype(np.uint8) for _ in LINEAGES]
    tree = rx.Tree.new(LINEAGES, seqs)
    assert tree.lineages == LINEAGES
    return tree, seqs


@pytest.fixture(scope="module")
def tree():
    return make_tree()[0]


@pytest.fixture(scope="module")
def nodes(tree):
    nv = tree.nodes()
    depth = np.zeros(len(nv["parent"]), np.int64)
    for v in range(1, len(depth)):
        depth[v] = depth[nv["parent"][v]] + 1
    nv["depth"] = depth
    return nv


def node_of(nodes, prefix):
    """The node of a lineage prefix such as 'C,c1': the node of that depth over the first reference whose lineage starts with it."""
    d = prefix.count(",") + 1
    r = next(i for i, l in enumerate(LINEAGES) if l == prefix or l.startswith(prefix + ","))
    hit = [v for v in range(len(nodes["depth"])) if nodes["depth"][v] == d and nodes["begin"][v] <= r < nodes["end"][v]]
    assert len(hit) == 1, (prefix, hit)
    return hit[0]


def deep(k):
    return ",".join(DEEP.split(",")[:k])


# ---- the hand-made batch: one row per query (the first row is all a profile reads), (lineage of the row's node, hundredths) ----
ROWS = [
    ("B,b1", [90, 50]),                                     # q0  exactly one exact match, reference 3: the override takes B,b2 with 100, 100
    ("B,b2", [95, 79]),                                     # q1  two exact matches (2 and 3): no override; 0 < L < depth at 80
    ("C,c1,c2,c3,c4", [79, 70, 60, 50, 40]),                # q2  L = 0 at 80
    ("C,c1,c2,c3,c5", [100, 100, 99, 85, 80]),              # q3  L = depth at 80
    ("A", [99]),                                            # q4  status 1: unclassifiable whatever its row says
    ("A", [80]),                                            # q5  one level, exactly at the cutoff
    (DEEP, [100] * 10 + [90] * 10 + [80] * 5 + [60] * 7),   # q6  32 levels: L = 25 at 80, 32 at 1, 10 at 100
    None,                                                   # q7  status 0 without a row: unclassifiable
    ("C,c1,c2,c3,c4", [100, 90, 0, 50, 50]),                # q8  stops at the FIRST level below the cutoff: L = 2 even at cutoff 1
    ("B,b1", [100, 100]),                                   # q9  status 2
    ("A", [0]),                                             # q10 L = 0 at every cutoff
    ("B,b1", [100, 100]),                                   # q11 status 1
]
STATUS = [0, 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 1]
EXACT = [[3], [2, 3], [], [], [0], [], [], [], [], [1], [], []]


def make_result(nodes):
    D = 32
    n = len(ROWS)
    row_off = np.zeros(n + 1, np.uint64)
    node, depth, hund = [], [], []
    for q, r in enumerate(ROWS):
        row_off[q + 1] = row_off[q] + (r is not None)
        if r is not None:
            node.append(node_of(nodes, r[0]))
            depth.append(len(r[1]))
            hund.append(r[1] + [0] * (D - len(r[1])))
    res = SimpleNamespace(n_queries=n, status=np.array(STATUS, np.uint8), row_off=row_off, row_node=np.array(node, np.uint32),
                          row_depth=np.array(depth, np.uint32), row_conf_hundredths=np.array(hund, np.uint8))
    exact_off = np.zeros(n + 1, np.uint64)
    exact_off[1:] = np.cumsum([len(e) for e in EXACT])
    exact_ids = np.array([i for e in EXACT for i in e], np.uint32)
    return res, exact_off, exact_ids


def table(nodes, rows):
    """{lineage prefix: (clade, direct, conf_sum)} -> the three arrays by node."""
    nn = len(nodes["depth"])
    clade, direct, conf = (np.zeros(nn, np.uint64) for _ in range(3))
    for prefix, (c, d, s) in rows.items():
        v = node_of(nodes, prefix)
        clade[v], direct[v], conf[v] = c, d, s
    return clade, direct, conf


def deep_rows(upto, direct_at):
    """The 32-level lineage of q6 counted down to level `upto`: 100 on levels 1-10, 90 on 11-20, 80 on 21-25, 60 on 26-32."""
    return {deep(k): (1, int(k == direct_at), 100 if k <= 10 else 90 if k <= 20 else 80 if k <= 25 else 60) for k in range(1, upto + 1)}


# (clade, direct, conf_sum) per node and the totals (queries, classified, unclassified, unclassifiable), worked by hand from ROWS
WANT = {
    (80, True): ({"A": (1, 1, 80), "B": (2, 1, 195), "B,b2": (1, 1, 100), "C": (2, 0, 200), "C,c1": (2, 1, 190), "C,c1,c2": (1, 0, 99),
                  "C,c1,c2,c3": (1, 0, 85), "C,c1,c2,c3,c5": (1, 1, 80), **deep_rows(25, 25)}, (12, 6, 2, 4)),
    (1, True): ({"A": (1, 1, 80), "B": (2, 0, 195), "B,b2": (2, 2, 179), "C": (3, 0, 279), "C,c1": (3, 1, 260), "C,c1,c2": (2, 0, 159),
                 "C,c1,c2,c3": (2, 0, 135), "C,c1,c2,c3,c4": (1, 1, 40), "C,c1,c2,c3,c5": (1, 1, 80), **deep_rows(32, 32)}, (12, 7, 1, 4)),
    (100, True): ({"B": (1, 0, 100), "B,b2": (1, 1, 100), "C": (2, 1, 200), "C,c1": (1, 1, 100), **deep_rows(10, 10)}, (12, 4, 4, 4)),
    # no override: q0 counts with its own row, B,b1 at 90 and 50
    (80, False): ({"A": (1, 1, 80), "B": (2, 2, 185), "C": (2, 0, 200), "C,c1": (2, 1, 190), "C,c1,c2": (1, 0, 99),
                   "C,c1,c2,c3": (1, 0, 85), "C,c1,c2,c3,c5": (1, 1, 80), **deep_rows(25, 25)}, (12, 6, 2, 4)),
    (1, False): ({"A": (1, 1, 80), "B": (2, 0, 185), "B,b1": (1, 1, 50), "B,b2": (1, 1, 79), "C": (3, 0, 279), "C,c1": (3, 1, 260), "C,c1,c2": (2, 0, 159),
                  "C,c1,c2,c3": (2, 0, 135), "C,c1,c2,c3,c4": (1, 1, 40), "C,c1,c2,c3,c5": (1, 1, 80), **deep_rows(32, 32)}, (12, 7, 1, 4)),
}


def test_the_header_declares_and_the_library_exports_the_additions():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+6\b", header)
    assert re.search(r"\}\s*rtx_profile_view\s*;", header)
    lib = rx._lib.load()
    for name in ("rtx_index_profile_begin", "rtx_index_profile_read", "rtx_index_profile_reset", "rtx_index_profile_end", "rtx_index_profile_time",
                 "rtx_profile_merge", "rtx_profile_format"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in rx._lib._SIGNATURES and hasattr(lib, name), name
    assert lib.rtx_abi_version() == 6


def test_the_tree_is_the_ragged_one(nodes):
    assert int(nodes["depth"].max()) == 32 and len(nodes["depth"]) == 1 + 1 + 3 + 6 + 32
    b2 = node_of(nodes, "B,b2")
    assert (int(nodes["begin"][b2]), int(nodes["end"][b2]), int(nodes["type"][b2])) == (2, 4, 1)   # one Taxon leaf over two references
    assert int(nodes["depth"][node_of(nodes, "A")]) == 1 and int(nodes["n_children"][node_of(nodes, "A")]) == 0


@pytest.mark.parametrize("cutoff, override_ok", sorted(WANT))
def test_expected_on_the_hand_worked_batch(nodes, cutoff, override_ok):
    res, exact_off, exact_ids = make_result(nodes)
    clade, direct, conf, totals, seen = checks.profile_expected(nodes, res, exact_off, exact_ids, cutoff, override_ok)
    rows, want_totals = WANT[cutoff, override_ok]
    wc, wd, ws = table(nodes, rows)
    assert np.array_equal(clade, wc) and np.array_equal(direct, wd) and np.array_equal(conf, ws)
    assert tuple(int(x) for x in totals) == want_totals
    assert seen["override"] == (1 if override_ok else 0) and seen["several_exact"] == 1 and seen["not_ok"] == 4
    if cutoff == 80:
        assert seen["l_zero"] == 2 and seen["l_partial"] == (3 if override_ok else 4) and seen["l_full"] == (3 if override_ok else 2)
    # the invariants of the definition: the root stays 0, a clade is its direct count and its children's clades, the direct counts are the classified
    assert clade[0] == 0 and direct[0] == 0 and int(direct.sum()) == int(totals[1]) and int(totals[1:].sum()) == int(totals[0])
    kids = np.zeros(len(clade), np.uint64)
    np.add.at(kids, nodes["parent"][1:].astype(np.int64), clade[1:])
    assert np.array_equal(clade[1:], (direct + kids)[1:])


def _emul_profile(emul, nodes, res, one, cutoff):
    nn = len(nodes["depth"])
    leaf = np.full(len(LINEAGES), NONE, np.uint32)
    for v in range(1, nn):
        if nodes["type"][v] == 1:
            leaf[int(nodes["begin"][v]):int(nodes["end"][v])] = v
    a = dict(status=res.status.astype(np.uint8), row_count=np.diff(res.row_off.astype(np.int64)).astype(np.uint32), row_begin=res.row_off[:-1].astype(np.uint64),
             row_node=res.row_node.astype(np.uint32), row_depth=res.row_depth.astype(np.uint8), row_hund=np.ascontiguousarray(res.row_conf_hundredths, dtype=np.uint8),
             parent=nodes["parent"].astype(np.uint32), node_depth=nodes["depth"].astype(np.uint8), leaf=leaf, one=np.ascontiguousarray(one, dtype=np.uint32))
    a = {k: np.ascontiguousarray(v) for k, v in a.items()}
    out = [np.zeros(nn, np.uint64) for _ in range(3)] + [np.zeros(4, np.uint64)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    emul.emul_profile.restype = None
    emul.emul_profile(C.c_uint64(res.n_queries), p(a["status"]), p(a["row_count"]), p(a["row_begin"]), p(a["row_node"]), p(a["row_depth"]), p(a["row_hund"]),
                      C.c_uint32(res.row_conf_hundredths.shape[1]), p(a["parent"]), p(a["node_depth"]), p(a["leaf"]), C.c_uint32(nn), C.c_uint32(len(LINEAGES)),
                      p(a["one"]), C.c_uint32(cutoff), *[p(x) for x in out])
    return out


def _one(exact_off, exact_ids, override_ok):
    n = len(exact_off) - 1
    cnt = np.diff(exact_off.astype(np.int64))
    one = np.full(n, NONE, np.uint32)
    if override_ok:
        sel = cnt == 1
        one[sel] = exact_ids[exact_off[:-1].astype(np.int64)[sel]]
    return one


@pytest.mark.parametrize("cutoff, override_ok", sorted(WANT))
def test_the_emulated_step_on_the_hand_worked_batch(emul, nodes, cutoff, override_ok):
    res, exact_off, exact_ids = make_result(nodes)
    got = _emul_profile(emul, nodes, res, _one(exact_off, exact_ids, override_ok), cutoff)
    rows, want_totals = WANT[cutoff, override_ok]
    for g, w in zip(got[:3], table(nodes, rows)):
        assert np.array_equal(g, w)
    assert tuple(int(x) for x in got[3]) == want_totals


def test_the_emulated_step_on_random_rows(emul, nodes):
    rng = np.random.default_rng(11)
    n, D, nn = 2000, 32, len(nodes["depth"])
    status = (rng.random(n) < 0.1).astype(np.uint8) * rng.integers(1, 3, n).astype(np.uint8)
    count = np.where(rng.random(n) < 0.05, 0, rng.integers(1, 4, n))
    row_off = np.zeros(n + 1, np.uint64)
    row_off[1:] = np.cumsum(count)
    nr = int(row_off[-1])
    node = rng.integers(1, nn, nr).astype(np.uint32)
    depth = nodes["depth"][node].astype(np.uint32)
    hund = np.zeros((nr, D), np.uint8)
    for r in range(nr):   # confidences fall along a lineage, sometimes from 100 in long runs, sometimes below every cutoff at once
        h = np.sort(rng.integers(0, 101, depth[r]))[::-1] if rng.random() < 0.7 else np.minimum(100, np.sort(rng.integers(60, 140, depth[r]))[::-1])
        hund[r, :depth[r]] = h
    res = SimpleNamespace(n_queries=n, status=status, row_off=row_off, row_node=node, row_depth=depth, row_conf_hundredths=hund)
    n_exact = rng.choice([0, 0, 1, 1, 2, 3], n)
    exact_off = np.zeros(n + 1, np.uint64)
    exact_off[1:] = np.cumsum(n_exact)
    exact_ids = rng.integers(0, len(LINEAGES), int(exact_off[-1])).astype(np.uint32)
    for cutoff in (1, 50, 80, 100):
        for override_ok in (True, False):
            want = checks.profile_expected(nodes, res, exact_off, exact_ids, cutoff, override_ok)
            got = _emul_profile(emul, nodes, res, _one(exact_off, exact_ids, override_ok), cutoff)
            for g, w in zip(got, want[:4]):
                assert np.array_equal(g, w), (cutoff, override_ok)
            seen = want[4]
            if cutoff in (50, 80):   # (at cutoff 1 next to nothing is unclassified, at 100 next to nothing reaches its leaf: equality is what counts there)
                assert min(seen["l_zero"], seen["l_partial"], seen["l_full"], seen["not_ok"], seen["several_exact"]) > 0, seen
            assert (seen["override"] > 0) == override_ok


# ---- the report: cutoff 1 of the hand-worked batch, 12 queries.  percent: 1 / 12 = 8.333 -> 8.33 (down), 2 / 12 = 16.667 -> 16.67 (up), 3 / 12 = 25.00;
# mean_conf: 195 / 2 = 97.5 -> 0.98 (half goes up), 260 / 3 = 86.67 -> 0.87 (up), 279 / 3 = 93 exactly; B, C and the inner levels have direct == 0;
# B,b1 (clade 0) has no line; the one-level A, the two-level B,b2, the five-level C lineages and the 32 levels of D come in pre-order
REPORT_HEAD = ("# cutoff=0.01\tqueries=12\tclassified=7\tunclassified=1\tunclassifiable=4\n"
               "clade\tdirect\tpercent\tmean_conf\tdepth\ttaxon\tlineage\n"
               "1\t1\t8.33\t0.80\t1\tA\tA\n"
               "2\t0\t16.67\t0.98\t1\tB\tB\n"
               "2\t2\t16.67\t0.90\t2\tb2\tB,b2\n"
               "3\t0\t25.00\t0.93\t1\tC\tC\n"
               "3\t1\t25.00\t0.87\t2\tc1\tC,c1\n"
               "2\t0\t16.67\t0.80\t3\tc2\tC,c1,c2\n"
               "2\t0\t16.67\t0.68\t4\tc3\tC,c1,c2,c3\n"
               "1\t1\t8.33\t0.40\t5\tc4\tC,c1,c2,c3,c4\n"
               "1\t1\t8.33\t0.80\t5\tc5\tC,c1,c2,c3,c5\n"
               "1\t0\t8.33\t1.00\t1\tD\tD\n"
               "1\t0\t8.33\t1.00\t2\td2\tD,d2\n")


def _report_tail():
    lines = []
    for k in range(3, 33):
        mean = "1.00" if k <= 10 else "0.90" if k <= 20 else "0.80" if k <= 25 else "0.60"
        lines.append(f"1\t{int(k == 32)}\t8.33\t{mean}\t{k}\td{k}\t{deep(k)}\n")
    return "".join(lines)


def test_the_report_byte_for_byte(tree, nodes):
    rows, totals = WANT[1, True]
    clade, direct, conf = table(nodes, rows)
    prof = rx.Profile(1, 0, clade, direct, conf, np.array(totals, np.uint64))
    text = rx.profile_text(tree, prof)
    assert text == REPORT_HEAD + _report_tail()
    # the bytes needed, and a buffer that is too small answered as rtx_records_format answers it
    lib = rx._lib.load()
    u64 = lambda x: x.ctypes.data_as(rx._lib.u64p)
    tot = np.array(totals, np.uint64)
    need = lib.rtx_profile_format(tree._h, u64(clade), u64(direct), u64(conf), u64(tot), 1, None, 0)
    assert need == len(text.encode())
    small = C.create_string_buffer(16)
    assert lib.rtx_profile_format(tree._h, u64(clade), u64(direct), u64(conf), u64(tot), 1, small, 16) == -need - 1024
    # cutoff 100 prints 1.00; an empty profile is its two head lines
    zero = rx.Profile(100, 0, np.zeros_like(clade), np.zeros_like(clade), np.zeros_like(clade), np.zeros(4, np.uint64))
    assert rx.profile_text(tree, zero) == "# cutoff=1.00\tqueries=0\tclassified=0\tunclassified=0\tunclassifiable=0\n" + REPORT_HEAD.split("\n")[1] + "\n"


def test_merge_sums_and_refuses(nodes):
    a_rows, a_tot = WANT[80, True]
    b_rows, b_tot = WANT[80, False]
    a = rx.Profile(80, 0, *table(nodes, a_rows), np.array(a_tot, np.uint64))
    b = rx.Profile(80, 0, *table(nodes, b_rows), np.array(b_tot, np.uint64))
    m = rx.profile_merge([a, b, a])
    for f in ("clade", "direct", "conf_sum", "totals"):
        assert np.array_equal(getattr(m, f), 2 * getattr(a, f) + getattr(b, f)), f
    assert (m.cutoff, m.flags) == (80, 0)
    one = rx.profile_merge([a])
    assert np.array_equal(one.clade, a.clade) and np.array_equal(one.totals, a.totals)
    for other in (rx.Profile(81, 0, b.clade, b.direct, b.conf_sum, b.totals), rx.Profile(80, 1, b.clade, b.direct, b.conf_sum, b.totals),
                  rx.Profile(80, 0, b.clade[:-1].copy(), b.direct[:-1].copy(), b.conf_sum[:-1].copy(), b.totals)):
        with pytest.raises(rx.RtxError) as e:
            rx.profile_merge([a, other])
        assert e.value.code == rx._lib.RTX_ERR_INVALID

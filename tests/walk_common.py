"""Exact inputs for the lineage evaluation (lineage.rs:61-179: prefix sums, the walk with its fallback chain, the stable sort).

Every probability here is a non-negative multiple of 2^-40 and every vector sums to exactly 1, so every partial sum, in any
order, is exact in double precision: the device, the oracle and the reference must agree bit for bit, ties between siblings
included.  The cases are built so that the rules no real input pins decide the answer: the LAST maximum of the fallback chain,
the 64-wide chunks of a node's children, rounding half away from zero, the stable order of equal rows, the boundaries of the
prefix kernel's threads / waves / sweeps / tiles and the gaps skipped tiles leave.

No GPU and no device code in here: evaluate_exact is a plain restatement of the reference in rational arithmetic."""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction
from itertools import accumulate

import numpy as np

U = 1 << 40                     # the unit: every probability is a whole number of 2^-40
INNER, TAXON, SEQUENCE = 0, 1, 2
MAX_DEPTH = 32                  # RTX_MAX_DEPTH
MAX_ROWS = 200                  # a row needs a confidence that rounds to 0.01 or more: at most 200 of them (kWalkMaxRows = 208)
TILE = 8192                     # references per tile of the prefix kernel


def u(e: int) -> int:
    """2^-e in units."""
    return U >> e


@dataclass
class Case:
    name: str
    tree: str                   # cases with the same key have the same lineages (one index serves them)
    lineages: list
    units: np.ndarray           # int64 [n]: probability in units of 2^-40
    note: str
    modes: tuple = (0, 1, 2)
    meta: dict = field(default_factory=dict)
    sequential_only: bool = False   # fewer than 9 references, relies on sequential order: exempt from the 2^-40 check (none so far)

    @property
    def probs(self) -> np.ndarray:
        return self.units.astype(np.float64) * 2.0 ** -40   # exact: the units are below 2^53


def sequences(n: int):
    """The cheapest references that build: 12 identical bases each (the walk never looks at them).  Flat bytes and offsets."""
    return np.full(12 * n, 1, np.uint8), (np.arange(n + 1, dtype=np.uint64) * 12)


def assert_dyadic(probs, sequential_only: bool = False):
    fr = [Fraction(float(p)) for p in probs]
    assert all(f >= 0 for f in fr)
    assert sum(fr) == 1
    if sequential_only:
        assert len(fr) < 9
        return
    assert all((f * U).denominator == 1 for f in fr)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference, restated (tree.rs:46-140, lineage.rs:61-179)
# ---------------------------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("label", "lo", "hi", "type", "children")

    def __init__(self, label, lo, typ):
        self.label, self.lo, self.hi, self.type, self.children = label, lo, lo + 1, typ, []


def build_tree(lineages) -> Node:
    """tree.rs:55-107 over lineages that are already in the tree's (sorted) order: a node per level, found again only as the LAST
    child of its parent; a Taxon where a lineage ends, with a Sequence child per reference."""
    root = Node("root", 0, INNER)
    idx = 0
    for lin in lineages:
        levels = lin.split(",")
        cur = root
        for k, name in enumerate(levels):
            if not cur.children or cur.children[-1].label != name:
                cur.children.append(Node(name, idx, TAXON if k == len(levels) - 1 else INNER))
            cur.hi = idx + 1
            cur = cur.children[-1]
        idx += 1
        cur.children.append(Node(cur.label, idx - 1, SEQUENCE))
        cur.hi = idx
    root.hi = idx
    return root


def exact_prefix(probs):
    """(prefix sums as integers, their common denominator): the doubles taken exactly."""
    nz = [(i, Fraction(float(p))) for i, p in enumerate(probs) if p != 0.0]
    den = max((f.denominator for _, f in nz), default=1)      # denominators of doubles are powers of two: the largest is the common one
    units = [0] * len(probs)
    for i, f in nz:
        units[i] = f.numerator * (den // f.denominator)
    return [0] + list(accumulate(units)), den


def hundredths(conf: Fraction, half_even: bool = False) -> int:
    x = conf * 100
    if half_even:
        return round(x)                                        # (Python rounds a Fraction half to even)
    return (x + Fraction(1, 2)).__floor__() if x >= 0 else -((-x + Fraction(1, 2)).__floor__())   # f64::round: half away from zero


def evaluate_exact(lineages, probs, *, first_max=False, half_even=False, unstable=False, stats=None, root=None):
    """Lineage::evaluate in rational arithmetic: [(first lineage index, hundredths per level)] in the order of the result.
    first_max / half_even / unstable switch one rule each to the plausible wrong one (what a test must be able to tell apart);
    stats, if given, counts the fallbacks that met a tie and the significant children at index 64 or above."""
    root = root or build_tree(lineages)
    prefix, den = exact_prefix(probs)
    conf = lambda nd: Fraction(prefix[nd.hi] - prefix[nd.lo], den)
    rows = []

    def recurse(node, path):                                   # lineage.rs:119-179
        no_sig, pushed = True, False
        for i, c in enumerate(node.children):
            k = hundredths(conf(c), half_even)
            if k == 0:
                continue
            no_sig = False
            if stats is not None and i >= 64:
                stats["sig_child_ge64"] += 1
            child_pushed = recurse(c, path + [k])
            if not child_pushed and c.type == TAXON:           # :141-149
                rows.append((c.lo, path + [k]))
                pushed = True
            pushed |= child_pushed
        if no_sig and node.type == INNER:                      # :151-177: the chain of largest children, by unrounded sums
            cur, p = node, list(path)
            while cur.type == INNER:
                vals = [conf(c) for c in cur.children]
                at = [i for i, v in enumerate(vals) if v == max(vals)]
                if stats is not None and len(at) > 1:
                    stats["fallback_tie"] += 1
                cur = cur.children[at[0] if first_max else at[-1]]   # Iterator::max_by keeps the LAST maximum
                p.append(1)
            rows.append((cur.lo, p))
            pushed = True
        return pushed

    recurse(root, [])
    if unstable:
        rows.reverse()
    return sorted(rows, key=lambda r: r[1], reverse=True)      # :91-93 stable, descending; a shorter prefix compares as less


def oracle_rows_exact(rows):
    """The oracle's rows in the form evaluate_exact returns."""
    return [(r["idx"], [int(round(c * 100)) for c in r["conf"]]) for r in rows]


def compare(res, oracle_rows, what=""):
    """A device result of one pseudo-query against OracleTree.lineage_evaluate: the number and order of rows, lineage indices,
    depths and hundredths equal; the two signals within 1e-12 (what test_device_math_cpu holds the same arithmetic to)."""
    assert res.n_queries == 1 and int(res.status[0]) == 0, what
    n = int(res.row_off[1])
    depth = [int(res.row_depth[r]) for r in range(n)]
    got = [(int(res.row_lineage[r]), [int(x) for x in res.row_conf_hundredths[r, :depth[r]]]) for r in range(n)]
    want = oracle_rows_exact(oracle_rows)
    assert n == len(oracle_rows), f"{what}: {n} rows, the oracle has {len(oracle_rows)}: {got[:8]} / {want[:8]}"
    assert depth == [len(r["conf"]) for r in oracle_rows], what
    first = next((i for i in range(n) if got[i] != want[i]), None)
    assert first is None, f"{what}: row {first}: {got[first]}, the oracle has {want[first]}"
    for r, o in enumerate(oracle_rows):
        assert [float(x) for x in res.row_conf[r, :depth[r]]] == o["conf"], (what, r)
        assert abs(float(res.row_local_signal[r]) - o["local_signal"]) <= 1e-12, (what, r)
        assert abs(float(res.global_signal[0]) - o["global_signal"]) <= 1e-12, (what, r)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _case(name, tree, masses: dict, note, **kw) -> Case:
    """masses: lineage -> units (a lineage may be listed with 0).  The tree's order is the bytewise order of the lineages."""
    lineages = sorted(masses)
    units = np.array([masses[l] for l in lineages], dtype=np.int64)
    assert int(units.sum()) == U, (name, int(units.sum()))
    return Case(name, tree, lineages, units, note, **kw)


def _units_case(name, tree, lineages, at: dict, note, **kw) -> Case:
    units = np.zeros(len(lineages), np.int64)
    for i, m in at.items():
        units[i] += m
    assert int(units.sum()) == U, (name, int(units.sum()))
    return Case(name, tree, lineages, units, note, **kw)


def wide_chunks():
    lin = [f"p:T{i:03d},s:S{i:03d}" for i in range(200)]
    at = {63: u(2), 64: u(2), 127: u(2), 128: u(3), 199: u(4)}
    small = [i for i in range(200) if i not in at]
    for i in small[:16]:
        at[i] = u(12)                                          # sixteen of 2^-12 and fifteen of 2^-8, all insignificant: the last 1/16
    for i in small[20:35]:
        at[i] = u(8)
    return [_units_case("wide_chunks", "wide_chunks", lin, at, "significant children at 63, 64, 127, 128, 199 of a node of 200: the edges "
                        "of the 64-wide scan, `next` resumed after every return from a child", meta=dict(node=[], named=[63, 64, 127, 128, 199], rows=5))]


def wide_nested():
    masses = {}
    outer = 130
    for p in range(outer):
        if p in (70, 100):
            for c in range(140):
                masses[f"p:P{p:03d},c:C{c:03d}"] = 0
        else:
            masses[f"p:P{p:03d},c:C000"] = 0
    for c, e in ((65, 2), (127, 3), (128, 3), (139, 4), (0, 8), (63, 8)):
        masses[f"p:P070,c:C{c:03d}"] = u(e)
    for c, e in ((64, 2), (130, 3), (1, 8), (66, 8)):
        masses[f"p:P100,c:C{c:03d}"] = u(e)
    for p in (0, 63, 64, 69, 71, 99, 101, 127, 128, 129, 5, 6):
        masses[f"p:P{p:03d},c:C000"] = u(8)
    return [_case("wide_nested", "wide_nested", masses, "two significant children (70, 100) in the second chunk of a node of 130, each with "
                  "significant children in the second and third chunk of its own 140: the outer node's saved mask must still name child 100",
                  meta=dict(nodes=[([], [70, 100]), ([70], [65, 127, 128, 139]), ([100], [64, 130])]))]


def _fallback_tree(n_cls=130):
    return [f"p:A,c:C{i:03d},s:S{i:03d}" for i in range(n_cls)] + ["p:B,c:C,s:S"]


def fallback_last_max():
    lin = _fallback_tree()
    out = []
    for name, maxima in (("fallback_last_max", [5, 69, 70]), ("fallback_all_equal", list(range(130))), ("fallback_max_0_64", [0, 64])):
        at = {i: u(9) for i in range(130)}
        if len(maxima) < 130:
            for i in maxima:
                at[i] = u(8)
        at[130] = U - sum(at.values())
        out.append(_units_case(name, "fallback", lin, at, f"130 insignificant classes under a significant phylum, the largest at {maxima if len(maxima) < 130 else 'all of them'}: "
                               "the last one wins (lane 5 meets 5 and 69 in two trips, 70 is another lane's)", meta=dict(chain=[([0], maxima)], row=maxima[-1])))
    # a chain three levels long, every level wider than 64 with a tie of its own
    v = 1 << 20                                                # 2^-20
    masses = {"p:B,c:C,o:O,f:F": 0}
    for c in range(66):
        if c != 65:
            masses[f"p:A,c:C{c:03d},o:O000,f:F000"] = (648 if c == 10 else 100) * v
    for o in range(66):
        if o != 64:
            masses[f"p:A,c:C065,o:O{o:03d},f:F000"] = (68 if o == 3 else 8) * v
    for f in range(66):
        masses[f"p:A,c:C065,o:O064,f:F{f:03d}"] = (2 if f in (1, 65) else 1) * v
    masses["p:B,c:C,o:O,f:F"] = U - sum(masses.values())
    c3 = _case("fallback_three_levels", "fallback3", masses, "a fallback chain through three nodes of 66 children, each with two largest children "
               "(10 | 65, 3 | 64, 1 | 65): the last at every level", meta=dict(chain=[([0], [10, 65]), ([0, 65], [3, 64]), ([0, 65, 64], [1, 65])]))
    c3.meta["row"] = c3.lineages.index("p:A,c:C065,o:O064,f:F065")
    return out + [c3]


def fallback_not_at_taxon():
    lin = ["p:A", "p:A,c:B", "p:A,c:B,s:C", "p:A,c:D", "p:E"]
    vs = [[u(8), u(8), u(8), u(8), U - u(6)], [u(1), u(2), u(3), u(4), u(4)], [u(1), 0, 0, 0, u(1)], [0, 0, u(1), 0, u(1)]]
    note = "Taxa that have Taxon children: a Taxon without a significant child gets its own row and no fallback"
    return [Case(f"fallback_not_at_taxon_{k}", "not_at_taxon", lin, np.array(v, np.int64), note, meta=dict(expect=[(4, [98]), (1, [2, 1])] if k == 0 else None))
            for k, v in enumerate(vs)]


def stable_equal_rows():
    lin = [f"p:T{i:03d}" for i in range(128)]
    return [Case("stable_equal_rows", "stable", lin, np.full(128, u(7), np.int64), "128 rows with the same confidence vector: they come back in the order of the walk")]


def sort_depth_tie():
    lin = ["p:A,s:X", "p:B,c:Y,s:Z", "p:C,s:W", "p:D,c:V,s:U"]
    return [Case("sort_depth_tie", "depth_tie", lin, np.full(4, u(2), np.int64), "equal prefixes: the longer vector first, then the order of the walk",
                 meta=dict(order=[1, 3, 0, 2]))]


def round_half_away():
    a = Case("round_half_away_3", "half3", ["p:A,s:X", "p:B,s:Y", "p:C,s:Z"], np.array([u(3), u(2), 5 * u(3)], np.int64), "12.5 -> 13, 62.5 -> 63",
             meta=dict(seen=[13, 25, 63]))
    b = Case("round_half_away_2", "half2", ["p:A,s:X", "p:B,s:Y"], np.array([3 * u(3), 5 * u(3)], np.int64), "37.5 -> 38, 62.5 -> 63", meta=dict(seen=[38, 63]))
    lin = ["p:A,c:B,s:X", "p:A,c:B,s:Y", "p:A,c:C,s:Z", "p:D,c:E,s:V", "p:D,c:E,s:W", "p:D,c:F,s:U"]
    c = Case("round_half_away_levels", "half_levels", lin, np.array([u(3), u(2), u(3), u(3), u(3), u(2)], np.int64),
             "halves at the species and the class level (12.5, 37.5) beside whole hundredths", meta=dict(seen=[13, 38]))
    return [a, b, c]


def deepest():
    D = MAX_DEPTH
    chain = lambda head, frm, tag: head + [f"l{k:02d}:{tag}" for k in range(frm, D)]
    masses = {}
    masses[",".join(chain([], 0, "a"))] = u(1)                                               # differs from the rest at level 0
    half = [f"l{k:02d}:b" for k in range(16)]
    masses[",".join(chain(half, 16, "m0"))] = u(2)                                            # ... at a middle level
    masses[",".join(chain(half, 16, "m1"))] = u(3)
    deep = [f"l{k:02d}:c" for k in range(D - 1)]
    for j in range(8):                                                                        # ... at level 31 only
        masses[",".join(deep + [f"l31:s{j}"])] = u(6) - (u(8) if j in (2, 5) else 0)
    for j in range(2):                                                                        # a fallback chain of 30 levels under l00:d,l01:d
        masses[",".join(chain(["l00:d", "l01:d"], 2, f"e{j}"))] = u(8)
    for j in range(51):                                                                       # without mass: branches off the first chain at every level
        k = 1 + j % (D - 1)
        masses[",".join(chain([f"l{i:02d}:a" for i in range(k)], k, f"z{j:02d}"))] = 0
    c = _case("deepest", "deepest", masses, "64 references of 32 levels: rows that differ at level 0, at level 16 and at level 31 only; a fallback chain "
              "of 30 levels (two tied children of 2^-8 under an ancestor of 2^-7)")
    assert len(c.lineages) == 64 and all(l.count(",") == D - 1 for l in c.lineages)
    return [c]


def tiled_lineages(n):
    """Species of one reference, genera of 8, families of 512, orders of 1024, classes of 8192: taxonomy boundaries on the edges of the
    prefix kernel's threads (8 references), waves (512), sweeps (1024) and tiles (8192)."""
    return [f"k:K{i >> 13:02d},o:O{i >> 10:03d},f:F{i >> 9:03d},g:G{i >> 3:05d},s:S{i:06d}" for i in range(n)]


PREFIX_EDGE_N = (1, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 65535)


def prefix_edges():
    out = []
    for n in PREFIX_EDGE_N:
        pts = sorted({i for i in (0, 7, 8, 511, 512, 1023, 1024, 8191, 8192, n - 1) if i < n})
        k = len(pts)
        at = {p: (u(j + 1) if j < k - 1 else u(max(k - 1, 0))) for j, p in enumerate(pts)}    # 1/2, 1/4, ..., the last one twice: sums to 1
        run = 1536 if n >= 2048 else (256 if n >= 320 else None)                              # 64 references of 2^-11 taken out of the first point
        if run is not None:
            at[0] -= u(5)
            for i in range(run, run + 64):
                at[i] = u(11)
        meta = dict(n=n, fallback_family=run == 1536)
        out.append(_units_case(f"prefix_edges_{n}", f"tiled_{n}", tiled_lineages(n), at, "mass on the references at the edges of threads, waves, sweeps and tiles"
                               + (", 64 references of 2^-11 that make a family of their own: a fallback under a significant order" if run == 1536 else ""), meta=meta))
        if n == 8193:   # thousands of distinct values: the probability table does not fit LDS (the global-memory variant of the prefix kernel)
            at2 = dict(at)
            for i in range(3000):
                at2[4096 + i] = (i + 1) << 10
            at2[0] -= sum((i + 1) << 10 for i in range(3000))
            out.append(_units_case("prefix_edges_8193_many_values", "tiled_8193", tiled_lineages(n), at2, "the same with 3000 further distinct values", meta=dict(meta, many_values=True)))
    return out


def _tile_points(n, live, shares):
    """Mass on the first and the last reference of every live tile and on its offsets 511 and 512 (1 and 2 in a tile of fewer than 513)."""
    at = {}
    for t in live:
        lo, hi = t * TILE, min((t + 1) * TILE, n)
        offs = [0, 511, 512, hi - lo - 1] if hi - lo > 513 else sorted({0, min(1, hi - lo - 1), min(2, hi - lo - 1), hi - lo - 1})
        for o, e in zip(offs, shares):
            at[lo + o] = at.get(lo + o, 0) + e
        if len(offs) < len(shares):
            at[lo] += sum(shares[len(offs):])
    return at


def tile_gaps():
    out = []
    q = (u(3), u(4), u(5), u(5))                               # a quarter per live tile
    for name, n, live in (("tile_gaps", 8 * TILE, (1, 3, 5, 7)), ("tile_gaps_minus_1", 8 * TILE - 1, (1, 3, 5, 7)),
                          ("tile_gaps_plus_1", 8 * TILE + 1, (1, 3, 5, 8)), ("tile_gaps_last_dead", 8 * TILE, (0, 2, 4, 6))):
        out.append(_units_case(name, f"tiled_{n}", tiled_lineages(n), _tile_points(n, live, q), f"only tiles {live} of {(n + TILE - 1) // TILE} hold mass: "
                               "the boundaries of the others reach the fused walk as gaps", meta=dict(n=n, live=live)))
    return out


def tile_gaps_overflow():
    n, live = 16 * TILE + 5, (1, 3, 5, 7, 9, 11, 13, 16)
    return [_units_case("tile_gaps_overflow", f"tiled_{n}", tiled_lineages(n), _tile_points(n, live, (u(4), u(5), u(6), u(6))), "eight runs of dead tiles: six gaps, the "
                        "seventh and eighth written out; significant taxa on both sides of the sixth gap and in the last tile of five references",
                        meta=dict(n=n, live=live, rows=32))]


def small_cases():
    return (wide_chunks() + wide_nested() + fallback_last_max() + fallback_not_at_taxon() + stable_equal_rows() + sort_depth_tie() + round_half_away() + deepest())


def all_cases():
    return small_cases() + prefix_edges() + tile_gaps() + tile_gaps_overflow()


# ---------------------------------------------------------------------------------------------------------------------------
# seeded fuzz: 12 trees, 30 vectors each
# ---------------------------------------------------------------------------------------------------------------------------
FUZZ_TREES, FUZZ_VECTORS, FUZZ_MAX_N = 12, 30, 20_000
FANOUTS = (1, 2, 3, 63, 64, 65, 130)


def fuzz_tree(seed: int):
    """Lineages of depth 1 to 8 and of variable length, fan-outs from FANOUTS, at most FUZZ_MAX_N references."""
    rng = np.random.default_rng(1000 + seed)
    depth = int(rng.integers(1, 9))
    lineages = []

    def grow(prefix, level, wide_left):
        wide = level == 0 or (wide_left > 0 and rng.random() < 0.2)
        fan = int(rng.choice(FANOUTS[3:] if wide else FANOUTS[:3]))
        for i in range(fan):
            if len(lineages) >= FUZZ_MAX_N - 1:
                break
            name = prefix + [f"l{level}:n{i:03d}"]
            ends = level + 1 == depth or rng.random() < 0.15
            if ends or rng.random() < 0.05:                    # a lineage that ends here (and, the second way, goes on below as well)
                for _ in range(1 + (rng.random() < 0.1)):      # now and then two references of one taxon
                    lineages.append(",".join(name))
            if not ends:
                grow(name, level + 1, wide_left - wide)
        return

    grow([], 0, 1)
    lineages.sort()
    return lineages


def fuzz_vectors(seed: int, lineages, root=None):
    """FUZZ_VECTORS of (units, mode): a composition of what is left of 2^40 over 1 to 40 references, beside a run of equal dyadic masses
    under one random ancestor (ties and fallbacks); the mode of the tap the vector is run in."""
    rng = np.random.default_rng(5000 + seed)
    n = len(lineages)
    root = root or build_tree(lineages)
    inner, late = [], []                                       # nodes of two references or more; children at index 64 or above

    def collect(nd):
        if nd.type != SEQUENCE and nd.hi - nd.lo >= 2:
            inner.append(nd)
        late.extend(nd.children[64:])
        for c in nd.children:
            collect(c)

    collect(root)
    out = []
    for _ in range(FUZZ_VECTORS):
        units = np.zeros(n, np.int64)
        left = U
        if inner:
            nd = inner[int(rng.integers(len(inner)))]
            k = int(rng.integers(1, max(2, min(8, (nd.hi - nd.lo).bit_length()))))   # 2^k references of the ancestor, from its first
            total = int(rng.integers(2, 8))                                            # ... that hold 2^-total together
            units[nd.lo:nd.lo + (1 << k)] = u(total + k)
            left -= u(total)
        m = int(rng.integers(1, min(40, n) + 1))
        where = rng.choice(n, size=m, replace=False)
        if late and rng.random() < 0.5:                                                # every second vector: mass below a child at index 64 or above
            nd = late[int(rng.integers(len(late)))]
            r = int(rng.integers(nd.lo, nd.hi))
            if r not in where:
                where[0] = r
        g = u(int(rng.choice([7, 8, 9, 40])))                                          # coarse parts round to halves and tie, fine ones do not
        parts = left // g
        cuts = np.sort(rng.integers(0, parts - m + 1, size=m - 1))                     # m positive parts: one each and a composition of the rest
        sizes = np.diff(np.concatenate([[0], cuts, [parts - m]])).astype(np.int64) + 1
        units[where] += sizes * g
        assert int(units.sum()) == U
        out.append((units, int(rng.integers(0, 3))))
    return out

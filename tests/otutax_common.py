"""The consensus taxonomy of the OTUs (raxtax_hip.h, "Consensus taxonomy of the OTUs") restated as brute-force Python, and the worlds the CPU
and GPU tests share: small trees built through rtx_tree_build, synthetic records (nothing is classified), OTUs given as plain arrays."""
from functools import lru_cache

import numpy as np

import raxtax_amd as rx
from raxtax_amd import _lib

MAX_DEPTH = _lib.RTX_MAX_DEPTH
UNCLASSIFIABLE, UNCLASSIFIED, CLASSIFIED = _lib.RTX_LIN_UNCLASSIFIABLE, _lib.RTX_LIN_UNCLASSIFIED, _lib.RTX_LIN_CLASSIFIED
FIELDS = ("sizes", "members", "classified", "depth", "node", "seed_rel", "clade", "conf")

# a dozen lineages of depth 3 .. 4, and one chain of depth RTX_MAX_DEPTH
LINEAGES = ["A,B,C", "A,B,D", "A,E,F", "A,E,G,H", "A,E,G,I", "J,K,L", "J,K,M,N", "J,O,P", "Q,R,S", "Q,R,T,U", "Q,V,W", "X,Y,Z",
            ",".join(f"c{d}" for d in range(MAX_DEPTH))]


class World:
    """A tree and its nodes by name: node("A,E,G") is the node id of that prefix, depth its levels"""

    def __init__(self, lineages):
        rng = np.random.default_rng(5)
        self.tree = rx.Tree.new(list(lineages), [rng.choice(np.array([1, 2, 4, 8], np.uint8), 40) for _ in lineages])
        n = self.tree.nodes()
        self.parent = n["parent"]
        self.n_nodes = len(self.parent)
        self.depth = np.zeros(self.n_nodes, np.uint32)
        for v in range(1, self.n_nodes):
            assert self.parent[v] < v
            self.depth[v] = self.depth[self.parent[v]] + 1
        lib = _lib.load()
        self.lineages = [lib.rtx_tree_lineage(self.tree._h, i).decode() for i in range(len(lineages))]
        self.by_name = {}
        for v in range(1, self.n_nodes):
            levels = self.lineages[int(n["begin"][v])].split(",")[:int(self.depth[v])]
            self.by_name[",".join(levels)] = v
        self.names = sorted(self.by_name)

    def node(self, name):
        return self.by_name[name]


@lru_cache(maxsize=None)
def world():
    return World(LINEAGES)


class Case:
    """Rows given one by one: add(otu, weight, name or None, hund=...); seeds default to the first row of every OTU"""

    def __init__(self, w=None):
        self.w = w or world()
        self.otu, self.weight, self.kind, self.L, self.node, self.hund = [], [], [], [], [], []
        self.seed = {}

    def add(self, k, weight, name, hund=None, kind=UNCLASSIFIED, n=1, seed=False):
        for _ in range(n):
            if seed or k not in self.seed:
                self.seed[k] = len(self.otu)
            v = self.w.node(name) if name else 0
            l = int(self.w.depth[v]) if name else 0
            h = list(hund) if hund is not None else [90] * l
            assert len(h) == l
            self.otu.append(k)
            self.weight.append(weight)
            self.kind.append(CLASSIFIED if name else kind)
            self.L.append(l)
            self.node.append(v)
            self.hund.append(h + [0] * (MAX_DEPTH - l))
        return self

    def arrays(self, order=None):
        """(otu, weight, seed), Lineages -- the rows in the given order (a permutation of the ranks: the seeds follow their rows)"""
        n = len(self.otu)
        order = np.arange(n) if order is None else np.asarray(order)
        inv = np.empty(n, np.int64)
        inv[order] = np.arange(n)
        n_otus = max(self.otu) + 1 if n else 0
        assert sorted(self.seed) == list(range(n_otus))
        seed = np.array([inv[self.seed[k]] for k in range(n_otus)], np.uint32)
        lin = rx.Lineages(np.array(self.kind, np.uint8)[order], np.array(self.L, np.uint8)[order], np.array(self.node, np.uint32)[order],
                          np.array(self.hund, np.uint8).reshape(n, MAX_DEPTH)[order])
        return (np.array(self.otu, np.uint32)[order], np.array(self.weight, np.uint64)[order], seed), lin


def path_of(parent, node, l):
    out = []
    for _ in range(l):
        out.append(int(node))
        node = parent[node]
    return out[::-1]


def brute(parent, otus, lin, agree=51):
    """the definition: per OTU dicts of clade and conf over all members' paths, then the descent to the child that qualifies"""
    otu, weight, seed = otus
    n_otus = len(seed)
    stride = max(1, int(lin.L.max()) if len(lin.L) else 1)
    out = dict(sizes=np.zeros(n_otus, np.uint64), members=np.zeros(n_otus, np.uint64), classified=np.zeros(n_otus, np.uint64), depth=np.zeros(n_otus, np.uint32),
               node=np.zeros(n_otus, np.uint32), seed_rel=np.zeros(n_otus, np.uint8), clade=np.zeros((n_otus, stride), np.uint64), conf=np.zeros((n_otus, stride), np.uint64))
    paths = [path_of(parent, lin.node[r], int(lin.L[r])) for r in range(len(otu))]
    clade = [dict() for _ in range(n_otus)]
    conf = [dict() for _ in range(n_otus)]
    size = [0] * n_otus
    for r, k in enumerate(otu):
        k, w = int(k), int(weight[r])
        size[k] += w
        out["members"][k] += 1
        if lin.kind[r] == CLASSIFIED:
            out["classified"][k] += w
        for d, v in enumerate(paths[r]):
            clade[k][v] = clade[k].get(v, 0) + w
            conf[k][v] = conf[k].get(v, 0) + w * int(lin.hund[r][d])
    for k in range(n_otus):
        out["sizes"][k] = size[k]
        cur, cons = 0, []
        while True:
            ok = [v for v in clade[k] if parent[v] == cur and clade[k][v] * 100 >= agree * size[k]]
            assert len(ok) <= 1, "two children qualify: impossible above 50 percent"
            if not ok:
                break
            cur = ok[0]
            out["clade"][k, len(cons)] = clade[k][cur]
            out["conf"][k, len(cons)] = conf[k][cur]
            cons.append(cur)
        out["depth"][k], out["node"][k] = len(cons), cur
        sp = paths[int(seed[k])]
        m = min(len(sp), len(cons))
        out["seed_rel"][k] = 3 if sp[:m] != cons[:m] else (0 if len(sp) == len(cons) else (1 if len(sp) > len(cons) else 2))
    return out


def assert_tax(got, want, what=""):
    """an OtuTaxonomy against brute()'s dict or another OtuTaxonomy, field by field, exactly"""
    for f in FIELDS:
        a, b = getattr(got, f), (want[f] if isinstance(want, dict) else getattr(want, f))
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {f} differs at {np.argwhere(a != b)[:5].tolist() if a.shape == b.shape else (a.shape, b.shape)}"


def fill(case, rng, k, n, names=None, weights=(1, 4), deep=False):
    """n rows of OTU k on random nodes (of `names`, or of the whole tree; one in eight with L = 0 of either kind), hundredths 50 .. 100"""
    w = case.w
    names = names or ([x for x in w.names if deep or w.depth[w.node(x)] <= 4])
    for _ in range(n):
        if rng.integers(8) == 0:
            case.add(k, int(rng.integers(*weights)), None, kind=int(rng.integers(2)))
        else:
            name = names[int(rng.integers(len(names)))]
            case.add(k, int(rng.integers(*weights)), name, hund=rng.integers(50, 101, int(w.depth[w.node(name)])).tolist())
    return case


def random_world(seed=23, n_otus=700, big=(300, 700, 1100)):
    """about 5 000 rows in 700 OTUs of geometric sizes, three of them above 256 members, over a tree of about 200 nodes"""
    rng = np.random.default_rng(seed)
    lineages = sorted({f"p{a},c{a}{b},o{a}{b}{c},g{a}{b}{c}{d}" for a in range(3) for b in range(3) for c in range(4) for d in range(4)})
    w = World(lineages + [f"p{a},c{a}{b},z{a}{b}" for a in range(3) for b in range(2)])
    case = Case(w)
    sizes = np.minimum(rng.geometric(0.25, n_otus), 200)
    for i, b in enumerate(big):
        sizes[5 + 90 * i] = b
    for k in range(n_otus):
        # most OTUs sit in one genus' neighbourhood, so that walks of every depth occur; some are spread over the tree
        if rng.integers(4):
            g = lineages[int(rng.integers(len(lineages)))].split(",")
            near = [",".join(g[:d]) for d in range(1, 5)] * 3 + [x for x in w.names if x.startswith(g[0] + "," + g[1])]
            fill(case, rng, k, int(sizes[k]), names=near, weights=(1, 50))
        else:
            fill(case, rng, k, int(sizes[k]), weights=(1, 50))
    return case


# ---- the crafted cases: name -> (Case, agree, {field: expected array or None}); built once, never changed

def _singletons(n):
    rng = np.random.default_rng(n)
    c = Case()
    for k in range(n):
        fill(c, rng, k, 1)
    return c


def _sized(*sizes):
    rng = np.random.default_rng(sum(sizes))
    c = Case()
    for k, n in enumerate(sizes):
        fill(c, rng, k, n, names=["A,B,C", "A,B,D", "A,E,F", "A,E,G,H", "J,K,L", "A,B", "A"])
    return c


def _stops_at_different_levels():
    """one packed wave: OTUs whose walks end at depth 0, 1, 2, 3, 4 and RTX_MAX_DEPTH"""
    c = Case()
    c.add(0, 1, "A,B,C").add(0, 1, "J,K,L")                        # an even split at level 0
    c.add(1, 1, "A,B,C").add(1, 1, "A,E,F")                        # A, then an even split
    c.add(2, 2, "A,E,F").add(2, 1, "A,E,G,H").add(2, 1, "A,B,C")   # A (4/4), E (3/4), then F with 2/4: stops
    c.add(3, 3, "A,E,F").add(3, 1, "A,E,G,H")                      # A, E, F (3/4)
    c.add(4, 5, "A,E,G,H").add(4, 1, "A,E,G,I")                    # four levels
    c.add(5, 1, LINEAGES[-1]).add(5, 1, ",".join(LINEAGES[-1].split(",")[:20]))  # the chain: 32 levels need 51 %, the shorter row drops out at 20
    c.add(6, 7, LINEAGES[-1])
    return c, np.array([0, 1, 2, 3, 4, 20, MAX_DEPTH], np.uint32)


def _threshold(agree, short):
    """S = 100 reads: `agree` of them on A,B,C, the rest on A,E,F: B and C hold exactly agree x S / 100; `short`: one read fewer there, the walk stops at A"""
    c = Case()
    c.add(0, 1, "A,B,C", n=agree - short).add(0, 1, "A,E,F", n=100 - agree + short)
    return c


def _threshold_packed(agree, short):
    """the same in a packed wave: 20 members, S = 100 as weights -- ten rows on A,B,C that weigh `agree` together, ten on A,E,F with the rest
    (P = 100: all twenty on A,B,C); `short`: one read moves from the last row on A,B,C to a row on A,E,F"""
    def split(total, n):
        return [total // n + (i < total % n) for i in range(n)]
    c = Case()
    here = split(agree, 10 if agree < 100 else 19)
    there = split(100 - agree, 10) if agree < 100 else [0]
    if short:
        here[-1] -= 1
        there[-1] += 1
    for w in here:
        c.add(0, w, "A,B,C")
    for w in there:
        if w:
            c.add(0, w, "A,E,F")
    return c


def _l_ends_above():
    """10 reads on A,B,C; 6 of them with L = 3, 4 with L = 2: A,B holds 10/10 and C only 6/10 -- 60 % passes 51 and fails 61"""
    return Case().add(0, 1, "A,B,C", n=6).add(0, 1, "A,B", n=4)


def _l_zero():
    """4 reads on A,B,C and 4 of L = 0 (two of either kind): they count in S alone, 50 % stops the walk at the root"""
    return Case().add(0, 1, "A,B,C", n=4).add(0, 1, None, kind=UNCLASSIFIED, n=2).add(0, 1, None, kind=UNCLASSIFIABLE, n=2)


def _spread(w):
    """300 light members spread over many nodes; names cycle through the tree's shallow nodes except those under J"""
    return [x for x in w.names if not x.startswith("J") and w.depth[w.node(x)] <= 4]


def _heavy_one():
    """the majority's weight in one member (301) against 300 dissenters of weight 1 on many nodes"""
    c = Case()
    other = _spread(c.w)
    for i in range(150):
        c.add(0, 1, other[i % len(other)])
    c.add(0, 301, "J,K,L")
    for i in range(150):
        c.add(0, 1, other[(i * 7) % len(other)])
    return c


def _light_many():
    """the same weight spread over 300 members of weight 1 on J,K,M,N against one dissenter of 299 on A,B,C: 300 of 599 is 50.08 %: stops"""
    c = Case().add(0, 299, "A,B,C", seed=True)
    c.add(0, 1, "J,K,M,N", n=300)
    return c


def _light_many_wins():
    """... and against one of 288: 300 of 588 is 51.02 %"""
    return Case().add(0, 288, "A,B,C", seed=True).add(0, 1, "J,K,M,N", n=300)


def _no_majority():
    """five top-level nodes, none with half of the weight"""
    c = Case()
    for i, name in enumerate(["A,B,C", "J,K,L", "Q,R,S", "X,Y,Z", "c0,c1"] * 30):
        c.add(0, 1 + i % 3, name)
    return c


def _wide_sums():
    """weights of 2^40: clade and conf pass 2^32 (and 100 x clade passes 2^46)"""
    c = Case()
    c.add(0, 1 << 40, "A,E,G,H", hund=[100, 99, 98, 97], n=3).add(0, 1 << 40, "A,E,G,I", hund=[100, 100, 100, 51]).add(0, (1 << 40) + 1, "A,B,C")
    for i in range(70):
        c.add(1, (1 << 40) + i, "J,K,M,N" if i % 4 else "J,K,L", hund=[100] * (4 if i % 4 else 3))
    return c


def _seed_rel():
    """all four relations, in the packed path; the same four with 70 members each, in a workgroup"""
    c = Case()
    for base, pad in ((0, 0), (4, 66)):
        c.add(base + 0, 1, "A,B,C", seed=True).add(base + 0, 1, "A,B,C", n=2 + pad)                       # 0: equal
        c.add(base + 1, 1, "A,B,C", seed=True).add(base + 1, 1, "A,B,D").add(base + 1, 1, "A,B", n=2 + pad)  # 1: the consensus A,B is a prefix of the seed's
        c.add(base + 2, 1, "A,B", seed=True).add(base + 2, 1, "A,B,C", n=3 + pad)                         # 2: the seed's is a prefix of the consensus
        c.add(base + 3, 1, "A,E,F", seed=True).add(base + 3, 1, "A,B,C", n=3 + pad)                       # 3: they part at level 1
    return c, np.array([0, 1, 2, 3] * 2, np.uint8)


PERMUTED = ("heavy_one", "heavy_one_50", "light_many", "light_many_wins", "no_majority")


@lru_cache(maxsize=None)
def cases():
    """name -> (Case, agree, expected fields)"""
    out = {}
    out["singletons_64"] = (_singletons(64), 51, {})
    out["singletons_65"] = (_singletons(65), 51, {})
    out["sizes_63_2"] = (_sized(63, 2), 51, {})
    out["sizes_64_65"] = (_sized(64, 65), 51, {})
    out["sizes_256_257_1025"] = (_sized(256, 257, 1025), 51, {})
    c, depth = _stops_at_different_levels()
    out["stops"] = (c, 51, dict(depth=depth))
    for agree in (51, 100):
        out[f"threshold_{agree}"] = (_threshold(agree, 0), agree, dict(depth=np.array([3], np.uint32), clade=[agree]))
        out[f"threshold_{agree}_short"] = (_threshold(agree, 1), agree, dict(depth=np.array([1], np.uint32)))
        out[f"threshold_{agree}_packed"] = (_threshold_packed(agree, 0), agree, dict(depth=np.array([3], np.uint32), clade=[agree], sizes=np.array([100], np.uint64)))
        out[f"threshold_{agree}_packed_short"] = (_threshold_packed(agree, 1), agree, dict(depth=np.array([1], np.uint32), sizes=np.array([100], np.uint64)))
    out["even_split"] = (Case().add(0, 3, "A,B,C").add(0, 3, "J,K,L"), 51, dict(depth=np.array([0], np.uint32), node=np.array([0], np.uint32)))
    out["splits_at_level_1"] = (Case().add(0, 2, "A,B,C").add(0, 2, "A,E,F").add(0, 1, "J,K,L"), 51, dict(depth=np.array([1], np.uint32)))
    out["l_ends_above_51"] = (_l_ends_above(), 51, dict(depth=np.array([3], np.uint32)))
    out["l_ends_above_61"] = (_l_ends_above(), 61, dict(depth=np.array([2], np.uint32)))
    out["l_zero"] = (_l_zero(), 51, dict(depth=np.array([0], np.uint32), classified=np.array([4], np.uint64), sizes=np.array([8], np.uint64)))
    out["heavy_one"] = (_heavy_one(), 51, dict(depth=np.array([0], np.uint32)))          # 301 of 601 is 50.08 %
    out["heavy_one_50"] = (_heavy_one().add(0, 12, "J,K,L"), 51, dict(depth=np.array([3], np.uint32)))  # 313 of 613 is 51.06 %
    out["light_many"] = (_light_many(), 51, dict(depth=np.array([0], np.uint32)))
    out["light_many_wins"] = (_light_many_wins(), 51, dict(depth=np.array([4], np.uint32), seed_rel=np.array([3], np.uint8)))
    out["no_majority"] = (_no_majority(), 51, dict(depth=np.array([0], np.uint32)))
    out["wide_sums"] = (_wide_sums(), 51, {})
    c, rel = _seed_rel()
    out["seed_rel"] = (c, 51, dict(seed_rel=rel))
    return out


def check_expected(name, got, expected):
    for f, want in expected.items():
        a = getattr(got, f) if not isinstance(got, dict) else got[f]
        if f == "clade":                      # the clade of the last level of OTU 0
            assert int(a[0, int((got["depth"] if isinstance(got, dict) else got.depth)[0]) - 1]) == want[0], (name, f)
        else:
            assert np.array_equal(a, want), (name, f, a.tolist(), np.asarray(want).tolist())


FIXED_PERMUTATION_SEED = 41


def permutation(n):
    return np.random.default_rng(FIXED_PERMUTATION_SEED).permutation(n)


def refusals():
    """name -> (otus, lineages, agree, parent or None): every refusal of the definition, one at a time"""
    w = world()

    def base():
        c = Case().add(0, 2, "A,B,C").add(0, 1, "A,E,F").add(1, 1, None)
        (otu, weight, seed), lin = c.arrays()
        return [otu, weight, seed], lin

    out = {}
    for agree in (50, 101, 1):
        o, l = base()
        out[f"agree_{agree}"] = (o, l, agree, None)
    o, l = base(); l.node[0] = w.n_nodes; out["node_out_of_range"] = (o, l, 51, None)
    o, l = base(); l.L[0] = 4; out["l_above_the_node_s_depth"] = (o, l, 51, None)
    o, l = base(); l.L[0] = 2; out["l_below_the_node_s_depth"] = (o, l, 51, None)
    o, l = base(); l.L[0] = MAX_DEPTH + 1; out["l_above_max_depth"] = (o, l, 51, None)
    o, l = base(); o[0][1] = 2; out["otu_out_of_range"] = (o, l, 51, None)
    o, l = base(); o[2][1] = 3; out["seed_out_of_range"] = (o, l, 51, None)
    o, l = base(); o[0][2] = 0; out["otu_without_a_row"] = (o, l, 51, None)
    o, l = base(); o[1][0] = 0; out["weight_zero"] = (o, l, 51, None)
    o, l = base(); o[1][:] = [1 << 57, 1 << 57, 1 << 57]; out["weights_overflow"] = (o, l, 51, None)
    o, l = base(); l.kind[2] = 3; out["kind_unknown"] = (o, l, 51, None)
    o, l = base(); l.kind[0] = UNCLASSIFIED; out["l_on_an_unclassified_row"] = (o, l, 51, None)
    o, l = base(); l.kind[2] = CLASSIFIED; out["classified_without_levels"] = (o, l, 51, None)
    o, l = base(); l.hund[0, 1] = 101; out["hundredths_above_100"] = (o, l, 51, None)
    o, l = base(); p = w.parent.copy(); p[3] = 5; out["parent_not_below"] = (o, l, 51, p)
    return out

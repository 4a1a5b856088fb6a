"""The semantics of the sample demultiplexing (include/raxtax_hip.h, rtx_demux_*) restated in numpy, and the tag lists and reads the
demultiplexing tests share.  Nothing here is packed and nothing comes from the library: per end a loop over the offsets and over the tags
(the tags of one length side by side in an array), the distance of a placement counted base by base.

  bytes      two bytes match when both are codes (1 .. 15) and share a bit.
  placement  a tag of m codes at offset s (0 <= s <= max_offset, s + m <= len) covers x[s .. s + m); d = its positions that do not match.
             A 3' tag is the 5' problem of the reversed tag in the reversed read.
  one end    d* = the least d over tags and admissible offsets; found iff d* <= max_mismatches; ambiguous iff found and two different tags
             reach d*; else the tag that reaches d*, at its least offset.
  verdict    3 either end ambiguous; 1 the list has 5' tags and none was found; 2 the same for 3'; 4 the pair is not in the table; 0.
  per read   sample (0xFFFFFFFF unless the verdict is 0), lo = s5 + m5 or 0, hi = len - (s3 + m3) or len, hi = max(hi, lo),
             hit = tag5 | tag3 << 16 (0xFFFF: none), info = verdict | d5 << 8 | d3 << 16 | s5 << 24 | s3 << 28."""
import numpy as np

NO_TAG, NONE = 0xFFFF, 0xFFFFFFFF
OK, NO_TAG5, NO_TAG3, AMBIGUOUS, UNKNOWN_PAIR = range(5)
A, Cc, G, T, W, Y, N = 1, 2, 4, 8, 9, 10, 15


def concat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    if len(reads):
        off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    flat = np.concatenate([np.asarray(r, np.uint8) for r in reads]) if len(reads) and off[-1] else np.zeros(0, np.uint8)
    return flat, off


class End:
    """The tags of one end, as searched (a 3' tag reversed), grouped by length."""

    def __init__(self, tags, end):
        self.places = [i for i, (_, e) in enumerate(tags) if e == end]
        self.length = {i: len(tags[i][0]) for i in self.places}
        self.groups = {}
        for i in self.places:
            c = np.asarray(tags[i][0], np.uint8)
            self.groups.setdefault(len(c), []).append((i, c[::-1] if end else c))
        self.groups = {m: (np.array([i for i, _ in g]), np.stack([c for _, c in g])) for m, g in self.groups.items()}

    def search(self, x, max_mismatches, max_offset):
        """(d*, tag, offset, found, ambiguous) in x (the read, reversed for the 3' end); d* = 255 when no placement is admissible."""
        x = np.where(x > 15, 0, x).astype(np.uint8)
        tag_d, tag_s = {}, {}                          # per tag: its least distance, and the least offset that has it
        for m, (idx, codes) in self.groups.items():
            least = np.full(len(idx), 255, np.int64)
            at = np.zeros(len(idx), np.int64)
            for s in range(max_offset + 1):
                if s + m > len(x):
                    continue
                d = m - ((codes & x[s:s + m]) != 0).sum(axis=1)
                closer = d < least
                least[closer] = d[closer]
                at[closer] = s
            for i, d, s in zip(idx[least < 255], least[least < 255], at[least < 255]):
                tag_d[int(i)], tag_s[int(i)] = int(d), int(s)
        if not tag_d:
            return 255, None, 0, False, False
        dstar = min(tag_d.values())
        reach = sorted(i for i, d in tag_d.items() if d == dstar)
        found = dstar <= max_mismatches
        return dstar, reach[0], tag_s[reach[0]], found, found and len(reach) > 1


def demux_ref(tags, pairs, max_mismatches, max_offset, reads):
    """(sample, lo, hi, hit, info, d5*, d3*) of the reads, one array each.  tags: (codes, end); pairs: (tag5 or None, tag3 or None, sample)."""
    e5, e3 = End(tags, 0), End(tags, 1)
    table = {(NO_TAG if a is None else a, NO_TAG if b is None else b): s for a, b, s in pairs}
    out = [[] for _ in range(7)]
    for x in reads:
        x = np.asarray(x, np.uint8)
        n = len(x)
        d5, t5, s5, f5, a5 = e5.search(x, max_mismatches, max_offset) if e5.places else (255, None, 0, False, False)
        d3, t3, s3, f3, a3 = e3.search(x[::-1], max_mismatches, max_offset) if e3.places else (255, None, 0, False, False)
        has5, has3 = f5 and not a5, f3 and not a3
        k5, k3 = (t5 if has5 else NO_TAG), (t3 if has3 else NO_TAG)
        sample = NONE
        if a5 or a3:
            verdict = AMBIGUOUS
        elif e5.places and not f5:
            verdict = NO_TAG5
        elif e3.places and not f3:
            verdict = NO_TAG3
        elif (k5, k3) not in table:
            verdict = UNKNOWN_PAIR
        else:
            verdict, sample = OK, table[(k5, k3)]
        lo = s5 + e5.length[t5] if has5 else 0
        hi = n - (s3 + e3.length[t3]) if has3 else n
        hi = max(hi, lo)
        info = verdict | (d5 if has5 else 0) << 8 | (d3 if has3 else 0) << 16 | (s5 if has5 else 0) << 24 | (s3 if has3 else 0) << 28
        for o, v in zip(out, (sample, lo, hi, k5 | k3 << 16, info, d5, d3)):
            o.append(v)
    return tuple(np.array(o, np.uint32) for o in out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tag lists
# ---------------------------------------------------------------------------------------------------------------------------------
def random_seq(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


def other(b):
    return {1: 2, 2: 4, 4: 8, 8: 1}[int(b)]


def spaced_tags(rng, count, m, min_dist=3):
    """`count` tags of m bases, pairwise at least min_dist apart (rejection sampling)."""
    kept = np.zeros((0, m), np.uint8)
    while len(kept) < count:
        c = random_seq(rng, m)
        if len(kept) == 0 or ((kept != c).sum(axis=1) >= min_dist).all():
            kept = np.vstack([kept, c])
    return [kept[i] for i in range(count)]


class Lists:
    """The lists of the tests: (tags, pairs) by name.  `l96`: 96 tags of 20 bases per end (`l1`, `l2`: its first ones), `l1024`: 1024 of 12 per
    end, pairwise at least 3 apart, `mixed`: 1, 8, 16, 17 and 32 codes per end with degenerate codes, `only5` / `only3`: one end of l96."""

    def __init__(self):
        rng = np.random.default_rng(77)
        self.f96, self.r96 = spaced_tags(rng, 96, 20), spaced_tags(rng, 96, 20)
        for t, positions in ((self.f96, (1, 6, 12, 18)), (self.r96, (0, 5, 11, 19))):   # two tags of either end four substitutions apart
            a, b = (7, 8) if t is self.f96 else (9, 10)
            t[b] = t[a].copy()
            for p in positions:
                t[b][p] = other(t[b][p])
        self.f1024, self.r1024 = spaced_tags(rng, 1024, 12), spaced_tags(rng, 1024, 12)
        self.fmix = [random_seq(rng, m) for m in (1, 8, 16, 17, 32)]
        self.rmix = [random_seq(rng, m) for m in (32, 17, 16, 8, 1)]
        self.fmix_inst, self.rmix_inst = [t.copy() for t in self.fmix], [t.copy() for t in self.rmix]   # an instance of each degenerate tag
        self.fmix[2][[0, 15]] = [self.fmix[2][0] | T | A, N]
        self.fmix[3][16] |= Cc | T
        self.fmix[4][[15, 16, 31]] = [N, self.fmix[4][16] | G, self.fmix[4][31] | A]
        self.rmix[0][[0, 16]] = [N, self.rmix[0][16] | A | T]
        self.rmix[1][0] |= G
        both = lambda f, r: [(c, 0) for c in f] + [(c, 1) for c in r]
        n = 96
        self.lists = {
            "l1": (both(self.f96[:1], self.r96[:1]), [(0, 1, 0)]),
            "l2": (both(self.f96[:2], self.r96[:2]), [(0, 2, 0), (1, 3, 1), (0, 3, 2)]),
            # samples 0 .. 4 (4 gets no pair of its own tags 90 .. 95: those pairs are missing); (0, 1) is a pair, (0, 2) is none
            "l96": (both(self.f96, self.r96), [(i, n + i, i % 4) for i in range(90)] + [(0, n + 1, 4)]),
            "l1024": (both(self.f1024, self.r1024), [(i, 1024 + i, i % 96) for i in range(1024)]),
            # interleaved: the place in the list is not the place within the end
            "mixed": ([t for pair in zip([(c, 0) for c in self.fmix], [(c, 1) for c in self.rmix]) for t in pair], [(2 * i, 2 * i + 1, i) for i in range(5)]),
            "only5": ([(c, 0) for c in self.f96], [(i, None, i % 5) for i in range(96)]),
            "only3": ([(c, 1) for c in self.r96], [(None, i, i % 5) for i in range(96)]),
        }

    def reads(self):
        """The 257 reads (see tests/test_gpu_demux.py for what the expectation is checked to contain)."""
        rng = np.random.default_rng(78)
        f, r = self.f96, self.r96
        amp = lambda n=300: random_seq(rng, n)
        cat = lambda *p: np.concatenate([np.asarray(x, np.uint8) for x in p])

        def subst(t, positions):
            t = t.copy()
            for p in positions:
                t[p] = other(t[p])
            return t

        reads = [cat(f[0], amp(), r[0]),                                # n = 1 is this one
                 np.zeros(0, np.uint8), amp(1), amp(19),                # empty, shorter than a tag
                 f[0].copy(), r[0].copy(),                              # equal to a tag
                 cat(f[0][:12], r[0][4:]), cat(f[0], r[0][10:]),        # shorter than m5 + m3: the cuts overlap
                 cat(f[0], r[0]),                                       # a bare tag pair: nothing is left
                 cat(f[0], amp(5000 - 40), r[0]),
                 cat(f[0], amp(), r[1]),                                # a pair of its own
                 cat(f[0], amp(), r[2]),                                # found, but no pair
                 cat(f[93], amp(), r[93]),
                 cat(f[0], amp()), cat(amp(), r[0])]                    # one end only
        first_mid_last = [[], [0], [10], [19], [0, 10], [0, 19], [0, 10, 19], [1, 10, 18], [0, 1, 10, 19], [0, 9, 10, 19]]   # 0 .. 4 substitutions
        for pos in first_mid_last:
            reads.append(cat(subst(f[3], pos), amp(), r[3]))
            reads.append(cat(f[4], amp(200), subst(r[4], pos)))
        for sp in (0, 1, 7, 15, 16):                                    # spacers (16: one more than any max_offset)
            reads.append(cat(amp(sp), f[5], amp(), r[5], amp(sp)))
            reads.append(cat(amp(sp), subst(f[6], [2]), amp(150), subst(r[6], [17, 3]), amp(15 - min(sp, 15))))
        # two tags tie: f[8] is f[7] with four substitutions (r[10] and r[9] likewise), the read's tag has two of them
        reads.append(cat(tie_of(f[7], f[8]), amp(), r[7]))
        reads.append(cat(f[7], amp(), tie_of(r[9], r[10])))
        for byte in (0, 15, 0x20, 200):                                 # bytes that are no code and N, inside and behind the tag
            s = cat(f[11], amp(), r[11])
            s[[4, 22, len(s) - 6, len(s) - 25]] = byte
            reads.append(s)
            s = cat(amp(2), f[12], amp(), r[12], amp(3))
            s[[0, 2 + 19, len(s) - 1, len(s) - 4]] = byte
            reads.append(s)
        for i in range(5):                                              # the mixed list: its tags at their lengths, degenerate codes instantiated
            reads.append(cat(self.fmix_inst[i], amp(), self.rmix_inst[i]))
            reads.append(cat(amp(1), subst(self.fmix_inst[i], [len(self.fmix_inst[i]) - 1]), amp(64), self.rmix_inst[i], amp(2)))
        reads.append(cat(self.fmix_inst[4][:20], self.rmix_inst[0][10:]))   # shorter than 32 + 32
        while len(reads) < 257:                                         # the bulk: random amplicons with tags of one of the lists
            k = len(reads)
            if k % 3 == 0:
                i = int(rng.integers(0, 96))
                a, b = f[i], r[i if k % 4 else int(rng.integers(0, 96))]
            elif k % 3 == 1:
                i = int(rng.integers(0, 1024))
                a, b = self.f1024[i], self.r1024[i if k % 4 else int(rng.integers(0, 1024))]
            else:
                i = int(rng.integers(0, 5))
                a, b = self.fmix_inst[i], self.rmix_inst[i]
            a, b = a.copy(), b.copy()
            for s in (a, b):
                for _ in range(int(rng.integers(0, 3))):
                    s[int(rng.integers(0, len(s)))] = int(rng.choice([1, 2, 4, 8, 15, 0x20]))
            parts = [amp(int(rng.integers(0, 4)))] + [a] * (k % 7 != 0) + [amp(int(rng.integers(60, 400)))] + [b] * (k % 5 != 0) + [amp(int(rng.integers(0, 4)))]
            reads.append(cat(*parts))
        assert len(reads) == 257
        return reads


def tie_of(a, b):
    """A tag as far from a as from b (both of one length)."""
    diff = np.nonzero(a != b)[0]
    t = a.copy()
    t[diff[:len(diff) // 2]] = b[diff[:len(diff) // 2]]
    if len(diff) % 2:
        t[diff[-1]] = next(x for x in (1, 2, 4, 8) if x not in (int(a[diff[-1]]), int(b[diff[-1]])))
    return t


_SHARED = {}


def shared():
    """(Lists, reads): built once per process."""
    if not _SHARED:
        lists = Lists()
        _SHARED["v"] = (lists, lists.reads())
    return _SHARED["v"]


_EXPECTED = {}


def expected(name, max_mismatches, max_offset):
    """demux_ref of the shared reads against list `name`, computed once per process and left unchanged."""
    key = (name, max_mismatches, max_offset)
    if key not in _EXPECTED:
        lists, reads = shared()
        tags, pairs = lists.lists[name]
        _EXPECTED[key] = demux_ref(tags, pairs, max_mismatches, max_offset, reads)
        for a in _EXPECTED[key]:
            a.setflags(write=False)
    return _EXPECTED[key]

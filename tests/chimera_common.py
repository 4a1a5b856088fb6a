"""The chimera check restated in numpy, from the definition in include/raxtax_hip.h and nothing else: sets of 8-mers per reference (an
inverted index over the reference sequences), one 0/1 row per reference over the read's windows, cumulative sums at the boundaries.  It
shares no code with the library; the tests hold rtx_chimera_read, the x86 emulator and the device against it field by field.

The references must come in the order the device numbers them (the tree's sorted order: Tree.original_index)."""
from __future__ import annotations

import numpy as np

NO_REF = 0xFFFFFFFF
OK, NO_KMER, TOO_LONG = 0, 1, 2
MAX_QUERY = 4096
FIELDS = ("status", "n_valid", "single", "parent", "seg", "pos", "left", "parent_a", "right", "parent_b", "delta", "flag")
_TWO = np.full(256, 255, np.uint8)
_TWO[[1, 2, 4, 8]] = [0, 1, 2, 3]


def window_codes(seq: np.ndarray):
    """(code, valid) of every window of eight bases: the 16-bit code with the first base on top, valid where all eight are 1, 2, 4 or 8."""
    seq = np.asarray(seq, np.uint8)
    n = max(0, len(seq) - 7)
    code = np.zeros(n, np.int64)
    valid = np.ones(n, bool)
    if n == 0:
        return code, valid
    two = _TWO[seq]
    for j in range(8):
        t = two[j:j + n]
        valid &= t != 255
        code = (code << 2) | (t & 3)
    return code, valid


class Restatement:
    def __init__(self, ref_bases: np.ndarray, ref_off: np.ndarray):
        ref_off = np.asarray(ref_off, np.int64)
        self.n_refs = len(ref_off) - 1
        keys = []
        for r in range(self.n_refs):   # the SET of 8-mers of every reference
            code, valid = window_codes(ref_bases[ref_off[r]:ref_off[r + 1]])
            keys.append(np.unique(code[valid]) * self.n_refs + r)
        keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
        self.post_ref = keys % max(self.n_refs, 1)
        self.post_off = np.searchsorted(keys // max(self.n_refs, 1), np.arange(65537))

    def record(self, read: np.ndarray, segments: int = 16, mindelta: int = 24) -> dict:
        S = int(segments)
        rec = dict(status=OK, n_valid=0, single=0, parent=NO_REF, seg=0, pos=0, left=0, parent_a=NO_REF, right=0, parent_b=NO_REF, delta=0, flag=0)
        if len(read) > MAX_QUERY:
            rec["status"] = TOO_LONG
            return rec
        code, valid = window_codes(read)
        n_pos = len(code)
        if not valid.any():
            rec["status"] = NO_KMER
            return rec
        b = np.array([s * n_pos // S for s in range(S + 1)], np.int64)
        idx = np.nonzero(valid)[0]
        seg_of = np.searchsorted(b[1:], idx, side="right")          # window i lies in segment s: b[s] <= i < b[s + 1]
        lo, hi = self.post_off[code[idx]], self.post_off[code[idx] + 1]
        refs = np.concatenate([self.post_ref[a:z] for a, z in zip(lo, hi)]) if len(idx) else np.zeros(0, np.int64)
        segs = np.repeat(seg_of, hi - lo)
        cnt = np.bincount(refs * S + segs, minlength=self.n_refs * S).reshape(self.n_refs, S)   # x_r summed per segment
        P = np.concatenate([np.zeros((self.n_refs, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)
        T = P[:, S]
        Suf = T[:, None] - P
        two = np.array([P[:, s].max() + Suf[:, s].max() for s in range(1, S)])
        seg = 1 + int(np.argmax(two))                               # the lowest s with the largest two[s]
        left, right, single = int(P[:, seg].max()), int(Suf[:, seg].max()), int(T.max())
        rec.update(n_valid=int(valid.sum()), single=single, parent=int(np.argmax(T)) if single else NO_REF, seg=seg, pos=int(b[seg]), left=left,
                   parent_a=int(np.argmax(P[:, seg])) if left else NO_REF, right=right, parent_b=int(np.argmax(Suf[:, seg])) if right else NO_REF,
                   delta=int(two[seg - 1]) - single)
        assert rec["delta"] >= 0
        rec["flag"] = int(rec["delta"] >= mindelta)
        return rec


def as_tuple(rec) -> tuple:
    """A record -- the restatement's dict or a row of the library's structured array -- as twelve ints."""
    return tuple(int(rec[f]) for f in FIELDS)


def tree_order(db, tree):
    """(bases, offsets) of a synthetic database in the order the tree numbers its references."""
    orig = np.asarray(tree.original_index(), np.int64)
    seqs = [db.seq(int(i)) for i in orig]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off


def substitute(rng, seq: np.ndarray, rate: float) -> np.ndarray:
    out = seq.copy()
    hit = rng.random(len(seq)) < rate
    out[hit] = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    return out


def planted_chimeras(db, n: int = 300, seed: int = 5, lo: int = 100, hi: int = 558, rate: float = 0.01):
    """Chimeras of two random references of a synthetic database: the head of one up to a breakpoint in [lo, hi], the tail of the other,
    then substitutions at `rate`.  Returns (sequences, (a, b, breakpoint) per read)."""
    rng = np.random.default_rng(seed)
    seqs, meta = [], []
    for _ in range(n):
        a, b = (int(x) for x in rng.integers(0, db.n, 2))
        bp = int(rng.integers(lo, hi + 1))
        seqs.append(substitute(rng, np.concatenate([db.seq(a)[:bp], db.seq(b)[bp:]]), rate))
        meta.append((a, b, bp))
    return seqs, meta


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if len(seqs) else np.zeros(0, np.uint8)), off

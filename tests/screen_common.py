"""The contaminant screen restated in plain Python over a dict of canonical values (include/raxtax_hip.h has the definition): no table, no
probing, no rolling words -- every window's value is a sum over its 16 bases.  The tests hold rx.screen_read, the x86 emulation of the
device's steps and the device itself against it.  home_slot() is the table's hash, used only to aim test inputs at chains."""
import ctypes as C
import random

import numpy as np

import raxtax_amd as rx

K = 16
NONE = 0xFFFFFFFF
_TWO = np.full(256, -1, np.int64)
for _code, _two in ((1, 0), (2, 1), (4, 2), (8, 3)):
    _TWO[_code] = _two
COMP = np.arange(256, dtype=np.uint8)          # the complement of a 4-bit code: its bits reversed (A 1 <-> T 8, C 2 <-> G 4)
for _c in range(16):
    COMP[_c] = ((_c & 1) << 3) | ((_c & 2) << 1) | ((_c & 4) >> 1) | ((_c & 8) >> 3)


def revcomp(codes):
    return COMP[np.asarray(codes, np.uint8)[::-1]].copy()


def rc_value(w):
    """The value of the reverse complement of the 16-mer with value w: its base j is 3 - base 15 - j."""
    out = 0
    for j in range(K):
        out |= (3 - ((w >> (2 * j)) & 3)) << (2 * (K - 1 - j))
    return out


def canonical(w):
    return min(w, rc_value(w))


def kmer_codes(w):
    """The 16 4-bit codes of the 16-mer with value w (first base in the most significant bits)."""
    return np.array([1 << ((w >> (2 * (K - 1 - j))) & 3) for j in range(K)], np.uint8)


def windows_of(codes):
    """(positions, canonical values) of the valid windows of a code array."""
    codes = np.asarray(codes, np.uint8)
    n = len(codes) - K + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    two = _TWO[codes]
    bad = np.concatenate(([0], np.cumsum(two < 0)))
    valid = (bad[K:] - bad[:-K]) == 0
    t = np.where(two < 0, 0, two)
    w = np.zeros(n, np.int64)
    r = np.zeros(n, np.int64)
    for j in range(K):
        w |= t[j:j + n] << (2 * (K - 1 - j))
        r |= (3 - t[j:j + n]) << (2 * j)
    pos = np.nonzero(valid)[0]
    return pos, np.minimum(w, r)[pos]


def make_set(seqs):
    """S as a dict: canonical value -> the lowest index of a sequence that holds it."""
    s = {}
    for i, codes in enumerate(seqs):
        for c in windows_of(codes)[1].tolist():
            s.setdefault(c, i)
    return s


def screen_ref(sset, params, codes, lo=0, hi=None):
    """(windows, hits, first, source, verdict) of codes[lo:hi] against the dict sset."""
    hi = len(codes) if hi is None else hi
    pos, vals = windows_of(np.asarray(codes, np.uint8)[lo:hi])
    hits, first, source = 0, NONE, NONE
    for p, c in zip(pos.tolist(), vals.tolist()):
        if c in sset:
            hits += 1
            if first == NONE:
                first, source = p, sset[c]
    windows = len(pos)
    verdict = 1 if hits >= params.min_hits and 100 * hits >= params.min_pct * windows else 0
    return windows, hits, first, source, verdict


def screen_many(sset, params, reads, lo=None, hi=None):
    rows = [screen_ref(sset, params, r, 0 if lo is None else int(lo[i]), None if hi is None else int(hi[i])) for i, r in enumerate(reads)]
    return tuple(np.array([row[k] for row in rows], np.uint32) for k in range(5))


def home_slot(c, log2m):
    return ((c * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - log2m)


_HASH_INV = pow(0x9E3779B1, -1, 1 << 32)


def keys_homed_at(slot, log2m, count, rng, taken=()):
    """`count` distinct canonical values whose home slot is `slot` in a table of 1 << log2m slots, none of them in `taken`."""
    out = []
    while len(out) < count:
        x = (slot << (32 - log2m)) | rng.getrandbits(32 - log2m)
        c = (x * _HASH_INV) & 0xFFFFFFFF
        if c == canonical(c) and c not in out and c not in taken:
            assert home_slot(c, log2m) == slot
            out.append(c)
    return out


def concat(reads):
    off = np.zeros(len(reads) + 1, np.uint64)
    if len(reads):
        off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    flat = np.concatenate([np.asarray(r, np.uint8) for r in reads]) if len(reads) and int(off[-1]) else np.zeros(0, np.uint8)
    return flat, off


def random_codes(rng, n):
    return np.array([1 << rng.randrange(4) for _ in range(n)], np.uint8)


def other_base(code):
    return {1: 2, 2: 4, 4: 8, 8: 1}[int(code)]


def plant(codes, off, source, g, n, rc=False):
    """Writes source[g : g + n] -- or its reverse complement -- to codes[off : off + n] and makes the bases of `codes` on either side differ
    from what `source` continues with (1 <= g, g + n < len(source)), so that exactly the n - 15 windows inside the stretch are the source's."""
    piece = source[g:g + n]
    before, behind = source[g - 1], source[g + n]
    if rc:
        piece, before, behind = revcomp(piece), COMP[source[g + n]], COMP[source[g - 1]]
    codes[off:off + n] = piece
    if off > 0:
        codes[off - 1] = other_base(before)
    if off + n < len(codes):
        codes[off + n] = other_base(behind)
    return codes


def emul_read(emul, sset_obj, codes, lo=0, hi=None):
    """emul_screen_read (rtx_emul.cpp) on codes[lo:hi] with the table of an rx.ScreenSet: (windows, hits, first, source)."""
    hi = len(codes) if hi is None else hi
    if not hasattr(sset_obj, "_emul_table"):
        sset_obj._emul_table = sset_obj.table()
    slots, log2m = sset_obj._emul_table
    x = np.ascontiguousarray(np.asarray(codes, np.uint8)[lo:hi])
    out = (C.c_uint32 * 4)()
    emul.emul_screen_read.restype = None
    emul.emul_screen_read(slots.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(log2m), x.ctypes.data_as(C.POINTER(C.c_uint8)) if len(x) else None,
                          C.c_uint32(len(x)), out)
    return tuple(int(v) for v in out)


class World:
    """A set as the library holds it and as the restatement holds it."""

    def __init__(self, seqs):
        self.seqs = [np.asarray(s, np.uint8) for s in seqs]
        self.obj = rx.ScreenSet(self.seqs)
        self.ref = make_set(self.seqs)


def adversarial_world():
    """A set given as single-window sequences whose keys crowd the end of a 1024-slot table: ten keys homed at slot 1020, three each at 1022
    and 1023 -- one chain from 1020 across the wrap to slot 11 -- and a few elsewhere.  absent: values homed inside that chain that the
    set does not hold."""
    rng = random.Random(50)
    keys = keys_homed_at(1020, 10, 10, rng) + keys_homed_at(1022, 10, 3, rng) + keys_homed_at(1023, 10, 3, rng) + keys_homed_at(500, 10, 2, rng)
    rng.shuffle(keys)
    world = World([kmer_codes(c) for c in keys])
    absent = []
    for slot in (1020, 1021, 1022, 1023, 0, 1, 5, 11):
        absent += keys_homed_at(slot, 10, 2, rng, taken=keys)
    return world, keys, absent


def large_world():
    """About 200 000 random canonical keys as single-window sequences, and as many values that are no members."""
    rng = np.random.default_rng(60)
    raw = rng.integers(0, 1 << 32, 420_000, dtype=np.uint64)
    two = (raw[:, None] >> (2 * (15 - np.arange(16, dtype=np.uint64)))) & np.uint64(3)
    rc = ((np.uint64(3) - two[:, ::-1]) << (2 * (15 - np.arange(16, dtype=np.uint64)))).sum(axis=1)
    canon = np.unique(np.minimum(raw, rc))
    rng.shuffle(canon)
    members, others = canon[:200_000], canon[200_000:400_000]
    codes = (np.uint8(1) << ((members[:, None] >> (2 * (15 - np.arange(16, dtype=np.uint64)))) & np.uint64(3)).astype(np.uint8)).astype(np.uint8)
    obj = rx.ScreenSet.from_arrays(codes.reshape(-1), np.arange(0, 16 * len(members) + 1, 16, dtype=np.uint64))
    ref = {int(c): i for i, c in enumerate(members.tolist())}
    return obj, ref, members, others


def large_reads(members, others, per_read=64):
    """Reads of `per_read` 16-mers each, a breaking code behind every one: members, non-members, and the two mixed."""
    def read_of(vals):
        two = (vals[:, None] >> (2 * (15 - np.arange(16, dtype=np.uint64)))) & np.uint64(3)
        codes = np.full((len(vals), 17), 15, np.uint8)
        codes[:, :16] = np.uint8(1) << two.astype(np.uint8)
        return codes.reshape(-1)
    reads = []
    for a in range(0, len(members), per_read):
        reads.append(read_of(members[a:a + per_read]))
        reads.append(read_of(others[a:a + per_read]))
    mixed = np.empty(2 * per_read, np.uint64)
    for a in range(0, 4096, per_read):
        mixed[0::2] = others[a:a + per_read]
        mixed[1::2] = members[a:a + per_read]
        reads.append(read_of(mixed))
    return reads

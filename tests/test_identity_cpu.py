"""Alignment identity (RTX_OPT_IDENTITY, rtx_identity.hip) without a GPU: the additions to the C ABI, the host function
rtx_semiglobal_distance, and the device's block step and plane construction (rtx_math.hpp: identity_block_init, identity_step) run
through the x86 emulator -- all against a plain Sellers recurrence written here in numpy.

sellers(q, r): D[i][0] = i, D[0][j] = 0 (the reference's overhang in front is free), D[i][j] = min(D[i-1][j-1] + mismatch, D[i-1][j] + 1,
D[i][j-1] + 1); the answer is the minimum of the last row (the overhang behind is free), column 0 -- the empty substring -- included.  Column
by column; the chain of vertical steps inside a column is minimum.accumulate(cand - idx) + idx.  Two bytes match when both are codes
(1 .. 15) and share a bit."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx

ROOT = Path(__file__).resolve().parent.parent
u8p = C.POINTER(C.c_uint8)


def sellers(q, r):
    q = np.asarray(q, np.uint8)
    r = np.asarray(r, np.uint8)
    m = len(q)
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    best = m
    qc = np.where(q > 15, 0, q).astype(np.uint8)
    for c in r:
        c = 0 if c > 15 else int(c)
        mis = ((qc & c) == 0).astype(np.int64)
        cand = np.empty(m + 1, np.int64)
        cand[0] = 0
        cand[1:] = np.minimum(col[:-1] + mis, col[1:] + 1)
        col = np.minimum.accumulate(cand - idx) + idx
        best = min(best, int(col[m]))
    return best


def revcomp(seq):
    s = np.asarray(seq, np.uint8)[::-1].copy()
    ok = s <= 15
    b = s[ok]
    s[ok] = ((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3)
    return s


def fixed_and_random_pairs():
    rng = np.random.default_rng(28)
    acgt = np.array([1, 2, 4, 8], np.uint8)
    rnd = lambda n: acgt[rng.integers(0, 4, n)]
    pairs = []
    ref = rnd(658)
    pairs.append((rnd(40), np.zeros(0, np.uint8)))                      # an empty reference: dist == qlen
    pairs.append((ref.copy(), ref))                                     # equal
    pairs.append((ref[200:400].copy(), ref))                            # a substring
    pairs.append((np.concatenate([ref[:300], rnd(30)]), ref[:300]))     # a prefix and 30 bases of overhang
    for pos in (0, 329, 657):
        s = ref.copy()
        s[pos] = {1: 2, 2: 4, 4: 8, 8: 1}[int(s[pos])]
        pairs.append((s, ref))                                          # a substitution
        pairs.append((np.insert(ref, pos, 1 if ref[pos] != 1 else 2), ref))  # an insertion
        pairs.append((np.delete(ref, pos), ref))                        # a deletion
    for side in (0, 1):                                                 # N and other ambiguity codes, byte 0 and byte 0x20, on either side
        for byte in (15, 3, 5, 10, 0, 0x20):
            a, b = ref[100:400].copy(), ref.copy()
            (a if side == 0 else b)[[150, 151, 290] if side == 0 else [250, 251, 390]] = byte
            pairs.append((a, b))
    for n in (1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096):
        r = rnd(n + 50)
        s = r[20:20 + n].copy()
        hit = rng.integers(0, n, max(1, n // 50))
        s[hit] = acgt[rng.integers(0, 4, len(hit))]
        pairs.append((s, r))
    codes = np.array([1, 2, 4, 8, 1, 2, 4, 8, 1, 2, 4, 8, 15, 3, 6, 9, 0, 0x20, 200], np.uint8)
    for k in range(300):                                                # random pairs: related by edits, with odd bytes, any lengths
        n = int(rng.integers(1, 400))
        r = codes[rng.integers(0, len(codes), n)]
        s = list(r[int(rng.integers(0, n)):][:int(rng.integers(1, 300))])
        for _ in range(int(rng.integers(0, 12))):
            p = int(rng.integers(0, len(s) + 1))
            op = int(rng.integers(0, 3))
            if op == 0 and p < len(s):
                s[p] = int(codes[rng.integers(0, len(codes))])
            elif op == 1:
                s.insert(p, int(codes[rng.integers(0, len(codes))]))
            elif len(s) > 1 and p < len(s):
                del s[p]
        if k % 7 == 0:
            s = s + list(rnd(int(rng.integers(1, 40))))
        if k % 31 == 0:
            r = np.zeros(0, np.uint8)
        pairs.append((np.array(s, np.uint8), np.asarray(r, np.uint8)))
    return pairs


@pytest.fixture(scope="module")
def pairs():
    ps = fixed_and_random_pairs()
    return [(q, r, sellers(q, r)) for q, r in ps]


def test_the_header_declares_and_the_library_exports_the_additions():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    assert re.search(r"#define\s+RTX_OPT_IDENTITY\s+28\b", header)
    assert re.search(r"#define\s+RTX_NO_DIST\s+0xFFFFFFFFu\b", header)
    assert re.search(r"#define\s+RTX_IDENTITY_MAX_QUERY\s+4096u?\b", header)
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+6\b", header)
    assert re.search(r"\bint\s+rtx_batch_identity\s*\(\s*rtx_index\s*\*\s*\w*\s*,\s*const\s+uint32_t\s*\*\*\s*dist\s*,\s*const\s+uint32_t\s*\*\*\s*qlen\s*\)", header)
    assert re.search(r"\bint\s+rtx_batch_identity_time\s*\(", header)
    assert re.search(r"\bint\s+rtx_semiglobal_distance\s*\(", header)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*rtx_query_align_fn\s*\)", header)
    assert re.search(r"\bint\s+rtx_raxtax_multi_ex3\s*\(", header)
    lib = rx._lib.load()
    for name in ("rtx_batch_identity", "rtx_batch_identity_time", "rtx_semiglobal_distance", "rtx_raxtax_multi_ex3"):
        assert name in rx._lib._SIGNATURES and hasattr(lib, name), name
    assert hasattr(lib, "rtx_raxtax_multi_ex2")   # stays
    assert rx.NO_DIST == 0xFFFFFFFF


def test_the_numpy_recurrence_on_cases_known_by_hand():
    a = np.array([1, 2, 4, 8, 1, 2], np.uint8)
    assert sellers(a, a) == 0
    assert sellers(a[1:4], a) == 0
    assert sellers(a, np.zeros(0, np.uint8)) == 6
    assert sellers(a, a[:4]) == 2                          # two bases hang over
    assert sellers(np.array([1, 1, 1], np.uint8), np.array([8, 8, 8, 8], np.uint8)) == 3
    assert sellers(np.array([15], np.uint8), np.array([4], np.uint8)) == 0
    assert sellers(np.array([0x20], np.uint8), np.array([0x20], np.uint8)) == 1


def test_semiglobal_distance_equals_the_recurrence(pairs):
    assert len(pairs) > 300
    for q, r, want in pairs:
        assert rx.semiglobal_distance(q, r) == want, (len(q), len(r))
        assert 0 <= want <= len(q)
    assert rx.semiglobal_distance(np.zeros(0, np.uint8), np.array([1, 2], np.uint8)) == 0


def _emul_identity(emul, stored, first, qlen, packed, minus, r):
    emul.emul_identity.restype = C.c_uint32
    r = np.ascontiguousarray(r, np.uint8)
    return emul.emul_identity(stored.ctypes.data_as(u8p), C.c_uint64(first), C.c_uint32(qlen), C.c_int(packed), C.c_int(minus),
                              r.ctypes.data_as(u8p), C.c_uint32(len(r)))


def _pack(first, seq):
    """`seq` two bases per byte, its first base at nibble `first` of the array (what a batch's input set holds for a query in its middle)."""
    nib = np.zeros(first + len(seq) + 2, np.uint8)
    nib[:first] = 7
    nib[first:first + len(seq)] = seq
    nib = nib[:len(nib) // 2 * 2]
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


def test_the_emulated_device_step_equals_the_recurrence(emul, pairs):
    for k, (q, r, want) in enumerate(pairs):
        if len(q) == 0:
            continue
        first = (3, 4, 0)[k % 3]
        raw = np.concatenate([np.full(first, 9, np.uint8), q, np.zeros(2, np.uint8)])
        assert _emul_identity(emul, raw, first, len(q), 0, 0, r) == want, k
        if q.max() <= 15:
            assert _emul_identity(emul, _pack(first, q), first, len(q), 1, 0, r) == want, k


def test_the_planes_of_a_minus_strand_query_are_those_of_its_reverse_complement(emul, pairs):
    """The device holds the query as the caller gave it and builds the planes of the classified orientation on the fly: given revcomp(q),
    minus = 1 must come to the distance of q itself."""
    for k, (q, r, want) in enumerate(pairs):
        if len(q) == 0:
            continue
        given = revcomp(q)
        first = (5, 0, 2)[k % 3]
        raw = np.concatenate([np.full(first, 9, np.uint8), given, np.zeros(2, np.uint8)])
        assert _emul_identity(emul, raw, first, len(q), 0, 1, r) == want, k
        if given.max() <= 15:
            assert _emul_identity(emul, _pack(first, given), first, len(q), 1, 1, r) == want, k


def test_identity_in_hundredths_of_a_percent(emul):
    emul.emul_identity_hundredths.restype = C.c_uint32
    for dist, qlen in ((0, 658), (9, 658), (658, 658), (1, 3), (1, 7), (2, 4096), (329, 658)):
        assert emul.emul_identity_hundredths(C.c_uint32(dist), C.c_uint32(qlen)) == ((qlen - dist) * 10000 + qlen // 2) // qlen
    assert emul.emul_identity_hundredths(C.c_uint32(9), C.c_uint32(658)) == 9863   # prints as 98.63

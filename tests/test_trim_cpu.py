"""Primer trimming (rtx_trim.hip, rtx_index_set_primers) without a GPU: the additions to the C ABI, the host function rtx_primer_search,
the device's staging, plane construction and search (rtx_math.hpp: trim_stage_row, trim_pattern_init, trim_read -> trim_search) run
through the x86 emulator, rtx_trim_apply and the checks of rtx_trim_create -- all against a plain Sellers recurrence written here in numpy.

search(p, x, w, k): X = x[0 .. min(len(x), w)).  D[i][0] = i, D[0][j] = 0 (the text in front of the match is free), D[i][j] = min(D[i-1][j-1]
+ mismatch, D[i-1][j] + 1, D[i][j-1] + 1); E[j] = D[m][j], E[0] = m.  e = min E, j* = the LARGEST j with E[j] == e; found iff e <= k.  Column by
column; the chain of vertical steps inside a column is minimum.accumulate(cand - idx) + idx.  Two bytes match when both are codes (1 .. 15)
and share a bit.  A 3' search is the search of the reversed pattern in the reversed read."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
NO_DIST = 0xFFFFFFFF
A, Cc, G, T, W, Y, N = 1, 2, 4, 8, 9, 10, 15


def window_of(m, k, w):
    return w if w else min(256, m + k + 32)


def search(p, x, w, k):
    """(j*, e) of the docstring, or (0, NO_DIST) when e > k.  w as resolved (never 0)."""
    p = np.asarray(p, np.uint8)
    x = np.asarray(x, np.uint8)[:w]
    m = len(p)
    idx = np.arange(m + 1, dtype=np.int64)
    col = idx.copy()
    best_e, best_j = m, 0
    for j, c in enumerate(x, 1):
        c = 0 if c > 15 else int(c)
        mis = ((p & c) == 0).astype(np.int64)
        cand = np.empty(m + 1, np.int64)
        cand[0] = 0
        cand[1:] = np.minimum(col[:-1] + mis, col[1:] + 1)
        col = np.minimum.accumulate(cand - idx) + idx
        if int(col[m]) <= best_e:          # <=: the largest j of the least E
            best_e, best_j = int(col[m]), j
    return (best_j, best_e) if best_e <= k else (0, NO_DIST)


def search_end(p, x, end, w, k):
    p = np.asarray(p, np.uint8)
    x = np.asarray(x, np.uint8)
    w = window_of(len(p), k, w)
    return search(p[::-1], x[::-1], w, k) if end else search(p, x, w, k)


def trim_ref(patterns, x):
    """(lo, hi, hit) of one read against a list of (codes, end, max_errors, window)."""
    best = {0: (0, NO_DIST, 0xFF), 1: (0, NO_DIST, 0xFF)}
    for i, (p, end, k, w) in enumerate(patterns):
        cut, e = search_end(p, x, end, w, k)
        if e < best[end][1]:
            best[end] = (cut, e, i)
    lo = best[0][0]
    hi = max(len(x) - best[1][0], lo)
    e5 = 0 if best[0][2] == 0xFF else best[0][1]
    e3 = 0 if best[1][2] == 0xFF else best[1][1]
    return lo, hi, best[0][2] | e5 << 8 | best[1][2] << 16 | e3 << 24


def cases():
    """(pattern, read, end, window, k) -- fixed and random."""
    rng = np.random.default_rng(31)
    acgt = np.array([1, 2, 4, 8], np.uint8)
    rnd = lambda n: acgt[rng.integers(0, 4, n)]
    other = lambda b: {1: 2, 2: 4, 4: 8, 8: 1}[int(b)]
    out = []
    for m in (1, 2, 31, 32, 33, 63, 64):
        p = rnd(m)
        body = rnd(300)
        for k in sorted({0, m - 1}):
            for w in sorted({1, max(m - 1, 1), m, 256, 0}):
                for end in (0, 1):
                    read = np.concatenate([rnd(3), p, body]) if end == 0 else np.concatenate([body, p, rnd(3)])
                    out.append((p, read, end, w, k))
            out.append((p, p[:max(m - 1, 0)].copy(), 0, 0, k))          # a text shorter than the pattern
            out.append((p, np.zeros(0, np.uint8), 0, 0, k))             # of length 0
            out.append((p, np.zeros(0, np.uint8), 1, 0, k))
            wx = window_of(m, k, 0)
            out.append((p, np.concatenate([rnd(wx - m), p]), 0, 0, k))  # of exactly the window, the primer at its end
            out.append((p, np.concatenate([rnd(wx - m + 1), p]), 0, 0, k))  # ... one base past it
    p = rnd(20)
    for endpos in (15, 16, 17, 31, 32, 33):                             # primers ending at these text positions (chunks of 32 bases, nibble pairs)
        if endpos >= 20:
            out.append((p, np.concatenate([rnd(endpos - 20), p, rnd(100)]), 0, 0, 2))
            out.append((p, np.concatenate([rnd(100), p, rnd(endpos - 20)]), 1, 0, 2))
        q = p[:12]
        out.append((q, np.concatenate([rnd(endpos - 12), q, rnd(100)]), 0, 0, 1))
        out.append((q, np.concatenate([rnd(100), q, rnd(endpos - 12)]), 1, 0, 1))
    p = rnd(25)
    for pos in (0, 12, 24):                                             # an edit at the first, a middle and the last primer base
        s = p.copy()
        s[pos] = other(s[pos])
        ins = np.insert(p, pos, other(p[pos]))
        dele = np.delete(p, pos)
        for seen in (s, ins, dele):
            for k in (0, 1, 2):
                out.append((p, np.concatenate([seen, rnd(200)]), 0, 0, k))
                out.append((p, np.concatenate([rnd(200), seen]), 1, 0, k))
                out.append((p, np.concatenate([rnd(5), seen, rnd(200)]), 0, 0, k))
    deg = np.array([G, G, W, A, Cc, W, G, G, W, T, G, A, A, Y, N, Cc, Y, T, A, Y, G, G], np.uint8)   # degenerate pattern codes
    inst = np.array([G, G, A, A, Cc, T, G, G, T, T, G, A, A, Cc, G, Cc, T, T, A, Cc, G, G], np.uint8)
    out.append((deg, np.concatenate([inst, rnd(100)]), 0, 0, 0))
    out.append((deg, np.concatenate([rnd(100), inst]), 1, 0, 0))
    amb = inst.copy()
    amb[[3, 9]] = (5, 15)                                               # ambiguity codes in the read: R holds A, N holds T
    out.append((deg, np.concatenate([amb, rnd(100)]), 0, 0, 0))
    amb[4] = 12                                                         # K does not hold C
    out.append((deg, np.concatenate([amb, rnd(100)]), 0, 0, 0))
    out.append((deg, np.concatenate([amb, rnd(100)]), 0, 0, 1))
    for byte in (0, 0x20, 200):                                         # read bytes that are no code match nothing, not even N
        s = inst.copy()
        s[14] = byte
        out.append((deg, np.concatenate([s, rnd(100)]), 0, 0, 0))
        out.append((deg, np.concatenate([s, rnd(100)]), 0, 0, 1))
        out.append((deg, np.concatenate([rnd(100), s]), 1, 0, 1))
        out.append((deg, np.full(60, byte, np.uint8), 0, 0, 21))
    # two j of equal E: pattern ACGT in ACGTT with k = 1 -- E[4] = 0 alone; pattern ACG, k = 1, in ACTGA: E = 1 at j = 2, 3 (AC-, ACT) and 4 (ACTG)
    out.append((np.array([A, Cc, G], np.uint8), np.array([A, Cc, T, G, A], np.uint8), 0, 0, 1))
    out.append((np.array([A, Cc, G, T], np.uint8), np.array([A, Cc, G, G, T, T, T], np.uint8), 0, 0, 1))
    out.append((np.array([A, A, A, A], np.uint8), np.full(40, A, np.uint8), 0, 0, 0))      # E = 0 from j = 4 on: the window's end wins
    out.append((np.array([A, A, A, A], np.uint8), np.full(40, A, np.uint8), 1, 10, 0))
    # the best E is k + 1: not found
    p = rnd(20)
    s = p.copy()
    s[[4, 9, 15]] = [other(s[4]), other(s[9]), other(s[15])]
    out.append((p, np.concatenate([s, rnd(9) * 0 + 200]), 0, 0, 2))
    out.append((p, np.concatenate([s, np.full(50, 200, np.uint8)]), 0, 0, 3))
    codes = np.array([1, 2, 4, 8, 1, 2, 4, 8, 1, 2, 4, 8, 15, 3, 6, 9, 0, 0x20, 200], np.uint8)
    pcodes = np.array([1, 2, 4, 8, 1, 2, 4, 8, 9, 10, 15, 5], np.uint8)
    for _ in range(300):                                                # random: a pattern, an edited copy somewhere near an end, odd bytes
        m = int(rng.integers(1, 65))
        p = pcodes[rng.integers(0, len(pcodes), m)]
        s = list(p)
        for _e in range(int(rng.integers(0, 5))):
            pos = int(rng.integers(0, len(s) + 1))
            op = int(rng.integers(0, 3))
            if op == 0 and pos < len(s):
                s[pos] = int(codes[rng.integers(0, len(codes))])
            elif op == 1:
                s.insert(pos, int(codes[rng.integers(0, len(codes))]))
            elif len(s) > 1 and pos < len(s):
                del s[pos]
        pre, post = codes[rng.integers(0, 12, int(rng.integers(0, 40)))], codes[rng.integers(0, len(codes), int(rng.integers(0, 300)))]
        end = int(rng.integers(0, 2))
        read = np.concatenate([pre, np.array(s, np.uint8), post]).astype(np.uint8)
        if end:
            read = read[::-1].copy()
            p = p[::-1].copy()
        k = int(rng.integers(0, m))
        w = int(rng.choice([0, 0, 1, m, 40, 256, int(rng.integers(1, 257))]))
        out.append((p, read, end, w, k))
    return [(np.ascontiguousarray(p, np.uint8), np.ascontiguousarray(x, np.uint8), e, w, k) for p, x, e, w, k in out]


@pytest.fixture(scope="module")
def solved():
    return [(p, x, end, w, k, search_end(p, x, end, w, k)) for p, x, end, w, k in cases()]


def test_the_header_declares_and_the_library_exports_the_additions():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+6\b", header)
    assert re.search(r"#define\s+RTX_TRIM_5P\s+0u\b", header) and re.search(r"#define\s+RTX_TRIM_3P\s+1u\b", header)
    assert re.search(r"#define\s+RTX_TRIM_MAX_PATTERNS\s+8\b", header)
    assert re.search(r"#define\s+RTX_TRIM_MAX_PATTERN\s+64\b", header)
    assert re.search(r"#define\s+RTX_TRIM_MAX_WINDOW\s+256\b", header)
    assert re.search(r"typedef\s+struct\s*\{\s*const\s+uint8_t\s*\*\s*codes\s*;\s*uint32_t\s+len\s*,\s*end\s*,\s*max_errors\s*,\s*window\s*;\s*\}\s*rtx_trim_pattern\s*;", header)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*rtx_query_trim_fn\s*\)", header)
    lib = _lib.load()
    for name in ("rtx_trim_create", "rtx_trim_run", "rtx_trim_destroy", "rtx_primer_search", "rtx_trim_apply", "rtx_index_set_primers",
                 "rtx_index_primers", "rtx_raxtax_last_trim", "rtx_raxtax_multi_ex4"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib._SIGNATURES and hasattr(lib, name), name
    assert hasattr(lib, "rtx_raxtax_multi_ex3")   # stays
    assert len(rx.raxtax_last_trim()) == 5


def test_the_numpy_recurrence_on_cases_known_by_hand():
    acgt = np.array([A, Cc, G, T], np.uint8)
    assert search(acgt, np.array([T, T, A, Cc, G, T, A], np.uint8), 256, 0) == (6, 0)
    assert search(acgt, np.array([T, T, A, Cc, G, T, A], np.uint8), 5, 0) == (0, NO_DIST)     # the window ends inside the primer
    assert search(acgt, np.array([T, T, A, Cc, G, T, A], np.uint8), 5, 1) == (5, 1)           # ... ACG- with one deletion
    assert search(acgt, np.zeros(0, np.uint8), 256, 3) == (0, NO_DIST)                        # E[0] = m > k
    assert search(np.array([A, Cc, G], np.uint8), np.array([A, Cc, T, G, A], np.uint8), 256, 1) == (4, 1)   # E = 1 at j = 2, 3 and 4: the largest
    assert search(np.array([N], np.uint8), np.array([0x20], np.uint8), 256, 0) == (0, NO_DIST)
    assert search(acgt, np.array([A, Cc, Cc, T], np.uint8), 256, 0) == (0, NO_DIST)           # the best E is k + 1: not found
    assert search(acgt, np.array([A, Cc, Cc, T], np.uint8), 256, 1) == (4, 1)
    assert search(np.array([W], np.uint8), np.array([T], np.uint8), 256, 0) == (1, 0)
    assert search_end(acgt, np.array([G, G, A, Cc, G, T, A], np.uint8), 1, 0, 0) == (5, 0)    # 3': ACGT and the A behind it go
    assert window_of(20, 2, 0) == 54 and window_of(64, 63, 0) == 159 and window_of(64, 63, 7) == 7


def test_primer_search_equals_the_recurrence(solved):
    assert len(solved) > 500
    found = ties = 0
    for p, x, end, w, k, want in solved:
        assert rx.primer_search(p, x, end=end, window=w, max_errors=k) == want, (len(p), len(x), end, w, k)
        found += want[1] != NO_DIST
    assert 100 < found < len(solved)


def test_a_3p_search_is_the_5p_search_of_the_reversed_problem(solved):
    for p, x, end, w, k, want in solved:
        assert rx.primer_search(p[::-1].copy(), x[::-1].copy(), end=1 - end, window=w, max_errors=k) == want


def _emul_trim_read(emul, patterns, x):
    codes = np.concatenate([np.asarray(p[0], np.uint8) for p in patterns])
    off = np.zeros(len(patterns) + 1, np.uint32)
    off[1:] = np.cumsum([len(p[0]) for p in patterns])
    end, k, w = (np.array([p[i] for p in patterns], np.uint32) for i in (1, 2, 3))
    x = np.ascontiguousarray(x, np.uint8)
    xs = x if len(x) else np.zeros(1, np.uint8)
    lo, hi, hit = C.c_uint32(), C.c_uint32(), C.c_uint32()
    emul.emul_trim_read.restype = None
    emul.emul_trim_read(C.c_uint32(len(patterns)), codes.ctypes.data_as(u8p), off.ctypes.data_as(u32p), end.ctypes.data_as(u32p),
                        k.ctypes.data_as(u32p), w.ctypes.data_as(u32p), xs.ctypes.data_as(u8p), C.c_uint32(len(x)), C.byref(lo), C.byref(hi), C.byref(hit))
    return lo.value, hi.value, hit.value


def test_the_emulated_device_search_equals_the_recurrence(emul, solved):
    """One pattern per run: the cut and the errors of every case come back in lo / hi and the hit word."""
    for p, x, end, w, k, (cut, e) in solved:
        lo, hi, hit = _emul_trim_read(emul, [(p, end, k, w)], x)
        none = e == NO_DIST
        if end == 0:
            assert (lo, hi) == (cut, max(len(x), cut)) and hit == ((0xFF if none else 0) | (0 if none else e) << 8 | 0xFF << 16), (len(p), len(x), w, k)
        else:
            assert (lo, hi) == (0, len(x) - cut) and hit == (0xFF | (0xFF if none else 0) << 16 | (0 if none else e) << 24), (len(p), len(x), w, k)


def test_the_emulated_device_read_equals_the_recurrence_over_several_patterns(emul, solved):
    """Four patterns, two per end, on the reads of the cases: the least errors, then the lowest index; overlapping cuts leave lo == hi."""
    rng = np.random.default_rng(5)
    for n, (p, x, end, w, k, _) in enumerate(solved):
        q = p.copy()
        q[int(rng.integers(0, len(q)))] = 15
        pats = [(p, 0, k, w), (q, 0, k, w), (p[::-1].copy(), 1, k, w), (q[::-1].copy(), 1, k, 0)]
        if n % 3 == 0:
            pats = [pats[1], pats[0], pats[3], pats[2]]
        assert _emul_trim_read(emul, pats, x) == trim_ref(pats, x), n
    # equal errors: the lower index
    p = np.array([A, Cc, G, T, A, Cc], np.uint8)
    x = np.concatenate([p, np.full(30, G, np.uint8), p])
    assert trim_ref([(p, 0, 0, 0), (p, 0, 0, 0), (p, 1, 0, 0)], x) == (6, 36, 0 | 0 << 8 | 2 << 16)
    assert _emul_trim_read(emul, [(p, 0, 0, 0), (p, 0, 0, 0), (p, 1, 0, 0)], x) == (6, 36, 2 << 16)
    assert _emul_trim_read(emul, [(p, 0, 0, 0), (p, 1, 0, 0)], p) == (6, 6, 1 << 16)      # one primer, both ends claim it: the read is left empty


def test_trim_apply():
    seqs = [np.array([1, 2, 4, 8, 1], np.uint8), np.zeros(0, np.uint8), np.array([8, 4], np.uint8), np.array([2, 2, 2], np.uint8)]
    flat = np.concatenate(seqs)
    off = np.array([0, 5, 5, 7, 10], np.uint64)
    lo = np.array([1, 0, 0, 3], np.uint32)
    hi = np.array([4, 0, 2, 3], np.uint32)          # a cut read, an empty one, an untouched one, lo == hi at the read's end
    out, ooff = rx.trim_apply(flat, off, lo, hi)
    assert list(ooff) == [0, 3, 3, 5, 5] and list(out) == [2, 4, 8, 8, 4]
    out, ooff = rx.trim_apply(flat, off, np.zeros(4, np.uint32), np.array([5, 0, 2, 3], np.uint32))
    assert list(ooff) == list(off) and list(out) == list(flat)
    out, ooff = rx.trim_apply(flat, off, np.array([5, 0, 1, 0], np.uint32), np.array([5, 0, 1, 0], np.uint32))
    assert list(ooff) == [0, 0, 0, 0, 0] and len(out) == 0
    out, ooff = rx.trim_apply(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32))   # n == 0
    assert list(ooff) == [0] and len(out) == 0
    for bad_lo, bad_hi in (([2, 0, 0, 0], [1, 0, 0, 0]), ([0, 0, 0, 0], [6, 0, 0, 0]), ([0, 1, 0, 0], [0, 1, 0, 0])):
        with pytest.raises(rx.RtxError) as e:
            rx.trim_apply(flat, off, np.array(bad_lo, np.uint32), np.array(bad_hi, np.uint32))
        assert e.value.code == _lib.RTX_ERR_INVALID
    big = np.arange(20000 * 7, dtype=np.uint32).astype(np.uint8)       # enough reads for the copy to be shared among threads
    boff = (np.arange(20001, dtype=np.uint64) * 7)
    out, ooff = rx.trim_apply(big, boff, np.full(20000, 2, np.uint32), np.full(20000, 6, np.uint32))
    assert np.array_equal(out, big.reshape(20000, 7)[:, 2:6].reshape(-1)) and int(ooff[-1]) == 80000


def _create(pats, n=None):
    arr, keep = rx.api._trim_patterns(pats)
    h = C.c_void_p()
    return _lib.load().rtx_trim_create(0, arr, len(keep) if n is None else n, C.byref(h)), h


def test_trim_create_refuses_bad_patterns_before_it_looks_for_a_device():
    ok = np.array([A, Cc, G, T, W, N], np.uint8)
    bad = [[(np.array([A, 0, G], np.uint8), 0, 0, 0)],                 # a byte that is no code
           [(np.array([A, 16, G], np.uint8), 0, 0, 0)],
           [(np.zeros(0, np.uint8), 0, 0, 0)],                         # len 0
           [(np.full(65, A, np.uint8), 0, 0, 0)],                      # len above 64
           [(ok, 0, 6, 0)],                                            # max_errors >= len
           [(ok, 0, 0, 257)],                                          # a window above 256
           [(ok, 2, 0, 0)],                                            # an unknown end
           [(ok, 0, 0, 0)] * 9,                                        # n above 8
           [(ok, 0, 0, 0), (ok, 1, 1, 0), (np.array([A, 200], np.uint8), 1, 0, 0)]]
    for pats in bad:
        rc, h = _create(pats)
        assert rc == _lib.RTX_ERR_INVALID and not h.value, pats
    lib = _lib.load()
    assert lib.rtx_trim_create(0, None, 1, C.byref(C.c_void_p())) == _lib.RTX_ERR_INVALID      # null arguments
    arr, keep = rx.api._trim_patterns([(ok, 0, 0, 0)])
    assert lib.rtx_trim_create(0, arr, 1, None) == _lib.RTX_ERR_INVALID
    assert lib.rtx_trim_create(0, arr, 0, C.byref(C.c_void_p())) == _lib.RTX_ERR_INVALID
    for m, k, w in ((64, 63, 256), (1, 0, 1)):                                                 # the limits themselves are fine
        cut, e = rx.primer_search(np.full(m, N, np.uint8), np.full(300, A, np.uint8), window=w, max_errors=k)
        assert (cut, e) == (w, 0)
    for kw in (dict(max_errors=6), dict(window=257), dict(end=2)):
        with pytest.raises(rx.RtxError) as e:
            rx.primer_search(ok, ok, **kw)
        assert e.value.code == _lib.RTX_ERR_INVALID
    if lib.rtx_device_count() == 0:
        rc, h = _create([(ok, 0, 1, 0), (ok, 1, 0, 40)])
        assert rc == _lib.RTX_ERR_NO_DEVICE and not h.value       # a valid list gets as far as the device
        with pytest.raises(rx.RtxError) as e:
            rx.Trim(0, [(ok, 0, 1, 0)])
        assert e.value.code == _lib.RTX_ERR_NO_DEVICE


def test_the_hit_word():
    assert rx.trim_hit(0xFF | 0xFF << 16) == (None, 0, None, 0)
    assert rx.trim_hit(3 | 2 << 8 | 7 << 16 | 63 << 24) == (3, 2, 7, 63)
    assert rx.trim_hit(0 | 0 << 8 | 0xFF << 16) == (0, 0, None, 0)
    p = np.array([A, Cc, G, T, A, Cc, G, T], np.uint8)
    x = np.concatenate([p, np.full(50, G, np.uint8), p[:5], p[6:]])     # the 3' copy has lost a base
    lo, hi, hit = trim_ref([(p, 1, 1, 0), (p, 0, 1, 0)], x)
    assert (lo, hi) == (8, 58) and rx.trim_hit(hit) == (1, 0, 0, 1) and hit == (1 | 0 << 8 | 0 << 16 | 1 << 24)


def test_the_pattern_list_of_a_primer_pair():
    pats = rx.primer_patterns(("GGWACW", "TAAACYTC"), error_percent=34)
    assert [(list(p.codes), p.end, p.max_errors) for p in pats] == [([4, 4, 9, 1, 2, 9], 0, 2), ([4, 1, 5, 4, 8, 8, 8, 1], 1, 2)]   # GGWACW; GARGTTTA
    both = rx.primer_patterns(("GGWACW", "TAAACYTC"), both_strands=True)
    assert [p.end for p in both] == [0, 1, 0, 1] and list(both[2].codes) == [8, 1, 1, 1, 2, 10, 8, 2] and list(both[3].codes) == [9, 4, 8, 9, 2, 2]
    assert [p.max_errors for p in both] == [0, 0, 0, 0]
    assert [p.end for p in rx.primer_patterns(("", "ACGT"))] == [1] and [p.end for p in rx.primer_patterns(("ACGT", ""))] == [0]
    with pytest.raises(ValueError, match="ACXT"):
        rx.primer_patterns(("ACXT", ""))

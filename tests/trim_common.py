"""The reference of the GPU tests of the primer trimming: Sellers' search of include/raxtax_hip.h as a plain numpy recurrence, over many reads at
once (one column of every read's table per step; tests/test_trim_cpu.py states the same recurrence read by read and holds the host function
and the emulated device code against it).

search(p, x, w, k): X = x[0 .. min(len(x), w)); D[i][0] = i, D[0][j] = 0, D[i][j] = min(D[i-1][j-1] + mismatch, D[i-1][j] + 1, D[i][j-1] + 1);
E[j] = D[m][j]; e = min E, j* = the LARGEST j with E[j] == e; found iff e <= k.  Two bytes match when both are codes (1 .. 15) and share a bit.
A 3' pattern: the reversed pattern in the reversed read.  Several patterns of an end: the least e, then the lowest index."""
import numpy as np

NO_DIST = 0xFFFFFFFF
NONE = 0xFF


def window_of(m, k, w):
    return w if w else min(256, m + k + 32)


def search_many(p, reads, w, k):
    """(cut[n], errors[n]) of pattern p in every read; (0, NO_DIST) where not found.  w as resolved."""
    p = np.asarray(p, np.uint8)
    n, m = len(reads), len(p)
    lens = np.array([min(len(r), w) for r in reads], np.int64)
    X = np.zeros((n, w), np.uint8)
    for i, r in enumerate(reads):
        r = np.asarray(r, np.uint8)[:w]
        X[i, :len(r)] = np.where(r > 15, 0, r)
    idx = np.arange(m + 1, dtype=np.int64)
    col = np.tile(idx, (n, 1))
    best_e = np.full(n, m, np.int64)
    best_j = np.zeros(n, np.int64)
    for j in range(1, w + 1):
        act = lens >= j
        if not act.any():
            break
        mis = ((p[None, :] & X[:, j - 1][:, None]) == 0).astype(np.int64)
        cand = np.empty((n, m + 1), np.int64)
        cand[:, 0] = 0
        cand[:, 1:] = np.minimum(col[:, :-1] + mis, col[:, 1:] + 1)
        new = np.minimum.accumulate(cand - idx, axis=1) + idx
        col = np.where(act[:, None], new, col)
        upd = act & (new[:, m] <= best_e)            # <=: the largest j of the least E
        best_e = np.where(upd, new[:, m], best_e)
        best_j = np.where(upd, j, best_j)
    found = best_e <= k
    return np.where(found, best_j, 0), np.where(found, best_e, NO_DIST)


def trim_many(patterns, reads):
    """(lo, hi, hit) per read for a list of patterns with .codes, .end, .max_errors, .window (rx.TrimPrimer)."""
    n = len(reads)
    lens = np.array([len(r) for r in reads], np.int64)
    rev = [np.asarray(r, np.uint8)[::-1] for r in reads]
    cut = [np.zeros(n, np.int64), np.zeros(n, np.int64)]
    err = [np.full(n, NO_DIST, np.int64), np.full(n, NO_DIST, np.int64)]
    pat = [np.full(n, NONE, np.int64), np.full(n, NONE, np.int64)]
    for i, p in enumerate(patterns):
        codes = np.asarray(p.codes, np.uint8)
        w = window_of(len(codes), p.max_errors, p.window)
        c, e = search_many(codes[::-1], rev, w, p.max_errors) if p.end else search_many(codes, reads, w, p.max_errors)
        better = e < err[p.end]                       # strictly: ties stay with the lower index
        cut[p.end] = np.where(better, c, cut[p.end])
        err[p.end] = np.where(better, e, err[p.end])
        pat[p.end] = np.where(better, i, pat[p.end])
    lo = cut[0]
    hi = np.maximum(lens - cut[1], lo)
    e5 = np.where(pat[0] == NONE, 0, err[0])
    e3 = np.where(pat[1] == NONE, 0, err[1])
    hit = pat[0] | e5 << 8 | pat[1] << 16 | e3 << 24
    return lo.astype(np.uint32), hi.astype(np.uint32), hit.astype(np.uint32)


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(0, np.uint8)])
    return flat, off

"""The probability stage (src/prob.rs:8-103) on injected histograms: an exact reference, the cases, and the comparison.

The kernels under test are prob_lookup_kernel (rtx_prob_tables.hip) and prob_table_kernel<false / true> (rtx_kernels.hip), reached through
rtx_debug_prob_hist with histograms given directly, so that a case can stand for millions of references and can be shaped after the
kernels' structure: the ballots of the distinct counts, the rows dropped as saturated at i_lo, their compaction and the padding to sixteen,
the 64-wide slices of i with their suffix maximum of live rows, the split of slice 0 between two waves, the clipping of a row by its buffer
descriptor, the 64-count groups of the recurrence kernel with their skips, starts and saturation breaks, the 64-step flush of its
global-memory variant.

REFERENCE.  `exact(case)`: prob.rs:8-103 restated in mpmath at 50 digits -- the pmf of prob.rs:121-170 as a ratio of binomial
coefficients held as Python integers and advanced by their exact ratios, cumulative sums, P(i) = prod cmf^h, table, Z, table / Z and the
global signal.  Nothing of the kernels' pruning (i_lo, saturation, the 2^-412 cut) is restated.  Cached per case, shared by the CPU and GPU
files.  Its cost is D (n + 1) high-precision powers per case (measured: tools/NOTES.md).

TOLERANCES (the issue's, not measured ones): |table / Z - exact| <= 1e-11 at every present count and the global signal within 1e-11;
status and number of distinct counts equal; Z of the device within four times the largest relative deviation the oracle and the two
emulators show for that case on the CPU (floor 1e-12): Z carries the conditioning of the ln-factorial table, enters nothing downstream,
and the factor four covers the order of the cross-lane sums.  Pruned runs against the exact values of the ORIGINAL histogram: above the
threshold within 1e-9 (proved: 4e-10, rtx_math.hpp), counts 1..u exactly 0, and within 1e-11 of emul_prob_lookup_pruned."""
import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

TOL = 1e-11          # the project's stated figure for table / Z and the global signal
TOL_PRUNED = 1e-9    # a pruned run against the full computation (proved bound 4e-10)
Z_FACTOR, Z_FLOOR = 4.0, 1e-12
DPS = 50
TAB_TMAX = 2047      # the memoised tables serve t up to here (rtx_api_batch.hip: kProbTablesMaxT)
Q_OK, Q_NO_KMERS = 0, 1
N_REFS = 5_000_000  # the N of the global signal's 1 / N in every launch: a launch has ONE n_refs, which enters nothing else (a case's own total is the sum of its bins)


@dataclass(frozen=True)
class Case:
    name: str
    t: int
    bins: tuple                      # ((count, multiplicity), ...) ascending by count
    note: str = ""
    # what the case promises about the kernels' structure, asserted on the emulators' stats by the CPU tests (None: no promise)
    live: int = None                 # rows still moving at i_lo (prob_lookup)
    slices: tuple = None             # the 64-wide slices (from i_lo) in which some live row moves last, ascending
    skipped: int = None              # groups of 64 counts prob_table_kernel skips
    span: int = None                 # n - i_lo
    pruned: bool = False             # also run through the lookup with the threshold emul_prune_threshold gives its top block
    tol: float = None                # bound on table / Z and the global signal where TOL cannot hold in double precision (see HEAVY)

    @property
    def n(self):
        return self.t // 2

    @property
    def n_refs(self):
        return sum(h for _, h in self.bins)

    @property
    def D(self):
        return len(self.bins)

    def hist(self, stride=None):
        h = np.zeros(stride or self.t + 1, np.uint32)
        for m, c in self.bins:
            h[m] = c
        return h


# HEAVY.  P(i) holds cmf_m(i)^h.  Where the cmf is near 1 a double holds it to 2^-53 at best, and its running sum is a few such steps
# off; the h-th power carries that h times: with h = 4e6 one step is 4.4e-10 of P(i), in ANY implementation in double precision (the
# oracle and both emulators are 2e-11 .. 9e-11 from the exact values on these shapes).  The bound for those cases is two steps, h 2^-52;
# at h = 1e5 the same reasoning gives 2.2e-11 and the cases are held to TOL all the same.
HEAVY_4M_TOL = 4_000_000 * 2.0 ** -52


def _case(name, t, bins, note="", **kw):
    if isinstance(bins, dict):
        bins = bins.items()
    bins = tuple(sorted((int(m), int(h)) for m, h in bins if h))
    assert all(0 <= m <= t for m, _ in bins) and len({m for m, _ in bins}) == len(bins)
    return Case(name, t, bins, note, **kw)


def _run(top, d, h=1):
    """d counts top, top - 1, ..., one reference each (h of them)."""
    return {m: h for m in range(top - d + 1, top + 1)}


def build_cases():
    c = []
    # ---- status and degenerate
    c.append(_case("t0", 0, {0: 12}, "t = 0: RTX_Q_NO_KMERS (u64 underflow at prob.rs:21)"))
    c.append(_case("t1_no_full", 1, {0: 12}, "t = 1 without a full overlap: n = 0, RTX_Q_NO_KMERS (zip_eq at prob.rs:162)"))
    c.append(_case("t1_full", 1, {0: 9, 1: 3}, "t = 1 with three full overlaps: Z = 3, p = 1/3, exactly"))
    c.append(_case("t2", 2, {0: 5, 1: 7}, "n = 1", live=1))
    c.append(_case("t3", 3, {1: 4, 2: 3}, "n = 1, bin 0 absent", live=2))
    c.append(_case("t9_no_hits", 9, {0: 7}, "every count 0: p[0] = 1/N, D = 1", live=0, skipped=1))
    # ---- the full-overlap arm
    c.append(_case("full_all_counts_401", 401, _run(401, 402), "every count 0..401: D = 402, the strides of 256 and 128 threads wrap"))
    c.append(_case("full_beside_one", 300, {300: 2, 57: 9}, "a full overlap beside a single other bin"))
    # ---- distinct-count boundaries, all rows live, bin 0 absent: D = rows
    for d in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129):
        bins = _run(259, d - 1, 2) if d > 1 else {}
        bins[262] = 1
        c.append(_case(f"d{d}", 300, bins, f"D = {d} at t = 300, every row live: the 16-row pad, the strides of 32 (pass 1) and 8 / 32 (pass 2), the "
                       "ballot words, the 64-count groups", live=d, skipped=0))
    bins = _run(259, 63, 2)
    bins[262] = 1
    bins[0] = 1000
    c.append(_case("d64_and_bin0", 300, bins, "64 live rows and bin 0: D = 65, the second group of the recurrence holds count 0 alone (skipped)",
                   live=64, skipped=1))
    # ---- live / dead split at t = 640: only the top rows are live, the low noise bins saturate before i_lo
    for k, low in ((1, 70), (2, 70), (1, 140), (2, 140)):
        bins = {m: 3000 for m in range(1, 1 + low)}
        bins[630] = 1
        if k == 2:
            bins[620] = 2
        bins[0] = 50000
        c.append(_case(f"split_top{k}_low{low}", 640, bins, f"{k} high count(s) over {low} noise bins: table = 0 for the noise without a load", live=k,
                       skipped=(1 + low + k + 63) // 64 - 1, pruned=(k, low) in ((1, 70), (2, 140))))
    for k in (63, 64, 65):
        bins = {m: 1000 for m in range(1, 61)}
        bins.update(_run(560, k))
        c.append(_case(f"split_live{k}", 640, bins, f"{k} live rows on top of 60 dead ones: the compaction's second turn starts with na > 0", live=k, pruned=k == 64))
    # ---- every count 0..t-1
    c.append(_case("all_counts_400", 400, _run(399, 400), "the shape of the reference's own P2 test, general arm"))
    c.append(_case("all_counts_640", 640, _run(639, 640), "D (n + 1) = 205 000: the large one"))
    # ---- slices: the live range from i_lo ends in slice 0, 1, 2, ... with rows ending in different slices
    c.append(_case("slice0_640", 640, {21: 1, 15: 5, 0: 100}, "everything inside slice 0", slices=(0,)))
    c.append(_case("slice1_640", 640, {60: 1, 40: 3, 12: 9, 0: 100}, "rows end in slices 0 and 1", slices=(0, 1)))
    c.append(_case("slice2_640", 640, {150: 1, 60: 2, 15: 5, 0: 100}, "rows end in slices 0, 1, 2", slices=(0, 1, 2)))
    c.append(_case("slice3_640", 640, {370: 1, 300: 2, 200: 3, 120: 5, 0: 100}, "the furthest slice a row reaches at t = 640 (its width from e^-100 to "
                   "saturation bounds it: every top count tried, 3 is the largest); no row ends in slice 0: its live rows come from the suffix maximum alone", slices=(1, 2, 3)))
    c.append(_case("slice_spread_640", 640, {**{m: 1 for m in range(58, 371, 8)}, 0: 100}, "forty rows ending in four slices: the live-row "
                   "counts of the slices differ by more than a batch of sixteen", live=40, slices=(0, 1, 2, 3), pruned=True))
    c.append(_case("slice4_1100", 1100, {600: 1, 450: 2, 300: 3, 200: 5, 120: 8, 0: 100}, "the furthest slice a row reaches at t = 1100 (4): the "
                   "11-plane class, n > 511", slices=(0, 1, 2, 3, 4), pruned=True))
    # ---- n - i_lo on either side of a slice boundary: the last lane of a slice is i = n (tops found with the emulator's i_lo)
    for want, t, top in ((63, 150, 149), (64, 150, 148), (65, 148, 145), (127, 640, 613), (128, 640, 612), (129, 640, 611)):
        c.append(_case(f"span{want}", t, {top: 1, top - 1: 2, top - 40: 4, top - 100: 6, 0: 50}, f"n - i_lo = {want}", span=want))
    c.append(_case("slice0_rows40", 150, _run(149, 40), "forty live rows with all of i in slice 0 (n - i_lo = 63): the halves of the row sum that "
                   "waves 0 and 1 take meet in Ppart, and nothing but slice 0 carries the result", live=40, slices=(0,), span=63))
    # ---- t = 126 .. 131: n = 63, 64, 65, the flush boundary of the global-memory recurrence
    for t in range(126, 132):
        c.append(_case(f"flush_t{t}", t, {t - 1: 1, t - 2: 1, t // 2: 3, 5: 40, 0: 9}, f"n = {t // 2}: the 64-step flush of kernel 2 beside i = n"))
    # ---- weight
    c.append(_case("one_bin_5m", 200, {37: 5_000_000}, "one bin of 5 000 000 alone", live=1))
    c.append(_case("heavy_noise_under_top", 640, {600: 1, 20: 4_000_000}, "4 000 000 at count 20 under a single top of 600", live=1, pruned=True))
    # one count shared by h references just under the top, placed where the top's mass meets that row's saturation: the terms of the
    # row's own sum behind its saturation index count h times in Z (a lookup that stops there is 4e-11 off at h = 1e5, 1e-8 at 4e6)
    for h, tag, tol in ((100_000, "1e5", None), (4_000_000, "4m", HEAVY_4M_TOL)):
        c.append(_case(f"heavy_{tag}_under_500", 640, {500: 1, 360: h, 0: 1000}, f"{h} references at count 360 under a top of 500", tol=tol))
        c.append(_case(f"heavy_{tag}_under_600", 640, {600: 1, 500: h, 0: 1000}, f"{h} references at count 500 under a top of 600", tol=tol))
    c.append(_case("tied_tops", 300, {210: 2, 60: 500, 0: 4000}, "two tied tops", pruned=True))
    c.append(_case("near_tied_tops", 300, {210: 1, 209: 1, 208: 3, 55: 800, 0: 4000}, "tops at M, M - 1, M - 2 with multiplicities 1, 1, 3", pruned=True))
    c.append(_case("top_t_minus_1", 300, {299: 1, 150: 10, 0: 500}, "a top at t - 1"))
    c.append(_case("flat_noise", 400, {m: 5000 for m in range(15, 65)}, "flat noise only: 50 bins of 5 000, no relative"))
    # ---- classes
    c.append(_case("long_2600", 2600, {**{m: 50 for m in range(300, 320)}, 2500: 1, 2499: 2, 1: 7, 0: 1000}, "24 bins at t = 2600: the recurrence "
                   "kernels with the 2^-512 rescaling of the start"))
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Exact:
    status: int
    ndist: int
    p: dict = field(default_factory=dict)    # count -> table / Z
    z: float = 0.0
    gs: float = 0.0


def _pmf_rows(t, n, counts, mp):
    """pmf_m(i) = C(m + i - 1, i) C(t - m + n - i - 1, n - i) / C(t + n - 1, n) for every m of counts, i = 0 .. n, as mpf."""
    total = 1
    for j in range(1, n + 1):                       # C(t + n - 1, n) by its exact ratios
        total = total * (t + j - 1) // j
    rows = {}
    for m in counts:
        a = [1] * (n + 1)                           # a[i] = C(m + i - 1, i)
        for i in range(1, n + 1):
            a[i] = a[i - 1] * (m + i - 1) // i
        r = t - m
        b = [1] * (n + 1)                           # b[j] = C(r + j - 1, j); the second factor at i is b[n - i]
        for j in range(1, n + 1):
            b[j] = b[j - 1] * (r + j - 1) // j
        rows[m] = [mp.mpf(a[i] * b[n - i]) / total for i in range(n + 1)]
    return rows


def exact_tables(t, bins, n_refs, variant=None):
    """(status, D, {m: table / Z as mpf}, Z as mpf, gs as mpf).  variant: a deliberately wrong restatement (the reference must notice those):
    'n_ceil' n = (t + 1) / 2, 'cmf_exclusive' the cmf without its own term, 'no_only_last' the full-overlap arm ignored."""
    import mpmath

    mp = mpmath.mp
    mp.dps = DPS
    counts = [m for m, _ in bins]
    D = len(counts)
    if t == 0:
        return Q_NO_KMERS, 0, {}, mp.mpf(0), mp.mpf(0)
    n = (t + 1) // 2 if variant == "n_ceil" else t // 2
    table = {}
    if counts[-1] == t and variant != "no_only_last":          # prob.rs:24-41, 105-119
        total = mp.binomial(t + n - 1, n)
        for m in counts:
            table[m] = mp.mpf(1) if m == t else mp.mpf(0) if m == 0 else mp.binomial(m + n - 1, n) / total
    else:
        if n == 0:
            return Q_NO_KMERS, D, {}, mp.mpf(0), mp.mpf(0)
        pmf = _pmf_rows(t, n, counts, mp)
        cmf = {}
        for m in counts:
            run, row = mp.mpf(0), []
            for i in range(n + 1):
                if variant == "cmf_exclusive":
                    row.append(run)
                    run += pmf[m][i]
                else:
                    run += pmf[m][i]
                    row.append(run)
            cmf[m] = row
        P = []
        for i in range(n + 1):                                 # prob.rs:62-73
            x = mp.mpf(1)
            for m, h in bins:
                x *= cmf[m][i] ** h
            P.append(x)
        for m in counts:                                       # prob.rs:74-90
            s = mp.mpf(0)
            for i in range(n + 1):
                if cmf[m][i] != 0 and P[i] != 0:
                    s += pmf[m][i] * P[i] / cmf[m][i]
            table[m] = s
    Z = sum((h * table[m] for m, h in bins), mp.mpf(0))        # prob.rs:97
    p = {m: table[m] / Z for m in counts}
    gs = mp.sqrt(sum((h * (p[m] - mp.mpf(1) / n_refs) ** 2 for m, h in bins), mp.mpf(0)))   # lineage.rs:86-90
    return Q_OK, D, p, Z, gs


@functools.lru_cache(maxsize=None)
def exact(case):
    status, D, p, Z, gs = exact_tables(case.t, case.bins, N_REFS)
    return Exact(status, D, {m: float(v) for m, v in p.items()}, float(Z), float(gs))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the CPU side: emulators and oracle on a case
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lnfact_cached(n):
    """The library's own ln-factorial table (rtx_debug_ln_factorial; needs no device): the emulators start from the numbers the kernels
    start from.  (The oracle's table differs from it in the last place of a quarter of its entries.)"""
    from raxtax_amd import _lib

    out = np.zeros(n, dtype=np.float64)
    rc = _lib.load().rtx_debug_ln_factorial(n, out.ctypes.data_as(_lib.f64p))
    assert rc == 0
    return out


def lnfact(t):
    return _lnfact_cached(4096 if 2 * t + 8 <= 4096 else 2 * t + 8)


def emul_table(emul, case, fn):
    """(rc, table / Z [t + 1], Z, gs, stats[4]) of emul_prob_table / emul_prob_lookup on the case's histogram."""
    t = case.t
    lf = lnfact(t)
    hist = case.hist()
    tz = np.zeros(t + 1)
    z, gs = C.c_double(), C.c_double()
    stats = np.zeros(4, dtype=np.uint64)
    f = getattr(emul, fn)
    f.restype = C.c_int
    rc = f(C.c_uint32(t), hist.ctypes.data_as(C.c_void_p), C.c_uint64(N_REFS), lf.ctypes.data_as(C.c_void_p), tz.ctypes.data_as(C.c_void_p),
           C.byref(z), C.byref(gs), stats.ctypes.data_as(C.c_void_p))
    return rc, tz, z.value, gs.value, [int(x) for x in stats]


def prune_threshold(emul, case):
    """(u, i* + 1) of emul_prune_threshold for the block of the case's 64 best references."""
    top = []
    for m, h in reversed(case.bins):
        top += [m] * min(h, 64 - len(top))
        if len(top) == 64:
            break
    hm = np.zeros(64, np.uint32)
    hm[: len(top)] = top
    lf = lnfact(case.t)
    u, i1 = C.c_uint32(), C.c_uint32()
    emul.emul_prune_threshold(C.c_uint32(case.t), C.c_uint64(case.n_refs), hm.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p),
                              C.c_uint32(TAB_TMAX), C.byref(u), C.byref(i1))
    return int(u.value), int(i1.value)


def emul_pruned(emul, case, u, i1):
    t = case.t
    lf = lnfact(t)
    hist = case.hist()
    tz = np.zeros(t + 1)
    z, gs = C.c_double(), C.c_double()
    emul.emul_prob_lookup_pruned.restype = C.c_int
    rc = emul.emul_prob_lookup_pruned(C.c_uint32(t), hist.ctypes.data_as(C.c_void_p), C.c_uint64(N_REFS), lf.ctypes.data_as(C.c_void_p),
                                      C.c_uint32(u), C.c_uint32(i1), tz.ctypes.data_as(C.c_void_p), C.byref(z), C.byref(gs))
    return rc, tz, z.value, gs.value


def oracle_table(oracle, case):
    """(status, table / Z [t + 1], Z) of the double-precision oracle (prob.rs restated in log space)."""
    sizes = np.repeat(np.array([m for m, _ in case.bins], np.uint16), [h for _, h in case.bins])
    try:
        table, z = oracle.prob_table(case.t, case.n, sizes)
    except ArithmeticError:
        return Q_NO_KMERS, None, 0.0
    return Q_OK, table / z, z


_Z_DEVS = {}


def z_deviations(case, emul, oracle):
    """Relative deviation of Z from the exact Z: (oracle, emul_prob_table, emul_prob_lookup)."""
    if case not in _Z_DEVS:
        ex = exact(case)
        devs = [abs(oracle_table(oracle, case)[2] - ex.z) / ex.z]
        for fn in ("emul_prob_table", "emul_prob_lookup"):
            rc, _, z, _, _ = emul_table(emul, case, fn)
            assert rc == 0
            devs.append(abs(z - ex.z) / ex.z)
        _Z_DEVS[case] = tuple(devs)
    return _Z_DEVS[case]


def z_margin(case, emul, oracle):
    """The relative deviation the device's Z may show from the exact Z: four times the largest of the oracle's and the two emulators' for
    the case (floor 1e-12)."""
    if exact(case).status != Q_OK:
        return None
    return max(Z_FACTOR * max(z_deviations(case, emul, oracle)), Z_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------------------------
# compare
# ---------------------------------------------------------------------------------------------------------------------------------------
def compare(case, status, ndist, tz, z, gs, label, z_tol=None, check_ndist=True):
    """One result (table / Z as an array over the counts, NaN or anything at absent ones) against the exact reference.  Returns the largest
    deviation of table / Z at a present count."""
    ex = exact(case)
    assert int(status) == ex.status, f"{label} {case.name}: status {status}, exact {ex.status}"
    if check_ndist:
        assert int(ndist) == ex.ndist, f"{label} {case.name}: {ndist} distinct counts, exact {ex.ndist}"
    if ex.status != Q_OK:
        return 0.0
    worst = 0.0
    for m, _ in case.bins:
        v = float(tz[m])
        assert v == v, f"{label} {case.name}: table / Z of the present count {m} was never written"
        worst = max(worst, abs(v - ex.p[m]))
    tol = case.tol or TOL
    assert worst <= tol, f"{label} {case.name}: table / Z off by {worst:.3e} (> {tol})"
    assert abs(float(gs) - ex.gs) <= tol, f"{label} {case.name}: global signal off by {abs(float(gs) - ex.gs):.3e}"
    if z_tol is not None:
        dz = abs(float(z) - ex.z) / ex.z
        assert dz <= z_tol, f"{label} {case.name}: Z off by {dz:.3e} relative (> {z_tol:.3e})"
    return worst


def compare_pruned(case, u, tz, tz_emul, label):
    """A pruned run (threshold u) against the exact values of the original histogram and against emul_prob_lookup_pruned."""
    ex = exact(case)
    assert ex.status == Q_OK
    worst = worst_e = 0.0
    for m, _ in case.bins:
        v = float(tz[m])
        assert v == v, f"{label} {case.name}: table / Z of the present count {m} was never written"
        if m > u:
            worst = max(worst, abs(v - ex.p[m]))
        elif m >= 1:
            assert v == 0.0, f"{label} {case.name}: count {m} <= threshold {u} holds {v}"
        if m > u:
            worst_e = max(worst_e, abs(v - float(tz_emul[m])))
    assert worst <= TOL_PRUNED, f"{label} {case.name}: pruned table / Z off by {worst:.3e}"
    assert worst_e <= TOL, f"{label} {case.name}: pruned table / Z {worst_e:.3e} from emul_prob_lookup_pruned"
    return worst


def dropped_mass(case, u):
    """What the references with a count up to u hold together in the exact reference."""
    ex = exact(case)
    return sum(h * ex.p[m] for m, h in case.bins if m <= u)


# ---------------------------------------------------------------------------------------------------------------------------------------
# fuzz (GPU file): seeded random histograms
# ---------------------------------------------------------------------------------------------------------------------------------------
CAP = 120_000        # D (n + 1) per case, except where a case says otherwise


def fuzz_cases(n_cases=40, seed=20261019):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_cases:
        t = int(rng.integers(2, 701))
        kind = int(rng.integers(0, 4))
        nb = int(rng.integers(1, 5)) if kind == 0 else int(rng.integers(60, 71)) if kind == 1 else int(rng.integers(120, 141)) if kind == 2 else max(t // 2, 1)
        nb = min(nb, t)                                       # counts 0 .. t - 1
        if (nb + 1) * (t // 2 + 1) > CAP:
            continue
        ms = rng.choice(t, nb, replace=False)
        bins = {int(m): int(round(10 ** rng.uniform(0, 6))) for m in ms}
        if rng.random() < 0.5 and t >= 8:                     # a top relative
            bins[int(rng.integers(3 * t // 4, t))] = int(rng.integers(1, 4))
        out.append(_case(f"fuzz{len(out)}", t, bins, "seeded random histogram"))
    return out

"""The cases of tests/prob_common.py on the CPU: the exact (mpmath) reference against the double-precision oracle and against the three
emulators of the probability kernels, the structure every case claims to exercise, and the reference's own sensitivity.

This is where a CPU-side bug of the arithmetic would show first and where the margins of Z are measured (printed: run with -s); the
device kernels meet the same cases in tests/test_gpu_prob_hist.py."""
import numpy as np
import pytest

import prob_common as pc

@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_emulators_and_oracle_against_the_exact_reference(case, emul, oracle):
    ex = pc.exact(case)
    st, p, z = pc.oracle_table(oracle, case)
    assert st == ex.status
    if st == pc.Q_OK:
        w = pc.compare(case, st, case.D, p, z, np.sqrt(sum(h * (p[m] - 1.0 / pc.N_REFS) ** 2 for m, h in case.bins)), "oracle", check_ndist=False)
        print(f"{case.name}: oracle {w:.2e}", end="")
    for fn in ("emul_prob_table", "emul_prob_lookup"):
        if fn == "emul_prob_lookup" and case.t > pc.TAB_TMAX:
            continue
        rc, tz, z, gs, _ = pc.emul_table(emul, case, fn)
        assert rc == (0 if ex.status == pc.Q_OK else 1), (fn, case.name)
        if rc == 0:
            w = pc.compare(case, pc.Q_OK, case.D, tz, z, gs, fn, check_ndist=False)
            print(f", {fn} {w:.2e}", end="")
    if ex.status == pc.Q_OK:
        print(f", Z deviations (oracle, table, lookup) {['%.2e' % d for d in pc.z_deviations(case, emul, oracle)]}")


def test_t1_with_full_overlaps_is_exact(emul):
    case = pc.BY_NAME["t1_full"]
    ex = pc.exact(case)
    assert ex.z == 3.0 and ex.p[1] == 1.0 / 3.0 and ex.p[0] == 0.0
    for fn in ("emul_prob_table", "emul_prob_lookup"):
        rc, tz, z, gs, _ = pc.emul_table(emul, case, fn)
        assert rc == 0 and z == 3.0 and tz[1] == 1.0 / 3.0 and tz[0] == 0.0


def test_no_hits_gives_the_uniform_value(emul):
    case = pc.BY_NAME["t9_no_hits"]
    assert pc.exact(case).p[0] == 1.0 / 7.0 and case.D == 1 and case.n_refs == 7


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.t >= 2], ids=lambda c: c.name)
def test_case_exercises_what_it_claims(case, emul):
    """The structure a case's note promises, read off the emulators' stats: D, the rows still moving at i_lo, the slices in which rows move
    last, n - i_lo, the groups the recurrence kernel skips."""
    rc, _, _, _, rec = pc.emul_table(emul, case, "emul_prob_table")
    assert rc == 0
    full = case.bins[-1][0] == case.t
    if case.t <= pc.TAB_TMAX and not full:
        rc, _, _, _, lk = pc.emul_table(emul, case, "emul_prob_lookup")
        assert rc == 0
        slices = tuple(s for s in range(16) if lk[3] >> s & 1)
        if case.live is not None:
            assert lk[0] == case.live, f"{case.name}: {lk[0]} live rows, promised {case.live}"
        if case.slices is not None:
            assert slices == case.slices, f"{case.name}: rows move last in slices {slices}, promised {case.slices}"
        if case.span is not None:
            assert case.n - lk[2] == case.span, f"{case.name}: n - i_lo = {case.n - lk[2]}, promised {case.span}"
        assert lk[2] == rec[3], "the two kernels start at the same i_lo"
    if case.skipped is not None:
        assert rec[2] == case.skipped, f"{case.name}: {rec[2]} groups skipped, promised {case.skipped}"


def test_the_case_list_covers_the_structure_of_the_kernels(emul):
    names = set(pc.BY_NAME)
    assert {f"d{d}" for d in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129)} <= names
    assert {f"span{s}" for s in (63, 64, 65, 127, 128, 129)} <= names
    assert {f"flush_t{t}" for t in range(126, 132)} <= names
    assert {pc.BY_NAME[f"flush_t{t}"].n for t in range(126, 132)} == {63, 64, 65}
    assert pc.BY_NAME["d129"].D == 129 and (129 + 63) // 64 == 3          # wave 0 of the recurrence kernel takes groups 0 and 2
    assert pc.BY_NAME["full_all_counts_401"].D == 402
    last = {c.name: max(c.slices) for c in pc.CASES if c.slices}
    assert {last[f"slice{s}_640"] for s in (0, 1, 2, 3)} == {0, 1, 2, 3} and last["slice4_1100"] == 4
    # the furthest slice a single row reaches: no top count at t = 640 gets past slice 3, none at t = 1100 past slice 4
    for t, far in ((640, 3), (1100, 4)):
        reach = 0
        for top in range(1, t, 7):
            reach = max(reach, pc.emul_table(emul, pc._case("probe", t, {top: 1, 0: 1}), "emul_prob_lookup")[4][3].bit_length() - 1)
        assert reach == far
    for c in pc.CASES:
        assert c.D * (c.n + 1) <= pc.CAP or c.name == "all_counts_640", c.name


PRUNED = [c for c in pc.CASES if c.pruned]


@pytest.mark.parametrize("case", PRUNED, ids=lambda c: c.name)
def test_pruned_lookup_emulator_against_the_exact_reference(case, emul):
    u, i1 = pc.prune_threshold(emul, case)
    assert u > 0, f"{case.name}: no threshold -- not a pruned case"
    assert any(0 < m <= u for m, _ in case.bins), f"{case.name}: the threshold {u} drops nothing"
    assert pc.dropped_mass(case, u) < 1e-9
    rc, tz, z, gs = pc.emul_pruned(emul, case, u, i1)
    assert rc == 0
    w = pc.compare_pruned(case, u, tz, tz, "emul_prob_lookup_pruned")
    print(f"{case.name}: u = {u}, i1 = {i1}, pruned emulator {w:.2e}, dropped mass {pc.dropped_mass(case, u):.2e}")


def test_there_are_about_eight_pruned_cases():
    assert 7 <= len(PRUNED) <= 10


@pytest.mark.parametrize("variant", ["n_ceil", "cmf_exclusive", "no_only_last"])
def test_the_reference_notices_a_wrong_restatement(variant):
    """Each perturbed restatement moves some case by more than 1e-9: the exact reference is not insensitive to what it restates."""
    probes = {"n_ceil": ["t3", "flush_t127", "span65"], "cmf_exclusive": ["t2", "tied_tops", "flush_t126"], "no_only_last": ["full_beside_one", "t1_full"]}[variant]
    worst = 0.0
    for name in probes:
        case = pc.BY_NAME[name]
        ex = pc.exact(case)
        try:
            st, _, p, _, _ = pc.exact_tables(case.t, case.bins, pc.N_REFS, variant=variant)
        except ZeroDivisionError:
            worst = 1.0            # the wrong restatement does not even normalise
            continue
        if st != ex.status:
            worst = 1.0
            continue
        worst = max([worst] + [abs(float(p[m]) - ex.p[m]) for m, _ in case.bins])
    assert worst > 1e-9, variant

"""The probability kernels of the device on injected histograms (rtx_debug_prob_hist) against exact sums (tests/prob_common.py).

prob_lookup_kernel (kernel 0), prob_table_kernel with its arrays in LDS (1) and in global memory (2) each take the whole case list in ONE
launch -- every t of the list, t = 0 and t = 1 between valid queries, one row stride -- so that prob_order_kernel, the order indirection,
hstride and the q / gq indexing are part of what is tested; a second launch carries the cases twice over in a shuffled order and must
reproduce the first bit for bit.  The handle holds a dozen references; the histograms stand for up to five million.

Tolerances are those of prob_common.py: 1e-11 on table / Z and the global signal against the 50-digit reference, status and number of
distinct counts equal, Z within four times the deviation the CPU implementations show for the case; pruned runs within 1e-9 of the exact
values of the unpruned histogram.  The largest deviation per kernel is printed (-s)."""
import time

import numpy as np
import pytest

import prob_common as pc
import raxtax_amd as rx
from raxtax_amd import _lib, synth

pytestmark = pytest.mark.gpu

KERNELS = {0: "lookup", 1: "recurrence in LDS", 2: "recurrence in global memory"}


def _accepted(kernel, cases):
    return [c for c in cases if kernel != 0 or c.t <= pc.TAB_TMAX]


def _launch(index, kernel, cases, thr=None, i1=None):
    stride = max(c.t for c in cases) + 8
    ts = np.array([c.t for c in cases], np.uint32)
    hists = np.stack([c.hist(stride) for c in cases])
    return index.debug_prob_hist(ts, hists, pc.N_REFS, kernel, thr, i1)


def _check(out, cases, label, emul, oracle):
    worst = (0.0, "")
    for q, c in enumerate(cases):
        w = pc.compare(c, out["status"][q], out["ndist"][q], out["table_z"][q], out["z"][q], out["gs"][q], label, z_tol=pc.z_margin(c, emul, oracle))
        worst = max(worst, (w, c.name))
        absent = np.ones(out["table_z"].shape[1], bool)
        absent[[m for m, _ in c.bins]] = False
        assert np.isnan(out["table_z"][q][absent]).all(), f"{label} {c.name}: an entry of an absent count was written"
    return worst


class World:
    def __init__(self):
        db = synth.make_db(12, fanouts=(1, 1, 2, 2, 3, 1))
        self.qs = synth.make_queries(db, 6, exact_frac=0.2)
        self.index = rx.Index(rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off))

    def classify(self):
        res = self.index.classify(self.qs.bases, self.qs.base_off)
        return (res.status.copy(), res.row_off.copy(), res.row_lineage.copy(), res.row_conf.copy(), res.row_local_signal.copy(), res.global_signal.copy())


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_every_case_in_one_launch_and_again_shuffled(world, emul, oracle, kernel):
    cases = _accepted(kernel, pc.CASES)
    assert {0, 1} <= {c.t for c in cases} and cases[0].t == 0 and len({c.t for c in cases}) > 15
    t0 = time.perf_counter()
    out = _launch(world.index, kernel, cases)
    t1 = time.perf_counter()
    worst = _check(out, cases, KERNELS[kernel], emul, oracle)
    # the cases twice over in a shuffled order: same bits, whatever the slot, the neighbours and the processing order
    order = np.random.default_rng(7 + kernel).permutation(2 * len(cases)) % len(cases)
    t2 = time.perf_counter()
    again = _launch(world.index, kernel, [cases[j] for j in order])
    t3 = time.perf_counter()
    for q, j in enumerate(order):
        c = cases[j]
        for key in ("z", "gs", "status", "ndist"):
            assert out[key][j].tobytes() == again[key][q].tobytes(), f"{KERNELS[kernel]} {c.name}: {key} depends on the slot"
        ms = [m for m, _ in c.bins]
        w = out["table_z"].shape[1]
        assert out["table_z"][j][ms].tobytes() == again["table_z"][q][:w][ms].tobytes(), f"{KERNELS[kernel]} {c.name}: table / Z depends on the slot"
    print(f"{KERNELS[kernel]}: {len(cases)} cases, largest deviation of table / Z {worst[0]:.3e} ({worst[1]}); first launch {t1 - t0:.2f} s"
          f"{' (builds the memoised tables up to t = 1100)' if kernel == 0 else ''}, shuffled launch of {len(order)} {t3 - t2:.2f} s")


def test_pruned_cases_through_the_lookup(world, emul):
    cases = [c for c in pc.CASES if c.pruned]
    thr = [pc.prune_threshold(emul, c) for c in cases]
    # between them a query without a threshold: prune_thr = 0 leaves it the full computation
    plain = pc.BY_NAME["d33"]
    cases, thr = cases + [plain], thr + [(0, 0)]
    out = _launch(world.index, 0, cases, [u for u, _ in thr], [i for _, i in thr])
    worst = (0.0, "")
    for q, (c, (u, i1)) in enumerate(zip(cases, thr)):
        assert int(out["status"][q]) == pc.Q_OK
        if u == 0:
            pc.compare(c, out["status"][q], out["ndist"][q], out["table_z"][q], out["z"][q], out["gs"][q], "lookup beside pruned queries")
            continue
        rc, tz_e, _, _ = pc.emul_pruned(emul, c, u, i1)
        assert rc == 0
        tz = out["table_z"][q].copy()
        assert all(tz[m] == 0.0 for m in range(1, min(u, c.t) + 1)), f"{c.name}: an entry up to the threshold {u} is not 0"
        worst = max(worst, (pc.compare_pruned(c, u, tz, tz_e, "pruned lookup"), c.name))
        # the distinct counts of a pruned query: those above the threshold, and bin 0 (which takes the others in)
        assert int(out["ndist"][q]) == 1 + sum(1 for m, _ in c.bins if m > u)
    print(f"pruned lookup: {len(cases) - 1} cases, largest deviation from the exact unpruned values {worst[0]:.3e} ({worst[1]})")


def test_classify_is_unchanged_by_the_tap(world):
    before = world.classify()
    cases = [pc.BY_NAME[n] for n in ("t0", "d17", "t1_full", "slice3_640", "flush_t128")]
    for kernel in (0, 1, 2):
        _launch(world.index, kernel, cases)
    after = world.classify()
    assert int(before[1][-1]) >= 1
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_lookup_refuses_reads_beyond_its_tables(world):
    with pytest.raises(rx.RtxError) as e:
        _launch(world.index, 0, [pc.BY_NAME["d1"], pc.BY_NAME["long_2600"]])
    assert e.value.code == _lib.RTX_ERR_TOO_LONG


FUZZ = pc.fuzz_cases()


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_fuzz_histograms(world, emul, oracle, kernel):
    assert len(FUZZ) == 40 and all((c.D) * (c.n + 1) <= pc.CAP and 2 <= c.t <= 700 for c in FUZZ)
    out = _launch(world.index, kernel, FUZZ)
    worst = _check(out, FUZZ, f"fuzz, {KERNELS[kernel]}", emul, oracle)
    print(f"fuzz, {KERNELS[kernel]}: {len(FUZZ)} histograms, largest deviation of table / Z {worst[0]:.3e} ({worst[1]})")

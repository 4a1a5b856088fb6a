"""The consensus taxonomy of the OTUs on the device (rtx_otutax.hip): rx.otu_taxonomy against the brute force of otutax_common.py and against
rx.otu_taxonomy_host, field by field, with no tolerance.  The crafted cases are those of test_otutax_cpu.py, where the brute force alone shows
what each of them was built to show; here the plan of the device is held to the sizes as well."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib
from otutax_common import PERMUTED, Case, assert_tax, brute, cases, check_expected, permutation, random_world, refusals, world

pytestmark = pytest.mark.gpu

# packed waves and workgroups of the plan: consecutive OTUs of at most 64 members share a wave while their members total at most 64
PLAN = {"singletons_64": (1, 0), "singletons_65": (2, 0), "sizes_63_2": (2, 0), "sizes_64_65": (1, 1), "sizes_256_257_1025": (0, 3), "stops": (1, 0),
        "heavy_one": (0, 1), "heavy_one_50": (0, 1), "threshold_51": (0, 1), "threshold_51_packed": (1, 0), "threshold_100_packed": (1, 0), "threshold_100_packed_short": (1, 0), "light_many": (0, 1), "no_majority": (0, 1), "wide_sums": (1, 1), "seed_rel": (1, 4)}


@pytest.fixture(scope="module")
def wanted():
    """the brute force of every case, once"""
    out = {}
    for name, (case, agree, _) in cases().items():
        otus, lin = case.arrays()
        out[name] = (otus, lin, brute(case.w.parent, otus, lin, agree))
    return out


@pytest.mark.parametrize("name", sorted(cases()))
def test_device_against_the_brute_force_and_the_host(name, wanted):
    case, agree, expected = cases()[name]
    otus, lin, want = wanted[name]
    got = rx.otu_taxonomy(case.w.tree, otus, lin, agree=agree)
    assert_tax(got, want, name)
    assert_tax(got, rx.otu_taxonomy_host(case.w.tree, otus, lin, agree=agree), name + " against the host")
    check_expected(name, got, expected)
    assert got.agree_pct == agree and got.stride == max(1, int(lin.L.max())) and all(t >= 0 for t in got.seconds) and got.seconds[2] > 0
    if name in PLAN:
        assert (got.packed_waves, got.big_otus) == PLAN[name]
    if name in PERMUTED:   # the ranks permuted by a fixed permutation: other lanes, other merge orders, the same result
        otus2, lin2 = case.arrays(permutation(len(otus[0])))
        assert_tax(rx.otu_taxonomy(case.w.tree, otus2, lin2, agree=agree), got, name + " permuted")


def test_small_otus_permuted_inside_a_packed_wave():
    """the three summary cases cut down to a wave: the majority in one heavy member of 40, in 21 light ones of 22, and in nobody of 40; the
    first two share a wave (62 members), so a segment boundary falls inside it"""
    c = Case()
    names = [x for x in c.w.names if not x.startswith("J") and c.w.depth[c.w.node(x)] <= 4]
    for i in range(39):
        c.add(0, 1, names[i % len(names)])
    c.add(0, 41, "J,K,L")
    c.add(1, 19, "A,B,C").add(1, 1, "J,K,M,N", n=21)
    for i in range(40):
        c.add(2, 1 + i % 3, ["A,B,C", "J,K,L", "Q,R,S", "X,Y,Z", "c0,c1"][i % 5])
    otus, lin = c.arrays()
    want = brute(c.w.parent, otus, lin)
    assert want["depth"].tolist() == [3, 4, 0]
    got = rx.otu_taxonomy(c.w.tree, otus, lin)
    assert_tax(got, want, "packed")
    assert (got.packed_waves, got.big_otus) == (2, 0)
    otus2, lin2 = c.arrays(permutation(len(otus[0])))
    assert_tax(rx.otu_taxonomy(c.w.tree, otus2, lin2), got, "packed, permuted")


@pytest.mark.parametrize("name", sorted(refusals()))
def test_device_refuses_on_the_host(name):
    otus, lin, agree, parent = refusals()[name]
    with pytest.raises(rx.RtxError) as e:
        rx.otu_taxonomy(world().tree if parent is None else parent, tuple(otus), lin, agree=agree)
    assert e.value.code == _lib.RTX_ERR_INVALID and "rtx_otu_taxonomy:" in str(e.value)


def test_random_world():
    case = random_world()
    otus, lin = case.arrays()
    want = brute(case.w.parent, otus, lin)
    got = rx.otu_taxonomy(case.w.tree, otus, lin)
    assert_tax(got, want, "random")
    assert got.big_otus == int((want["members"] > 64).sum()) >= 3 and got.packed_waves >= 20
    assert_tax(rx.otu_taxonomy(case.w.tree, otus, lin, agree=75), brute(case.w.parent, otus, lin, 75), "random at 75")
    assert_tax(rx.otu_taxonomy(case.w.tree, otus, lin, agree=100), rx.otu_taxonomy_host(case.w.tree, otus, lin, agree=100), "random at 100")


def test_no_rows_and_no_device():
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    lin = rx.Lineages(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros((0, 4), np.uint8))
    got = rx.otu_taxonomy(world().tree, none, lin)
    assert got.n_otus == 0 and got.n_rows == 0 and got.packed_waves == 0
    case, _, _ = cases()["even_split"]
    otus, lin = case.arrays()
    with pytest.raises(rx.RtxError) as e:
        rx.otu_taxonomy(case.w.tree, otus, lin, device=1 << 20)
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE

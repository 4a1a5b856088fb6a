"""The per-sample counters beside the taxon profile (rtx_index_profile_begin_samples, rtx_batch_prefetch_samples, profile_samples_kernel).
The expectation comes from code that exists without them: the `direct` and `totals` that profile_begin / profile_read of a plain handle
give when the reads of each sample are run alone.  Integers, held for equality."""
import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from demux_common import NONE, concat

pytestmark = pytest.mark.gpu
S = 5            # samples; sample 3 receives no read
CUTOFF = 0.8


@pytest.fixture(scope="module")
def fixture():
    """280 reads against 400 references: a sample per read (every seventh read none), in an order that mixes the samples within every wave;
    the reads of sample 0 and of sample 1 come from different halves of the database."""
    db = synth.make_db(400)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    qs = synth.make_queries(db, 280, seed=43)
    rng = np.random.default_rng(45)
    reads = [qs.seq(i).copy() for i in range(280)]
    reads[5] = np.zeros(0, np.uint8)                                     # unclassifiable
    reads[6] = (1 << rng.integers(0, 4, 300)).astype(np.uint8)          # unrelated: most likely unclassified
    reads[12] = db.seq(77).copy()                                        # an exact match: the override
    sample = np.array([NONE if i % 7 == 0 else (0, 1, 2, 4)[i % 4] for i in range(280)], np.uint32)
    sample[[5, 6, 12]] = [0, 1, 2]
    assert 3 not in sample and (sample == NONE).sum() == 40
    return tree, reads, sample


def profile_alone(tree, reads, weights=None, **kw):
    """The profile of a plain handle that sees these reads alone."""
    index = rx.Index(tree, **kw)
    index.profile_begin(CUTOFF)
    if len(reads):
        if weights is not None:
            index.prefetch_weights(weights)
        index.classify(*concat(reads))
    prof = index.profile_read()
    index.profile_end()
    return prof


@pytest.fixture(scope="module")
def alone(fixture):
    tree, reads, sample = fixture
    return [profile_alone(tree, [r for r, s in zip(reads, sample) if s == k]) for k in list(range(S)) + [NONE]]


def assert_per_sample(got, want, what):
    for k in range(S):
        assert np.array_equal(got.direct[k], want[k].direct), f"{what}: direct of sample {k} differs at {np.nonzero(got.direct[k] != want[k].direct)[0][:8]}"
        assert np.array_equal(got.totals[k], want[k].totals), f"{what}: totals of sample {k}: {got.totals[k]} against {want[k].totals}"


def test_per_sample_counts_equal_each_sample_run_alone(fixture, alone):
    tree, reads, sample = fixture
    # the expectation itself: two samples with different non-zero nodes, one all-zero sample, every kind of query
    nz = [set(np.nonzero(a.direct)[0]) for a in alone[:S]]
    assert nz[0] and nz[1] and nz[0] != nz[1] and not nz[3] and not alone[3].totals.any()
    assert all(int(sum(a.totals[k] for a in alone[:S])) > 0 for k in range(4))
    plain = profile_alone(tree, reads)
    index = rx.Index(tree)
    index.profile_begin(CUTOFF, n_samples=S)
    index.prefetch_samples(sample)
    index.classify(*concat(reads))
    got = index.profile_read_samples()
    assert got.direct.shape == (S, len(plain.direct)) and got.totals.shape == (S, 4) and (got.cutoff, got.flags) == (80, 0)
    assert_per_sample(got, alone, "one batch")
    # the global counters of the same profile are what they are without the per-sample path
    glob = index.profile_read()
    for name in ("clade", "direct", "conf_sum", "totals"):
        assert np.array_equal(getattr(glob, name), getattr(plain, name)), name
    # every read is in one sample or in none
    assert np.array_equal(got.direct.sum(axis=0) + alone[S].direct, glob.direct)
    assert np.array_equal(got.totals.sum(axis=0) + alone[S].totals, glob.totals)
    # a second download of one run adds nothing
    index.profile_reset()
    assert not index.profile_read_samples().direct.any() and not index.profile_read_samples().totals.any()
    index.prefetch_samples(sample)
    index.upload(*concat(reads))
    index.run()
    index.download()
    index.download()
    assert_per_sample(index.profile_read_samples(), alone, "second download")
    # a batch with nothing staged, and one whose count does not match, count in no sample
    index.profile_reset()
    index.classify(*concat(reads))
    index.prefetch_samples(sample[:100])
    index.classify(*concat(reads))
    z = index.profile_read_samples()
    assert not z.direct.any() and not z.totals.any() and int(index.profile_read().totals[0]) == 2 * len(reads)
    # several batches add up: the reads in three pieces of odd sizes
    index.profile_reset()
    for a, b in ((0, 65), (65, 129), (129, 280)):
        index.prefetch_samples(sample[a:b])
        index.classify(*concat(reads[a:b]))
    assert_per_sample(index.profile_read_samples(), alone, "three batches")
    index.profile_end()
    with pytest.raises(rx.RtxError) as e:
        index.profile_read_samples()
    assert e.value.code == _lib.RTX_ERR_STATE


def test_both_strands_index_by_the_callers_query(fixture, alone):
    tree, reads, sample = fixture
    flipped = [rx.api.revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    index = rx.Index(tree, strand="both")
    index.profile_begin(CUTOFF, n_samples=S)
    index.prefetch_samples(sample)
    index.classify(*concat(flipped))
    got = index.profile_read_samples()
    want = [profile_alone(tree, [r for r, s in zip(flipped, sample) if s == k], strand="both") for k in range(S)]
    assert_per_sample(got, want, "both strands")
    index.profile_end()


def test_weights_scale_the_counts(fixture):
    tree, reads, sample = fixture
    weights = np.array([(i * 7) % 5 for i in range(len(reads))], np.uint32)      # some 0: those reads do not count
    want = [profile_alone(tree, [r for r, s in zip(reads, sample) if s == k], weights[sample == k]) for k in range(S)]
    assert any((w.direct > 4).any() for w in want)
    index = rx.Index(tree)
    index.profile_begin(CUTOFF, n_samples=S)
    index.prefetch_weights(weights)
    index.prefetch_samples(sample)
    index.classify(*concat(reads))
    assert_per_sample(index.profile_read_samples(), want, "weights")
    index.profile_end()


def test_refusals(fixture):
    tree, reads, sample = fixture
    index = rx.Index(tree)
    n_nodes = len(tree.nodes()["parent"])
    too_many = _lib.RTX_PROFILE_MAX_SAMPLE_COUNTERS // n_nodes + 1
    for n in (0, too_many):
        with pytest.raises(rx.RtxError) as e:
            index.profile_begin(CUTOFF, n_samples=n)
        assert e.value.code == _lib.RTX_ERR_INVALID
    assert "RTX_PROFILE_MAX_SAMPLE_COUNTERS" in str(e.value)
    with pytest.raises(rx.RtxError) as e:                               # no profile at all, then a profile without samples
        index.prefetch_samples(sample)
    assert e.value.code == _lib.RTX_ERR_STATE
    index.profile_begin(CUTOFF)
    for call in (lambda: index.prefetch_samples(sample), index.profile_read_samples):
        with pytest.raises(rx.RtxError) as e:
            call()
        assert e.value.code == _lib.RTX_ERR_STATE
    index.profile_end()
    index.profile_begin(CUTOFF, n_samples=S)
    bad = sample.copy()
    bad[17] = S
    with pytest.raises(rx.RtxError) as e:
        index.prefetch_samples(bad)
    assert e.value.code == _lib.RTX_ERR_INVALID
    index.classify(*concat(reads))                                       # the refused samples were not staged
    assert not index.profile_read_samples().totals.any()
    index.profile_end()


def test_merge_of_two_handles_equals_one_handle(fixture, alone):
    tree, reads, sample = fixture
    parts = []
    for a, b in ((0, 150), (150, 280)):
        index = rx.Index(tree)
        index.profile_begin(CUTOFF, n_samples=S)
        index.prefetch_samples(sample[a:b])
        index.classify(*concat(reads[a:b]))
        parts.append(index.profile_read_samples())
        index.profile_end()
    merged = rx.sample_profile_merge(parts)
    assert_per_sample(merged, alone, "merge")
    other = rx.SampleProfile(parts[1].cutoff, parts[1].flags, parts[1].direct[:S - 1], parts[1].totals[:S - 1])
    with pytest.raises(rx.RtxError) as e:
        rx.sample_profile_merge([parts[0], other])
    assert e.value.code == _lib.RTX_ERR_INVALID
    # the table of the merged counters: a column per sample, the all-zero sample included
    names = [f"s{k}" for k in range(S)]
    text = rx.sample_table_text(tree, names, merged)
    lines = text.split("\n")
    assert lines[0] == f"# cutoff=0.80\tsamples={S}" and lines[5] == "depth\ttaxon\tlineage\t" + "\t".join(names) and text.endswith("\n")
    assert lines[1] == "# queries\t" + "\t".join(str(int(a.totals[0])) for a in alone[:S])
    by_lineage = {l.split("\t")[2]: l.split("\t")[3:] for l in lines[6:-1]}
    for k in range(S):                                                   # the cells are the clade counts the plain profile of that sample has
        ref = rx.profile_text(tree, alone[k]).split("\n")[2:-1]
        assert {l.split("\t")[6]: l.split("\t")[0] for l in ref} == {lin: c[k] for lin, c in by_lineage.items() if c[k] != "0"}

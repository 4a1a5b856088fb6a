"""RTX_OPT_DEVICE_TEXT (Index(device_text=True)): rtx_raxtax and rtx_raxtax_multi take the lines of their chunks from the device
(rtx_text.hip).  The messages a sender receives are the same as with the host formatter: over chunks enqueued ahead of one another, with
run-aheads abandoned and chunks repeated (RTX_OPT_RUN_AHEAD = 2), on two handles of one GPU, with and without `.tsv`, in every flag mode."""
from pathlib import Path

import pytest

import raxtax_amd as rx
from raxtax_amd import synth

pytestmark = pytest.mark.gpu

FASTA = Path(__file__).resolve().parent / "golden" / "diptera_queries.fasta"


def _messages(index, queries, chunk, tsv, skip=False, raw=False):
    got = []
    rx.raxtax(queries, index, skip, raw, chunk, lambda l, o, t: got.append((l, o, t)), tsv)
    return got


def _set_text(index, on):
    rx._lib.check(index._lib.rtx_index_set_option(index._h, 24, int(on)))


@pytest.fixture(scope="module")
def synthetic():
    db = synth.make_db(60_000)
    qs = synth.make_queries(db, 100_000, seed=11)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    queries = [(qs.labels[i], qs.bases[qs.base_off[i]:qs.base_off[i + 1]]) for i in range(len(qs.labels))]
    return tree, queries


@pytest.mark.parametrize("aid", [1, 2])
def test_chunks_enqueued_ahead_send_the_same_messages(synthetic, aid):
    tree, queries = synthetic
    index = rx.Index(tree, device=0)
    assert index.prune_verdict[0]                                # pruned, two streams: the shape that runs ahead
    rx._lib.check(index._lib.rtx_index_set_option(index._h, 23, aid))
    chunk = 34_000                                               # three chunks of two sub-batches or more
    for tsv in (True, False):
        _set_text(index, False)
        host = _messages(index, queries, chunk, tsv)
        _set_text(index, True)
        before = index.run_ahead_stats
        dev = _messages(index, queries, chunk, tsv)
        ahead, abandoned = (a - b for a, b in zip(index.run_ahead_stats, before))
        assert len(dev) == len(queries) and dev == host, tsv
        assert all((t is not None) == tsv for _, _, t in dev)
        assert ahead >= 1, (ahead, abandoned)
        assert abandoned >= 1 or aid == 1, (ahead, abandoned)   # (aid 2: a chunk forced to run again, its text with it)
    rx._lib.check(index._lib.rtx_index_set_option(index._h, 23, 0))


def test_two_handles_of_one_gpu(synthetic):
    tree, queries = synthetic
    queries = queries[:40_000]
    plain = rx.Index(tree, device=0)
    host = _messages(plain, queries, 10_000, True)
    del plain
    handles = [rx.Index(tree, device=0, device_text=True), rx.Index(tree, device=0, device_text=True)]
    assert _messages(handles, queries, 10_000, True) == host


@pytest.mark.parametrize("skip,raw", [(False, False), (True, False), (False, True)])
def test_real_composition_in_every_flag_mode(skip, raw):
    text = FASTA.read_text()
    tree = rx.parse_reference_fasta_str(text)
    queries = rx.parse_query_fasta_str(text)
    index = rx.Index(tree)
    host = _messages(index, queries, 3000, True, skip, raw)
    _set_text(index, True)
    assert _messages(index, queries, 3000, True, skip, raw) == host

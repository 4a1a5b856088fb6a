"""Result text formatted on the device (rtx_text.hip: rtx_index_text_setup, rtx_batch_prefetch_labels, rtx_batch_text; Index.classify_text):
for every query the `.out` and `.tsv` text equals, byte for byte, what rtx_format_query prints for the same view, label, bases and exact
matches -- real composition with the override, the pruned path over many tiles, long reads and queries without result, deep lineages, long
and non-ASCII labels, exact ids passed in and looked up on the device, and batches enqueued ahead (RTX_OPT_RUN_AHEAD)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib, synth
from raxtax_amd._lib import ptr, u8p, u32p

pytestmark = pytest.mark.gpu

FASTA = Path(__file__).resolve().parent / "golden" / "diptera_queries.fasta"
_CAP = 1 << 22
_BUF = [C.create_string_buffer(_CAP), C.create_string_buffer(_CAP)]


def _flat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if len(seqs) else np.zeros(1, np.uint8)).astype(np.uint8), off


def _host_texts(index, labels, bases, base_off, ex_ids, ex_off, flags, tsv):
    """rtx_format_query over the last download, query by query (the reference of the device text)."""
    lib = _lib.load()
    v = index._view
    status = np.ctypeslib.as_array(v.status, shape=(v.n_queries,))
    out, tv, n_over = [], [], 0
    tl = C.c_int64()
    one = np.zeros(1, np.uint8)
    for q in range(v.n_queries):
        if status[q] != 0:
            out.append("")
            tv.append("")
            continue
        s = bases[int(base_off[q]):int(base_off[q + 1])]
        ids = ex_ids[int(ex_off[q]):int(ex_off[q + 1])] if ex_off is not None else np.zeros(0, np.uint32)
        n_over += len(ids) == 1
        idp = np.ascontiguousarray(ids if len(ids) else np.zeros(1, np.uint32), np.uint32)
        lab = labels[q].encode() if isinstance(labels[q], str) else labels[q]
        n = lib.rtx_format_query(index.tree._h, C.byref(v), q, lab, ptr(np.ascontiguousarray(s) if len(s) else one, u8p), len(s), ptr(idp, u32p),
                                 len(ids), flags, _BUF[0], _CAP, _BUF[1] if tsv else None, _CAP if tsv else 0, C.byref(tl))
        _lib.check(n)
        out.append(_BUF[0].raw[:n].decode())
        tv.append(_BUF[1].raw[:tl.value].decode() if tsv else None)
    return out, (tv if tsv else None), n_over


def _compare(index, labels, bases, base_off, ids, off, flags, tsv, got_out, got_tsv):
    want_out, want_tsv, n_over = _host_texts(index, labels, bases, base_off, ids, off, flags, tsv)
    bad = [q for q in range(len(want_out)) if got_out[q] != want_out[q]]
    assert not bad, (len(bad), bad[:5], got_out[bad[0]][:300], want_out[bad[0]][:300])
    if tsv:
        bad = [q for q in range(len(want_tsv)) if got_tsv[q] != want_tsv[q]]
        assert not bad, (len(bad), bad[:5])
    else:
        assert got_tsv is None
    return n_over


@pytest.fixture(scope="module")
def diptera():
    text = FASTA.read_text()
    tree = rx.parse_reference_fasta_str(text)
    queries = rx.parse_query_fasta_str(text)
    labels = [l for l, _ in queries]
    bases, off = _flat([s for _, s in queries])
    return tree, rx.Index(tree), labels, bases, off


@pytest.mark.parametrize("skip,raw", [(False, False), (True, False), (False, True)])
def test_diptera_self_classification_text(diptera, skip, raw):
    """All 7 868 records against themselves, exact matches looked up on the device; `.out` and `.tsv`."""
    tree, ix, labels, bases, off = diptera
    assert len(labels) == 7868 and ix.has_exact_lookup
    got_out, got_tsv = ix.classify_text(bases, off, labels, skip_exact_matches=skip, raw_confidence=raw, tsv=True)
    ids, eoff = ix.device_exact_matches()
    flags = (_lib.RTX_SKIP_EXACT_MATCHES if skip else 0) | (_lib.RTX_RAW_CONFIDENCE if raw else 0)
    n_over = _compare(ix, labels, bases, off, ids, eoff, flags, True, got_out, got_tsv)
    assert n_over > 5
    if not (skip or raw):
        assert sum(o.count("\n") + 1 for o in got_out if o) > len(labels)  # rows beyond the first of a query


def test_diptera_exact_ids_from_the_caller_and_out_only(diptera):
    tree, ix, labels, bases, off = diptera
    ids, eoff = ix.exact_matches(bases, off)
    got_out, got_tsv = ix.classify_text(bases, off, labels, ids, eoff)
    assert got_tsv is None
    assert _compare(ix, labels, bases, off, ids, eoff, 0, False, got_out, None) > 5


def test_pruned_path_over_many_tiles():
    db = synth.make_db(80_000)                      # 10 tiles of 8 192 references
    qs = synth.make_queries(db, 6000, seed=21, exact_frac=0.2)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    labels = [f"q{i}" for i in range(qs.n)]
    for records in (None, 0):         # the records path (default), then the dense epilogues alone (RTX_OPT_RECORDS = 0)
        ix = rx.Index(tree, prune_self_sample=False, debug_taps=True, records=records)
        ids, eoff = ix.exact_matches(qs.bases, qs.base_off)
        got_out, got_tsv = ix.classify_text(qs.bases, qs.base_off, labels, ids, eoff, tsv=True)
        assert ix.prune_verdict[0]
        st = ix.debug_prune_stats()   # (of the last sub-batch)
        assert (st["record_queries"] > 0) == (records is None), st
        assert _compare(ix, labels, qs.bases, qs.base_off, ids, eoff, 0, True, got_out, got_tsv) > 5
        del ix


def test_long_reads_failed_queries_deep_lineages_and_long_labels():
    rng = np.random.default_rng(3)
    deep = [",".join(f"lvl{d}_{i % 3}_{d}" for d in range(32)) for i in range(40)]
    shallow = [f"k_{i % 2},p_{i % 5}" for i in range(40)]
    lineages = deep + shallow
    refs = [rng.choice(np.array([1, 2, 4, 8], np.uint8), int(rng.integers(1500, 2100))) for _ in lineages]
    tree = rx.Tree.new(lineages, refs)
    ix = rx.Index(tree)
    qseqs, labels = [], []
    for i in range(300):
        r = refs[i % len(refs)]
        k = i % 6
        if k == 0:
            s = r[:5].copy()                               # no 8-mer: status != 0
        elif k == 1:
            s = r[: int(rng.integers(1031, 2055))].copy()  # the 11-plane class
        else:
            a = int(rng.integers(0, 400))
            s = r[a:a + int(rng.integers(300, 700))].copy()
        if k >= 3:
            hit = rng.random(len(s)) < 0.03
            s[hit] = rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), int(hit.sum()))
        qseqs.append(s)
        labels.append(("ß€中-" * 3 if i % 4 == 0 else "") + f"read{i}" + ("L" * 5000 if i % 25 == 0 else ""))
    bases, off = _flat(qseqs)
    got_out, got_tsv = ix.classify_text(bases, off, labels, tsv=True)
    st = np.ctypeslib.as_array(ix._view.status, shape=(len(labels),))
    assert (st != 0).sum() >= 40 and all(got_out[q] == "" for q in np.nonzero(st)[0])
    ids, eoff = ix.device_exact_matches()
    _compare(ix, labels, bases, off, ids, eoff, 0, True, got_out, got_tsv)
    assert any(o.count(",") >= 31 for o in got_out)
    assert any(len(o.encode()) > 5000 for o in got_tsv)


def test_batches_enqueued_ahead_keep_their_own_text():
    """The staged interface with RTX_OPT_RUN_AHEAD: chunk c + 1 runs while chunk c is downloaded; the text of every chunk comes from its
    own labels, bases and rows."""
    db = synth.make_db(40_000)
    qs = synth.make_queries(db, 12_000, seed=5, exact_frac=0.2)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    ix = rx.Index(tree, sub_batch=1024)
    _lib.check(ix._lib.rtx_index_set_option(ix._h, 23, 2))   # every second run-ahead is abandoned (RTX_RETRY_CHUNK): the retry path as well
    _lib.check(ix._lib.rtx_index_text_setup(ix._h, tree._h, _lib.RTX_TEXT_TSV))
    chunk = 3000
    cuts = list(range(0, qs.n, chunk)) + [qs.n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = qs.base_off[a:b + 1]
        parts.append((qs.bases[int(o[0]):int(o[-1])].copy(), (o - o[0]).astype(np.uint64), [f"c{a}_{q}" for q in range(b - a)]))

    def stage(c):
        bases, off, labels = parts[c]
        labs = (C.c_char_p * len(labels))(*[l.encode() for l in labels])
        _lib.check(ix._lib.rtx_batch_prefetch_labels(ix._h, len(labels), labs))
        ix.prefetch(bases, off)

    stage(0)
    ix.activate()
    ix.run(0)
    c = 0
    while c < len(parts):
        if c + 1 < len(parts):
            stage(c + 1)
        rc = _lib.check(ix._lib.rtx_batch_download_then_run(ix._h, C.byref(ix._view), 0))
        if rc == 1:  # RTX_RETRY_CHUNK: this chunk again, the next one staged anew
            stage(c)
            ix.activate()
            ix.run(0)
            continue
        got_out, got_tsv = ix.last_text()
        bases, off, labels = parts[c]
        ids, eoff = ix.device_exact_matches()
        _compare(ix, labels, bases, off, ids, eoff, 0, True, got_out, got_tsv)
        c += 1
    enq, abandoned = ix.run_ahead_stats
    assert enq >= 1 and abandoned >= 1, (enq, abandoned)


def test_text_needs_setup_and_labels():
    db = synth.make_db(1500, fanouts=(2, 2, 3, 3, 3, 2))
    qs = synth.make_queries(db, 50)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    ix = rx.Index(tree)
    ix.classify(qs.bases, qs.base_off)
    with pytest.raises(rx.RtxError) as e:
        ix.last_text()
    assert e.value.code == _lib.RTX_ERR_STATE
    _lib.check(ix._lib.rtx_index_text_setup(ix._h, tree._h, 0))
    ix.classify(qs.bases, qs.base_off)                       # no labels staged with the batch
    with pytest.raises(rx.RtxError):
        ix.last_text()
    other = rx.Tree.new_flat(db.lineages[:100], db.seq_bytes, db.seq_off[:101])
    with pytest.raises(rx.RtxError):
        _lib.check(ix._lib.rtx_index_text_setup(ix._h, other._h, 0))


def test_labels_of_a_refused_batch_do_not_pass_to_the_next():
    db = synth.make_db(1500, fanouts=(2, 2, 3, 3, 3, 2))
    qs = synth.make_queries(db, 50)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    ix = rx.Index(tree)
    _lib.check(ix._lib.rtx_index_text_setup(ix._h, tree._h, 0))
    labs = (C.c_char_p * qs.n)(*[f"stale{q}".encode() for q in range(qs.n)])
    _lib.check(ix._lib.rtx_batch_prefetch_labels(ix._h, qs.n, labs))
    bad = qs.base_off.copy()
    bad[3], bad[4] = bad[4], bad[3]                              # not monotone: the prefetch is refused
    with pytest.raises(rx.RtxError):
        ix.prefetch(qs.bases, bad)
    ix.classify(qs.bases, qs.base_off)                           # a batch of as many queries, without labels of its own
    with pytest.raises(rx.RtxError) as e:
        ix.last_text()
    assert e.value.code == _lib.RTX_ERR_STATE

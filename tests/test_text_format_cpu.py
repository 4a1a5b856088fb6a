"""The number formatting and the line layout of the device text (rtx_text.hip), on x86 through the emulator (rtx_emul.cpp over
rtx_math.hpp: the code the kernels run).  Signals are "{:.5}" and confidences "{:.2}" as printf / Rust print them -- the exact binary
value rounded half to even -- and a whole batch's text equals rtx_format_query's, line for line."""
import ctypes as C
import struct

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib


def _numbers(emul, vals, n_hund=0):
    v = np.ascontiguousarray(vals, dtype=np.float64)
    cap = 40 * len(v) + 8 * n_hund + 4096 + 400 * int(np.sum(~np.isfinite(v) | (np.abs(np.nan_to_num(v)) > 1e18)))
    buf = C.create_string_buffer(cap)
    emul.emul_text_numbers.restype = C.c_int64
    n = emul.emul_text_numbers(v.ctypes.data_as(C.c_void_p), C.c_uint64(len(v)), C.c_uint32(n_hund), buf, C.c_uint64(cap))
    assert n >= 0
    return buf.raw[:n].decode().split("\n")[:-1]


def _check(emul, vals):
    got = _numbers(emul, vals)
    want = ["%.5f" % x for x in vals]
    bad = [(x, g, w) for x, g, w in zip(vals, got, want) if g != w]
    assert not bad, bad[:10]


def test_signals_random_doubles(emul):
    rng = np.random.default_rng(5)
    vals = rng.random(1_000_000) * 10.0
    got = _numbers(emul, vals)
    want = [f"{x:.5f}" for x in vals.tolist()]
    assert got == want


def test_signals_on_and_beside_rounding_boundaries(emul):
    vals = [k / 64 for k in range(128)]
    for n in range(0, 200_000, 1):
        for x in (n * 1e-5 + 0.5e-5, n * 1e-5 - 0.5e-5):
            if x >= 0:
                vals += [x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, 1e9))]
    vals += [9.999995, float(np.nextafter(9.999995, 0)), float(np.nextafter(9.999995, 20)), 0.999995, 0.0, -0.0, 5e-324, 2.2250738585072014e-308 / 3,
             2.2250738585072014e-308, 1e-300, 1.0, 0.5, 123456.7890149, 999999.999995, 1e6, 3e7, 2.0 ** 53 - 0.5, 2.0 ** 53, 2.0 ** 63 + 2048,
             1.8446744073709552e19, 1e22, 1.7976931348623157e308, -0.125, -1e-5, -2.5e-6, -7.5e-6, -123.456785, -1e300]
    _check(emul, vals)


def test_non_finite_signals_print_what_the_host_path_prints(emul):
    """inf / nan: the expected text is rtx_format_query's on a hand-made view (its fallback is snprintf)."""
    lib = _lib.load()
    tree = rx.Tree.new(["a,b"], [np.array([1, 2, 4, 8, 1, 2, 4, 8, 1, 2], np.uint8)])
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    vals = [float("inf"), float("-inf"), float("nan"), neg_nan]
    nq = len(vals)
    local = np.array(vals, np.float64)
    gs = np.array(vals[::-1], np.float64)
    depth = np.full(nq, 2, np.uint32)
    conf = np.zeros((nq, 32))
    conf[:, :2] = 0.5
    begin = np.arange(nq, dtype=np.uint64)
    count = np.ones(nq, np.uint32)
    lin = np.zeros(nq, np.uint32)
    t = np.full(nq, 3, np.uint32)
    status = np.zeros(nq, np.uint8)
    v = _lib.ResultView()
    v.n_queries, v.n_rows = nq, nq
    P = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    v.t, v.status, v.global_signal = P(t, C.c_uint32), P(status, C.c_uint8), P(gs, C.c_double)
    v.row_begin, v.row_count = P(begin, C.c_uint64), P(count, C.c_uint32)
    v.row_lineage, v.row_node, v.row_depth = P(lin, C.c_uint32), P(lin, C.c_uint32), P(depth, C.c_uint32)
    v.row_conf, v.row_local_signal = P(conf, C.c_double), P(local, C.c_double)
    buf = C.create_string_buffer(4096)
    seq = np.array([1, 2, 4, 8], np.uint8)
    got = _numbers(emul, vals)
    for q in range(nq):
        n = lib.rtx_format_query(tree._h, C.byref(v), q, b"q", P(seq, C.c_uint8), 4, None, 0, 0, buf, 4096, None, 0, None)
        assert n > 0
        host = buf.raw[:n].decode().split("\t")
        assert host[3] == got[q] and host[4] == got[nq - 1 - q], (vals[q], host, got)


def test_confidences_are_a_table_of_hundredths(emul):
    got = _numbers(emul, [], n_hund=256)
    assert got == ["%.2f" % (k / 100.0) for k in range(256)]


def _rows_view(rng, lineages, nq, deep):
    """A hand-made batch: per query 0 .. 12 rows (status != 0 without rows), confidences as hundredths."""
    n_lin = len(lineages)
    counts = rng.integers(1, 13, nq).astype(np.uint32)
    status = np.zeros(nq, np.uint8)
    status[rng.random(nq) < 0.1] = 1
    counts[status != 0] = 0
    begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    nr = int(counts.sum())
    lin = rng.integers(0, n_lin, nr).astype(np.uint32)
    levels = np.array([l.count(",") + 1 for l in lineages], np.uint32)
    depth = levels[lin].copy()
    hund = np.zeros((nr, deep), np.uint8)
    for r in range(nr):
        hund[r, :depth[r]] = np.sort(rng.integers(0, 101, depth[r]))[::-1]
    local = rng.random(nr)
    gs = rng.random(nq)
    return dict(counts=counts, status=status, begin=begin, lin=lin, depth=depth, hund=hund, local=local, gs=gs, levels=levels)


@pytest.mark.parametrize("tsv", [False, True])
def test_batch_text_equals_rtx_format_query(emul, tsv):
    lib = _lib.load()
    rng = np.random.default_rng(11)
    lineages = sorted({",".join(f"L{d}_{rng.integers(0, 3)}" for d in range(rng.integers(1, 33))) for _ in range(60)})
    seqs = [rng.choice(np.array([1, 2, 4, 8, 15], np.uint8), 30) for _ in lineages]
    tree = rx.Tree.new(lineages, seqs)
    lineages = [tree.lineage(i) for i in range(tree.num_tips)]
    deep = 32
    nq = 300
    b = _rows_view(rng, lineages, nq, deep)
    labels = [("ü-" * int(rng.integers(0, 4)) + f"q{q}" + ("x" * 5000 if q % 97 == 0 else "")).encode() for q in range(nq)]
    qseqs = [rng.choice(np.array([1, 2, 4, 8, 3], np.uint8), int(rng.integers(0, 90))) for _ in range(nq)]
    exact = [[] if q % 5 else ([int(rng.integers(0, len(lineages)))] if q % 10 else [1, 2]) for q in range(nq)]
    one = np.array([e[0] if len(e) == 1 else 0xFFFFFFFF for e in exact], np.uint32)

    lin_b = b"".join(l.encode() for l in lineages)
    lin_off = np.concatenate([[0], np.cumsum([len(l.encode()) for l in lineages])]).astype(np.uint64)
    lab_b = b"".join(labels)
    lab_off = np.concatenate([[0], np.cumsum([len(l) for l in labels])]).astype(np.uint64)
    seq_b = np.concatenate(qseqs + [np.zeros(1, np.uint8)])
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in qseqs])]).astype(np.uint64)
    depth8 = b["depth"].astype(np.uint8)
    cap = 1 << 24
    out = C.create_string_buffer(cap)
    off = np.zeros(nq + 1, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    emul.emul_text_batch.restype = C.c_int64
    n = emul.emul_text_batch(C.c_char_p(lin_b), vp(lin_off), vp(b["levels"].astype(np.uint8)), vp(b["lin"]), vp(depth8), vp(b["hund"]),
                             vp(b["local"]), C.c_uint32(deep), C.c_uint64(nq), C.c_char_p(lab_b), vp(lab_off), vp(b["status"]), vp(b["begin"]),
                             vp(b["counts"]), vp(b["gs"]), vp(one), vp(seq_b), vp(seq_off), C.c_int(int(tsv)), out, C.c_uint64(cap), vp(off))
    assert n == off[-1] > 0
    raw = out.raw[:n]

    conf = np.zeros((len(b["lin"]), 32))
    conf[:, :deep] = b["hund"] / 100.0
    v = _lib.ResultView()
    v.n_queries, v.n_rows = nq, len(b["lin"])
    P = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))
    t = np.full(nq, 3, np.uint32)
    depth32 = b["depth"].astype(np.uint32)
    v.t, v.status, v.global_signal = P(t, C.c_uint32), P(b["status"], C.c_uint8), P(b["gs"], C.c_double)
    v.row_begin, v.row_count = P(b["begin"], C.c_uint64), P(b["counts"], C.c_uint32)
    v.row_lineage, v.row_node, v.row_depth = P(b["lin"], C.c_uint32), P(b["lin"], C.c_uint32), P(depth32, C.c_uint32)
    v.row_conf, v.row_local_signal = P(conf, C.c_double), P(b["local"], C.c_double)
    hcap = 1 << 20
    hb, tb, tl = C.create_string_buffer(hcap), C.create_string_buffer(hcap), C.c_int64()
    n_over = 0
    for q in range(nq):
        got = raw[int(off[q]):int(off[q + 1])]
        assert got.endswith(b"\0")
        if b["status"][q] != 0:
            assert got == b"\0"
            continue
        ex = np.array(exact[q] or [0], np.uint32)
        n_over += one[q] != 0xFFFFFFFF
        k = lib.rtx_format_query(tree._h, C.byref(v), q, labels[q], P(qseqs[q], C.c_uint8) if len(qseqs[q]) else P(seq_b, C.c_uint8),
                                 len(qseqs[q]), P(ex, C.c_uint32), len(exact[q]), 0, hb, hcap, tb if tsv else None, hcap if tsv else 0, C.byref(tl))
        assert k > 0
        want = (tb.raw[:tl.value] if tsv else hb.raw[:k]) + b"\0"
        assert got == want, q
    assert n_over > 5

"""bench.py --dump-outputs without a GPU: dump_outputs on a result view made by hand (rows stored out of query order, as the library
leaves them) -- float32 / float64 files, at most 64 MB, seeded samples beyond their sizes, rows in query order, confidences beyond a
row's depth zeroed, the same files from the same view."""
import ctypes as C
import os

import numpy as np
import pytest

import bench
import raxtax_amd as rx
from raxtax_amd import _lib


def _view(nq, seed, stride=7):
    rng = np.random.default_rng(seed)
    count = rng.integers(1, 4, nq).astype(np.uint32)
    nr = int(count.sum())
    begin = np.zeros(nq, np.uint64)
    acc = 0
    for q in rng.permutation(nq):          # the rows of a batch sit in processing order
        begin[q] = acc
        acc += int(count[q])
    keep = dict(t=rng.integers(100, 650, nq).astype(np.uint32), status=np.zeros(nq, np.uint8), gs=rng.random(nq), begin=begin, count=count,
                lin=rng.integers(0, 5000, nr).astype(np.uint32), node=rng.integers(0, 9000, nr).astype(np.uint32),
                depth=rng.integers(1, stride + 1, nr).astype(np.uint32), conf=rng.random((nr, stride)), ls=rng.random(nr))
    v = _lib.ResultView()
    v.n_queries, v.n_rows, v.row_conf_stride = nq, nr, stride

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))
    v.t, v.status, v.global_signal = p(keep["t"], C.c_uint32), p(keep["status"], C.c_uint8), p(keep["gs"], C.c_double)
    v.row_begin, v.row_count = p(keep["begin"], C.c_uint64), p(keep["count"], C.c_uint32)
    v.row_lineage, v.row_node, v.row_depth = p(keep["lin"], C.c_uint32), p(keep["node"], C.c_uint32), p(keep["depth"], C.c_uint32)
    v.row_conf, v.row_local_signal = p(keep["conf"], C.c_double), p(keep["ls"], C.c_double)
    return v, keep        # (keep: the arrays the view points into)


@pytest.mark.parametrize("nq", [1000, 1_200_000])
def test_dump_outputs_of_a_view(tmp_path, nq):
    v, _keep = _view(nq, 1)
    info = bench.dump_outputs(tmp_path / "a", rx, v)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == info["files"] and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert info["queries"] == min(nq, bench.DUMP_QUERIES) and info["row_queries"] == min(nq, bench.DUMP_ROW_QUERIES)
    assert (np.diff(a["query_ids"]) > 0).all() and (np.diff(a["row_query_ids"]) >= 0).all()
    res = rx.Result(v)
    qi = a["query_ids"].astype(np.int64)
    assert np.array_equal(a["t"], res.t[qi]) and np.array_equal(a["global_signal"], res.global_signal[qi])
    assert np.array_equal(a["n_rows"], np.diff(res.row_off.astype(np.int64))[qi])
    for q in np.unique(a["row_query_ids"])[::97].astype(np.int64):
        sel = a["row_query_ids"] == q
        rows = res.rows(int(q))
        assert [r.lineage for r in rows] == [int(x) for x in a["row_lineage"][sel]]
        assert [r.local_signal for r in rows] == list(a["row_local_signal"][sel])
        for r, c, d in zip(rows, a["row_conf"][sel], a["row_depth"][sel]):
            assert r.confidence_values == list(c[: int(d)]) and not c[int(d):].any()
    assert bench.dump_outputs(tmp_path / "b", rx, v) == dict(info, dir=str(tmp_path / "b"))
    assert all(np.array_equal(np.load(tmp_path / "b" / f), a[f[:-4]]) for f in files)

"""Device text (rtx_text.hip) at BASELINE.json configs[2]: 1 M synthetic COI-length queries against 500 000 references.  Per mode (text
off, `.out`, `.out` + `.tsv`) the host time of rtx_batch_download -- which runs the text passes and copies the text when the text is on --
after the run has finished (rtx_batch_sync), and the bytes of text per query.  Kernel times: run it under rocprofv3 --kernel-trace --stats
(text_measure_kernel, text_write_kernel, rocprim's scan).

    python tools/device_text_probe.py [--refs 500000] [--queries 1000000] [--reps 3]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

import raxtax_amd as rx  # noqa: E402
from raxtax_amd import _lib, synth  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=500_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    db = synth.make_db(a.refs)
    qs = synth.make_queries(db, a.queries, seed=3)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
    ix = rx.Index(tree)
    lib = ix._lib
    labs = (C.c_char_p * qs.n)(*[l.encode() for l in qs.labels])
    out = {"refs": a.refs, "queries": qs.n}
    for name, flags in (("off", None), ("out", 0), ("out+tsv", _lib.RTX_TEXT_TSV), ("off_again", None)):
        _lib.check(lib.rtx_index_text_setup(ix._h, tree._h if flags is not None else None, flags or 0))
        ms = []
        for _ in range(a.reps + 1):  # the first one sizes the buffers
            if flags is not None:
                _lib.check(lib.rtx_batch_prefetch_labels(ix._h, qs.n, labs))
            ix.prefetch(qs.bases, qs.base_off)
            ix.activate()
            ix.run(0)
            ix.sync()
            t0 = time.perf_counter()
            ix.download(copy=False)
            ms.append((time.perf_counter() - t0) * 1e3)
        rec = {"download_ms": [round(x, 3) for x in ms[1:]], "download_ms_median": round(float(np.median(ms[1:])), 3)}
        if flags is not None:
            tv = _lib.TextView()
            _lib.check(lib.rtx_batch_text(ix._h, C.byref(tv)))
            rec["out_bytes_per_query"] = round(tv.out_off[qs.n] / qs.n, 1)
            if tv.tsv:
                rec["tsv_bytes_per_query"] = round(tv.tsv_off[qs.n] / qs.n, 1)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    base = (out["off"]["download_ms_median"] + out["off_again"]["download_ms_median"]) / 2
    scale = 1e6 / qs.n
    out["text_ms_per_1M_queries"] = {"out": round((out["out"]["download_ms_median"] - base) * scale, 2),
                                     "out+tsv": round((out["out+tsv"]["download_ms_median"] - base) * scale, 2)}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

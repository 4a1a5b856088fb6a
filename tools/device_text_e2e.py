"""rtx_raxtax end to end with RTX_OPT_DEVICE_TEXT off and on (the messages formatted by the host or by rtx_text.hip), into a sender that keeps
nothing (rtx_sender_discard, as bench.py's value_end_to_end), at host shares 1 and 8 (rtx_set_host_share), `.out` and `.out` + `.tsv`:
  synthetic  BASELINE.json configs[2]: 1 M COI-length queries against 500 000 references
  diptera16  the 600 Diptera records x 16 (tests/test_gpu_pruned_path.py: _diptera_expanded) as database, its 9 600 sequences x 11 as queries
Per leg: the median of three calls in ms, queries/s, and rtx_raxtax_last_timing's busy ms (host lookup, device stage, format, sender).

    python tools/device_text_e2e.py [--chunk 131072] [--legs synthetic,diptera16]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

import raxtax_amd as rx  # noqa: E402
from raxtax_amd import synth  # noqa: E402

lib = rx._lib.load()
SENDER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p)
lib.rtx_raxtax.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p), rx._lib.u8p, rx._lib.u64p,
                           ctypes.c_int, ctypes.c_int, ctypes.c_uint64, SENDER, ctypes.c_void_p, ctypes.c_int]
DISCARD = ctypes.cast(lib.rtx_sender_discard, SENDER)


def leg(name, tree, index, labels_py, bases, off, chunk):
    n = len(off) - 1
    labels = (ctypes.c_char_p * n)(*[l.encode() for l in labels_py])
    bases = np.ascontiguousarray(bases)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    res = []
    for share in (1, 8):
        rx._lib.check(lib.rtx_set_host_share(share))
        for tsv in (0, 1):
            for text in (0, 1):
                rx._lib.check(lib.rtx_index_set_option(index._h, 24, text))
                counted = (ctypes.c_uint64 * 2)()

                def call():
                    rx._lib.check(lib.rtx_raxtax(index._h, tree._h, n, labels, rx._lib.ptr(bases, rx._lib.u8p), rx._lib.ptr(off, rx._lib.u64p),
                                                 0, 0, chunk, DISCARD, ctypes.cast(counted, ctypes.c_void_p), tsv))
                call()
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    call()
                    ms.append((time.perf_counter() - t0) * 1e3)
                busy = (ctypes.c_double * 4)()
                nc = ctypes.c_uint64()
                rx._lib.check(lib.rtx_raxtax_last_timing(busy, ctypes.byref(nc)))
                med = float(np.median(ms))
                rec = {"leg": name, "host_share": share, "tsv": tsv, "device_text": text, "queries": n, "chunks": int(nc.value),
                       "ms_median": round(med, 1), "ms": [round(x, 1) for x in ms], "queries_per_s": round(n / med * 1e3),
                       "busy_ms": {"lookup": round(busy[0] * 1e3, 1), "device": round(busy[1] * 1e3, 1), "format": round(busy[2] * 1e3, 1),
                                   "sender": round(busy[3] * 1e3, 1)}}
                print(json.dumps(rec), flush=True)
                res.append(rec)
    rx._lib.check(lib.rtx_set_host_share(1))
    rx._lib.check(lib.rtx_index_set_option(index._h, 24, 0))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=131072)
    ap.add_argument("--legs", default="synthetic,diptera16")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if "synthetic" in legs:
        db = synth.make_db(500_000)
        qs = synth.make_queries(db, 1_000_000, seed=3)
        tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off)
        index = rx.Index(tree)
        leg("synthetic", tree, index, qs.labels, qs.bases, qs.base_off, a.chunk)
        del index, tree, db, qs
    if "diptera16" in legs:
        from test_gpu_pruned_path import _diptera_expanded
        lineages, flat, off, seqs = _diptera_expanded(16)
        tree = rx.Tree.new_flat(lineages, flat, off)
        index = rx.Index(tree, prune_self_sample=False)
        q = seqs * 11
        qoff = np.zeros(len(q) + 1, np.uint64)
        qoff[1:] = np.cumsum([len(s) for s in q])
        leg("diptera16", tree, index, [f"d{i}" for i in range(len(q))], np.concatenate(q), qoff, a.chunk)
    return 0


if __name__ == "__main__":
    sys.exit(main())

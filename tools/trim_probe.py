#!/usr/bin/env python3
"""What primer trimming (rtx_index_set_primers, rtx_trim.hip) costs: with the option off against the parent commit, and with it on.
    off  `python bench.py` (--bench-args) in a built checkout of the parent commit (--parent TREE) and in this tree, interleaved, --repeats
         runs each, every run a process of its own: the option is off when this tree's figures lie inside the parent's own spread.
    on   1 M synthetic reads of 658 + 2 x 25 bases (primer + amplicon + revcomp(primer), one read in four with a primer error, one in ten
         without primers) and four patterns (a degenerate pair registered for both strands), in a process of its own:
           rtx_trim_run alone, packing and transfer included, in reads per second; its kernel alone from HIP events (rtx_trim_kernel_time);
           rtx_raxtax into rtx_sender_discard against --refs references on those reads with the option on and off (off classifies the reads
           with their primers on: the same bytes in, another answer), with the busy seconds of the stage (rtx_raxtax_last_trim).
    python tools/trim_probe.py [--parent TREE] [--repeats 3] [--refs N --queries N] [--out profiles/trim_probe.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYC"   # 25 bases each

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it the option-off leg is left out")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--bench-args", default="--gpus 1 --steps 5 --warmup 1 --no-cpu-baseline")
ap.add_argument("--refs", type=int, default=500_000)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--chunk", type=int, default=131072, help="queries per chunk of rtx_raxtax (what raxtax-hip uses)")
ap.add_argument("--timed", type=int, default=3, help="timed calls behind one warm-up call; their median is the figure")
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()


def child():
    sys.path.insert(0, str(HERE))
    import raxtax_amd as rx
    from raxtax_amd import _lib, synth
    db = synth.make_db(args.refs)
    qs = synth.make_queries(db, args.queries)
    n, L = args.queries, db.length
    rng = np.random.default_rng(7)
    pats = rx.primer_patterns((FWD, REV), both_strands=True)
    inst = lambda t: np.array([[b for b in (1, 2, 4, 8) if c & b][0] for c in rx.encode_iupac(t)], np.uint8)
    f, r = inst(FWD), rx.api.revcomp(inst(REV))
    W = len(f) + L + len(r)
    reads = np.empty((n, W), np.uint8)
    reads[:, :len(f)] = f
    reads[:, len(f):len(f) + L] = qs.bases.reshape(n, L)
    reads[:, len(f) + L:] = r
    err = np.nonzero(rng.integers(0, 4, n) == 0)[0]                      # one read in four: a substitution in the 5' primer
    reads[err, rng.integers(0, len(f), len(err))] = 1
    bare = np.nonzero(rng.integers(0, 10, n) == 0)[0]                    # one in ten: no primers (random bases in their place)
    reads[bare, :len(f)] = 1 << rng.integers(0, 4, (len(bare), len(f)))
    reads[bare, len(f) + L:] = 1 << rng.integers(0, 4, (len(bare), len(r)))
    bases = reads.reshape(-1)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
    out = dict(reads=n, read_length=W, patterns=len(pats))
    t = rx.Trim(0, pats)
    ts, ks = [], []
    for k in range(1 + args.timed):
        t0 = time.perf_counter()
        lo, hi, hit = t.run(bases, off)
        ts.append(time.perf_counter() - t0)
        ks.append(t.kernel_ms())
    dt = float(np.median(ts[1:]))
    out["trim_run"] = dict(seconds=round(dt, 4), calls=[round(x, 4) for x in ts], reads_per_s=round(n / dt), kernel_ms=[round(x, 3) for x in ks],
                           kernel_reads_per_s=round(n / (float(np.median(ks[1:])) * 1e-3)), with5=int(((hit & 0xFF) != 0xFF).sum()),
                           with3=int((((hit >> 16) & 0xFF) != 0xFF).sum()), staged_bytes_per_read=2 * 16 * ((max(len(p.codes) + p.max_errors + 32 for p in pats) + 31) // 32) + 4)
    del t
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    index = rx.Index(tree)
    lib = _lib.load()
    sender = C.cast(lib.rtx_sender_discard, C.c_void_p)
    lib.rtx_raxtax.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), _lib.u8p, _lib.u64p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    labels = (C.c_char_p * n)(*[b"q%d" % i for i in range(n)])
    for name, on in (("raxtax_off", False), ("raxtax_on", True), ("raxtax_off_again", False)):
        index.set_primers(pats if on else [])
        ts = []
        for k in range(1 + args.timed):
            count = (C.c_uint64 * 2)(0, 0)
            t0 = time.perf_counter()
            _lib.check(lib.rtx_raxtax(index._h, tree._h, n, labels, _lib.ptr(bases, _lib.u8p), _lib.ptr(off, _lib.u64p), 0, 0, args.chunk, sender, C.cast(count, C.c_void_p), 0))
            ts.append(time.perf_counter() - t0)
        busy, n_chunks = rx.raxtax_last_timing()
        line = dict(seconds=round(float(np.median(ts[1:])), 4), calls=[round(x, 4) for x in ts], messages=int(count[0]), queries_per_s=round(n / float(np.median(ts[1:]))),
                    busy_lookup_device_format_sender=[round(b, 4) for b in busy], chunks=n_chunks)
        if on:
            q, w5, w3, e, b = rx.raxtax_last_trim()
            line.update(trim_queries=q, with5=w5, with3=w3, emptied=e, trim_busy_seconds=round(b, 4))
        out[name] = line
    print("PROBE " + json.dumps(out), flush=True)


if args.child:
    child()
    sys.exit(0)


def bench(root):
    p = subprocess.run([sys.executable, "bench.py"] + args.bench_args.split(), cwd=root, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
    if p.returncode != 0:   # (nothing more is started on the device behind a process that died)
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"bench.py in {root}: exit status {p.returncode}")
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return dict(value=line["value"], end_to_end=(line.get("value_end_to_end") or {}).get("value"))


summary = dict(bench_args=args.bench_args, repeats=args.repeats)
if args.parent:
    legs = [("parent", str(Path(args.parent).resolve())), ("this", str(HERE))]
    runs = {name: [] for name, _ in legs}
    for rep in range(args.repeats):
        for name, root in legs:
            runs[name].append(bench(root))
            print(name, rep, json.dumps(runs[name][-1]), flush=True)
    off = {}
    for key in ("value", "end_to_end"):
        a, b = ([r[key] for r in runs[name] if r[key] is not None] for name in ("parent", "this"))
        if a and b:
            off[key] = dict(parent=a, this=b, parent_min=min(a), parent_max=max(a), this_median=float(np.median(b)), this_inside_spread_of_parent=bool(min(a) <= float(np.median(b)) <= max(a)),
                            this_over_parent_median=round(float(np.median(b)) / float(np.median(a)), 4))
    summary["option_off"] = off
cmd = [sys.executable, __file__, "--child", "--refs", str(args.refs), "--queries", str(args.queries), "--chunk", str(args.chunk), "--timed", str(args.timed)]
p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
if p.returncode != 0:
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    sys.exit(f"option-on leg: exit status {p.returncode}")
summary["option_on"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

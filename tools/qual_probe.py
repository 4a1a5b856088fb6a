#!/usr/bin/env python3
"""What the quality filter (rtx_index_set_quality, rtx_qual.hip) costs: with the option off against the parent commit, and with it on.
    off  `python bench.py` (--bench-args) in a built checkout of the parent commit (--parent TREE) and in this tree, interleaved, --repeats
         runs each, every run a process of its own: the option is off when this tree's median lies inside the parent's own spread.
    on   --queries synthetic reads of 250 and of 658 bases with realistic quality strings (Q falls along the read from about 38 to about 12
         with noise, one base in a few hundred drops to Q 2) under --maxee 2 --truncq 2, in a process of its own:
           rtx_qual_run alone: the kernel from HIP events (rtx_qual_kernel_time) and the call split into the host's staging pass, the copies
           with the wait around the kernel, and the kernel (rtx_qual_stage_times);
           rx.qual_read, the same computation on ONE host thread, over a sample of the same reads, in reads per second;
           rtx_raxtax into rtx_sender_discard against --refs references on the 658-base reads with the option on and off: the busy seconds of
           the stage (rtx_raxtax_last_qual) beside the device busy seconds of the handle (rtx_raxtax_last_timing, busy[1]); and with the
           option off on the reads as the filter leaves them (cut and emptied beforehand): what the handle alone needs for those reads.
    python tools/qual_probe.py [--parent TREE] [--repeats 3] [--refs N --queries N] [--out profiles/qual_probe.json]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it the option-off leg is left out")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--bench-args", default="--gpus 1 --steps 5 --warmup 1 --no-cpu-baseline")
ap.add_argument("--refs", type=int, default=500_000)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--chunk", type=int, default=131072, help="queries per chunk of rtx_raxtax (what raxtax-hip uses)")
ap.add_argument("--timed", type=int, default=3, help="timed calls behind one warm-up call; their median is the figure")
ap.add_argument("--host-sample", type=int, default=20000, help="reads the one-thread host function is timed on")
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()


def qualities(rng, n, L):
    """[n, L] quality bytes (base 33): Q falls from about 38 to about 12 along the read, with noise; one base in 400 drops to Q 2."""
    slope = (38 - (np.arange(L) * 26) // L).astype(np.int16)
    q = np.clip(slope[None, :] + rng.integers(-3, 4, (n, L), dtype=np.int16), 3, 41)
    q[rng.random((n, L)) < 1 / 400] = 2
    return (33 + q).astype(np.uint8)


def child():
    sys.path.insert(0, str(HERE))
    import raxtax_amd as rx
    from raxtax_amd import _lib, synth
    params = rx.QualParams(max_ee=2.0, trunc_qual=2)
    n = args.queries
    rng = np.random.default_rng(7)
    db = synth.make_db(args.refs)
    qs = synth.make_queries(db, n)
    L = db.length
    full = qs.bases.reshape(n, L)
    out = dict(reads=n, params="--maxee 2 --truncq 2")
    stage = rx.Qual(0, params)
    kept = {}
    for W in (250, L):
        bases = np.ascontiguousarray(full[:, :W]).reshape(-1)
        quals = qualities(rng, n, W).reshape(-1)
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        ts, ks, parts = [], [], []
        for k in range(1 + args.timed):
            t0 = time.perf_counter()
            hi, ee, verdict = stage.run(bases, quals, off)
            ts.append(time.perf_counter() - t0)
            ks.append(stage.kernel_ms())
            parts.append(stage.stage_seconds())
        dt = float(np.median(ts[1:]))
        mid = lambda xs: float(np.median(xs[1:]))
        t0 = time.perf_counter()
        m = min(args.host_sample, n)
        for i in range(m):
            rx.qual_read(params, bases[i * W:(i + 1) * W], quals[i * W:(i + 1) * W])
        host_python = time.perf_counter() - t0
        out[f"reads_of_{W}"] = dict(
            seconds=round(dt, 4), calls=[round(x, 4) for x in ts], reads_per_s=round(n / dt), kernel_ms=[round(x, 3) for x in ks],
            kernel_reads_per_s=round(n / (mid(ks) * 1e-3)), kernel_bytes_per_s=round(n * W / (mid(ks) * 1e-3)),
            staging_seconds=round(mid([p[0] for p in parts]), 4), copies_and_wait_seconds=round(mid([p[1] for p in parts]), 4),
            kernel_seconds=round(mid(ks) * 1e-3, 5), passed=int((verdict == 0).sum()), cut_short=int(((verdict == 0) & (hi < W)).sum()),
            host_one_thread=dict(reads=m, seconds_through_python=round(host_python, 3), reads_per_s_through_python=round(m / host_python)))
        kept[W] = (bases, quals, off, np.where(verdict == 0, hi, 0).astype(np.uint32))
    # (the host figure is rx.qual_read called read by read: it includes the ctypes call around every read)
    del stage
    bases, quals, off, keep_hi = kept[L]
    cut_bases, cut_off = rx.trim_apply(bases, off, np.zeros(n, np.uint32), keep_hi)   # what the handle receives with the option on
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    index = rx.Index(tree)
    lib = _lib.load()
    sender = C.cast(lib.rtx_sender_discard, C.c_void_p)
    lib.rtx_raxtax_multi_ex5.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), _lib.u8p, _lib.u64p, C.c_int, C.c_int,
                                         C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _lib.u8p, C.c_void_p, C.c_void_p]
    labels = (C.c_char_p * n)(*[b"q%d" % i for i in range(n)])
    handles = (C.c_void_p * 1)(index._h.value)
    for name, on in (("raxtax_off", False), ("raxtax_on", True), ("raxtax_off_on_the_filtered_reads", False), ("raxtax_off_again", False)):
        index.set_quality(params if on else None)
        b_now, o_now = (cut_bases, cut_off) if name == "raxtax_off_on_the_filtered_reads" else (bases, off)
        ts = []
        for k in range(1 + args.timed):
            count = (C.c_uint64 * 2)(0, 0)
            t0 = time.perf_counter()
            _lib.check(lib.rtx_raxtax_multi_ex5(handles, 1, tree._h, n, labels, _lib.ptr(b_now, _lib.u8p), _lib.ptr(o_now, _lib.u64p), 0, 0, args.chunk, sender,
                                                C.cast(count, C.c_void_p), 0, None, None, None, None, _lib.ptr(quals, _lib.u8p) if on else None, None, None))
            ts.append(time.perf_counter() - t0)
        busy, n_chunks = rx.raxtax_last_timing()
        line = dict(seconds=round(float(np.median(ts[1:])), 4), calls=[round(x, 4) for x in ts], messages=int(count[0]), queries_per_s=round(n / float(np.median(ts[1:]))),
                    busy_lookup_device_format_sender=[round(b, 4) for b in busy], chunks=n_chunks)
        if on:
            q, passed, cut, why, b = rx.raxtax_last_qual()
            line.update(qual_queries=q, passed=passed, cut_short=cut, reasons=why, qual_busy_seconds=round(b, 4), device_busy_seconds=round(busy[1], 4),
                        stage_hides_behind_the_device=bool(b < busy[1]))
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
cmd = [sys.executable, __file__, "--child", "--refs", str(args.refs), "--queries", str(args.queries), "--chunk", str(args.chunk), "--timed", str(args.timed),
       "--host-sample", str(args.host_sample)]
p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
if p.returncode != 0:
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    sys.exit(f"option-on leg: exit status {p.returncode}")
summary["option_on"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

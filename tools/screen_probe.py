#!/usr/bin/env python3
"""What the contaminant screen (rtx_index_set_screen, rtx_screen.hip) costs: with the option off against the parent commit, and with it on.
    off  `python bench.py` (--bench-args) in a built checkout of the parent commit (--parent TREE) and in this tree, interleaved, --repeats
         runs each, every run a process of its own: the option is off when this tree's median lies inside the parent's own spread.
    on   --queries synthetic reads of 250 and of 658 bases, one in ten cut from a seeded random 5 386-base genome, in a process of its own:
           rtx_screen_run alone against the 5 386-base set and against a set of --big-set random bases: the kernel from HIP events
           (rtx_screen_kernel_time) and the call split into the host's staging pass, the copies with the wait around the kernel, and the
           kernel (rtx_screen_stage_times); beside it rtx_qual's kernel on the same reads in the same run -- it streams the same bytes and
           probes nothing -- and the ratio of the two;
           rtx_raxtax into rtx_sender_discard against --refs references on the 658-base reads with the option on and off: the busy seconds
           of the stage (rtx_raxtax_last_screen) beside the device busy seconds of the handle (rtx_raxtax_last_timing, busy[1]); and with
           thresholds that no read meets: the stage without the cut of the chunks behind it.
    python tools/screen_probe.py [--parent TREE] [--repeats 3] [--legs off,on] [--refs N --queries N] [--out profiles/screen_probe.json]"""
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
ap.add_argument("--big-set", type=int, default=4_000_000, help="bases of the large contaminant set")
ap.add_argument("--chunk", type=int, default=131072, help="queries per chunk of rtx_raxtax (what raxtax-hip uses)")
ap.add_argument("--timed", type=int, default=3, help="timed calls behind one warm-up call; their median is the figure")
ap.add_argument("--legs", default="off,on", help="which legs to run; with --out an existing file keeps the leg that is not run")
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()


def child():
    sys.path.insert(0, str(HERE))
    import raxtax_amd as rx
    from raxtax_amd import _lib, synth
    n = args.queries
    rng = np.random.default_rng(7)
    codes = lambda k: (np.uint8(1) << rng.integers(0, 4, k).astype(np.uint8)).astype(np.uint8)
    genome = codes(5386)
    sets = {"set_of_5386_bases": rx.ScreenSet([genome]), f"set_of_{args.big_set}_bases": rx.ScreenSet([genome, codes(args.big_set)])}
    db = synth.make_db(args.refs)
    qs = synth.make_queries(db, n)
    L = db.length
    full = qs.bases.reshape(n, L).copy()
    doubled = np.concatenate([genome, genome])
    for i in range(0, n, 10):                                        # 10 % contaminant reads
        at = int(rng.integers(0, 5386))
        full[i] = doubled[at:at + L] if at + L <= len(doubled) else doubled[:L]
    out = dict(reads=n, contaminant_share=0.1, params="defaults (min_hits 2, min_pct 50)")
    for name, sset in sets.items():
        out[name] = dict(info=sset.info())
    qual = rx.Qual(0, rx.QualParams(max_ee=2.0, trunc_qual=2))
    mid = lambda xs: float(np.median(xs[1:]))
    for W in (250, L):
        bases = np.ascontiguousarray(full[:, :W]).reshape(-1)
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        quals = np.full(n * W, 33 + 30, np.uint8)
        qk = []
        for k in range(1 + args.timed):
            qual.run(bases, quals, off)
            qk.append(qual.kernel_ms())
        for name, sset in sets.items():
            stage = rx.Screen(0, sset, rx.ScreenParams())
            ts, ks, parts = [], [], []
            for k in range(1 + args.timed):
                t0 = time.perf_counter()
                windows, hits, first, source, verdict = stage.run(bases, off)
                ts.append(time.perf_counter() - t0)
                ks.append(stage.kernel_ms())
                parts.append(stage.stage_seconds())
            dt = mid(ts)
            out[name][f"reads_of_{W}"] = dict(
                seconds=round(dt, 4), calls=[round(x, 4) for x in ts], reads_per_s=round(n / dt), kernel_ms=[round(x, 3) for x in ks],
                kernel_bytes_per_s=round(n * W / (mid(ks) * 1e-3)), probes=int(windows.sum()), hits=int(hits.sum()), contaminants=int(verdict.sum()),
                staging_seconds=round(mid([p[0] for p in parts]), 4), copies_and_wait_seconds=round(mid([p[1] for p in parts]), 4),
                kernel_seconds=round(mid(ks) * 1e-3, 5), qual_kernel_ms=[round(x, 3) for x in qk], kernel_over_qual_kernel=round(mid(ks) / mid(qk), 2))
            del stage
    del qual
    bases = np.ascontiguousarray(full).reshape(-1)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    index = rx.Index(tree)
    lib = _lib.load()
    sender = C.cast(lib.rtx_sender_discard, C.c_void_p)
    lib.rtx_raxtax_multi.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), _lib.u8p, _lib.u64p, C.c_int, C.c_int,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    labels = (C.c_char_p * n)(*[b"q%d" % i for i in range(n)])
    handles = (C.c_void_p * 1)(index._h.value)
    small = sets["set_of_5386_bases"]
    never = rx.ScreenParams(min_hits=1 << 31, min_pct=100)         # screens every read and flags none: no chunk is cut, every read is classified
    for name, on in (("raxtax_off", False), ("raxtax_on", True), ("raxtax_on_nothing_flagged", True), ("raxtax_off_again", False)):
        index.set_screen(small if on else None, never if name == "raxtax_on_nothing_flagged" else None)
        ts = []
        for k in range(1 + args.timed):
            count = (C.c_uint64 * 2)(0, 0)
            t0 = time.perf_counter()
            _lib.check(lib.rtx_raxtax_multi(handles, 1, tree._h, n, labels, _lib.ptr(bases, _lib.u8p), _lib.ptr(off, _lib.u64p), 0, 0, args.chunk, sender,
                                            C.cast(count, C.c_void_p), 0))
            ts.append(time.perf_counter() - t0)
        busy, n_chunks = rx.raxtax_last_timing()
        line = dict(seconds=round(mid(ts), 4), calls=[round(x, 4) for x in ts], messages=int(count[0]), queries_per_s=round(n / mid(ts)),
                    busy_lookup_device_format_sender=[round(b, 4) for b in busy], chunks=n_chunks)
        if on:
            q, screened, contaminants, b = rx.raxtax_last_screen()
            line.update(screen_queries=q, screened=screened, contaminants=contaminants, screen_busy_seconds=round(b, 4), device_busy_seconds=round(busy[1], 4),
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
if args.out and Path(args.out).exists():
    summary.update(json.loads(Path(args.out).read_text()), bench_args=args.bench_args, repeats=args.repeats)
legs_wanted = args.legs.split(",")
if args.parent and "off" in legs_wanted:
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
if "on" not in legs_wanted:
    print(json.dumps(summary, indent=1))
    if args.out:
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    sys.exit(0)
cmd = [sys.executable, __file__, "--child", "--refs", str(args.refs), "--queries", str(args.queries), "--chunk", str(args.chunk), "--timed", str(args.timed),
       "--big-set", str(args.big_set)]
p = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
if p.returncode != 0:
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    sys.exit(f"option-on leg: exit status {p.returncode}")
summary["option_on"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

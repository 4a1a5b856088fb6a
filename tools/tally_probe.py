#!/usr/bin/env python3
"""What the table of distinct reads (rtx_index_set_tally, rtx_tally.hip) costs end to end: rtx_raxtax into rtx_sender_discard, 1 M synthetic
658-base queries against 500 000 references (the shapes of BASELINE.json configs[2]) in chunks of 131 072, with 0 %, 50 % and 90 % of the
queries copies of another one (drawn from the distinct ones with a fixed seed, the order shuffled).  Three legs, interleaved per repeat as
tools/ab_run.sh interleaves its runs, every measurement in a process of its own:
    (a) another tree of this repository, built (--parent TREE: a checkout of the parent commit), no tally
    (b) this tree, no tally              -- must lie inside the spread of (a)
    (c) this tree, a tally on the handle -- a fresh object per call (every sequence is new to it: the table, the arena and the matrix grow
        from their initial sizes), with rtx_raxtax_last_tally's busy time, and rtx_tally_add alone over the same chunks in reads/s: into a
        fresh object (first sight) and once more into the same one (every read found)
    python tools/tally_probe.py [--parent TREE] [--repeats 5] [--shares 0,50,90] [--refs N --queries N] [--out profiles/tally_probe.json]
The inputs are generated once and handed to the children through a file in --work (default: build/tally_probe)."""
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
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (leg a); without it the leg is left out")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--shares", default="0,50,90")
ap.add_argument("--refs", type=int, default=500_000)
ap.add_argument("--queries", type=int, default=1_000_000)
ap.add_argument("--chunk", type=int, default=131072, help="queries per chunk of rtx_raxtax (what raxtax-hip uses)")
ap.add_argument("--timed", type=int, default=3, help="timed calls per share and process, behind one warm-up call; their median is the figure")
ap.add_argument("--work", default=str(HERE / "build" / "tally_probe"))
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # tree:tally -- one process of one leg
args = ap.parse_args()
shares = [int(s) for s in args.shares.split(",")]
work = Path(args.work)
inputs = work / f"inputs_{args.refs}_{args.queries}.npz"


def child(tree_root: str, tally: bool):
    sys.path.insert(0, tree_root)
    import raxtax_amd as rx
    from raxtax_amd import _lib
    z = np.load(inputs, allow_pickle=False)
    lineages = bytes(z["lineages"]).decode().split("\n")
    tree = rx.Tree.new_flat(lineages, z["seq_bytes"], z["seq_off"], kmer_map=False)
    index = rx.Index(tree)
    lib = _lib.load()
    sender = C.cast(lib.rtx_sender_discard, C.c_void_p)
    lib.rtx_raxtax.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), _lib.u8p, _lib.u64p, C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    n, L = args.queries, int(z["length"])
    labels = (C.c_char_p * n)(*[b"q%d" % i for i in range(n)])
    q_all = z["q_bases"].reshape(n, L)
    out = []
    for share in shares:
        rng = np.random.default_rng(1000 + share)
        n_distinct = n - n * share // 100
        pick = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, n - n_distinct)])
        pick = pick[rng.permutation(n)]
        bases = np.ascontiguousarray(q_all[pick]).reshape(-1)
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        ts, busy, entries = [], [], 0
        for k in range(1 + args.timed):
            count = (C.c_uint64 * 2)(0, 0)
            if tally:
                index.set_tally(rx.Tally())
            t0 = time.perf_counter()
            _lib.check(lib.rtx_raxtax(index._h, tree._h, n, labels, _lib.ptr(bases, _lib.u8p), _lib.ptr(off, _lib.u64p), 0, 0, args.chunk, sender, C.cast(count, C.c_void_p), 0))
            if tally:
                entries = index.tally.info()["entries"]   # (exact on the host; the last chunk's append and count may still run: read() would wait)
            ts.append(time.perf_counter() - t0)
            assert count[0] > 0.98 * n, count[0]
            if tally:
                busy.append(rx.raxtax_last_tally()[3])
        line = dict(share=share, tally=tally, seconds=round(float(np.median(ts[1:])), 4), calls=[round(t, 4) for t in ts], messages=int(count[0]), text_bytes=int(count[1]))
        if tally:
            index.set_tally(None)
            line.update(entries=entries, tally_busy_seconds=round(float(np.median(busy[1:])), 4))
            alone = []
            for fresh in (True, False):
                if fresh:
                    t = rx.Tally()
                    t.add(bases[:L], off[:2])   # (the first launch of the kernels is not the stage's cost)
                t0 = time.perf_counter()
                for a in range(0, n, args.chunk):
                    b = min(n, a + args.chunk)
                    t.add(bases[a * L:b * L], off[a:b + 1] - off[a])
                t.add(bases[:L], off[:2])          # (an add waits for everything enqueued before its scan: the last chunk's append and count are in)
                alone.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            totals = t.read().totals               # the download of the table and its sort on the host, once per run
            t_read = time.perf_counter() - t0
            assert totals["reads"] == 2 * n + 3 and totals["entries"] == entries, (totals, entries)
            line.update(add_alone_first_sight_reads_per_s=round(n / alone[0]), add_alone_all_found_reads_per_s=round(n / alone[1]), read_seconds=round(t_read, 4))
        out.append(line)
    print("PROBE " + json.dumps(out), flush=True)


if args.child:
    root, flag = args.child.rsplit(":", 1)
    child(root, flag == "1")
    sys.exit(0)

# ---- the parent process: inputs once, then the legs in turn
sys.path.insert(0, str(HERE))
from raxtax_amd import synth  # noqa: E402

work.mkdir(parents=True, exist_ok=True)
if not inputs.exists():
    db = synth.make_db(args.refs)
    qs = synth.make_queries(db, args.queries)
    np.savez(inputs, lineages=np.frombuffer("\n".join(db.lineages).encode(), np.uint8), seq_bytes=db.seq_bytes, seq_off=db.seq_off, q_bases=qs.bases, length=db.length)
    del db, qs
legs = ([("a", str(Path(args.parent).resolve()), 0)] if args.parent else []) + [("b", str(HERE), 0), ("c", str(HERE), 1)]
results = {name: [] for name, _, _ in legs}
for rep in range(args.repeats):
    for name, root, tally in legs:
        cmd = [sys.executable, __file__, "--child", f"{root}:{tally}", "--shares", args.shares, "--refs", str(args.refs), "--queries", str(args.queries),
               "--chunk", str(args.chunk), "--timed", str(args.timed), "--work", str(work)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=""))
        if p.returncode != 0:   # (nothing more is started on the device behind a process that died)
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"leg {name}, repeat {rep}: exit status {p.returncode}")
        line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1]
        results[name].append(json.loads(line[6:]))
        print(name, rep, line[6:], flush=True)
summary = dict(workload=dict(references=args.refs, queries=args.queries, length=658, chunk=args.chunk, sender="rtx_sender_discard", repeats=args.repeats,
                             timed_calls_per_process=args.timed), shares={})
for i, share in enumerate(shares):
    s = {}
    for name in results:
        secs = [r[i]["seconds"] for r in results[name]]
        s[name] = dict(seconds=secs, median=round(float(np.median(secs)), 4), min=min(secs), max=max(secs))
    if "a" in s:
        s["b_inside_spread_of_a"] = bool(s["a"]["min"] <= s["b"]["median"] <= s["a"]["max"])
    c = [r[i] for r in results["c"]]
    s["c"].update(entries=c[0]["entries"], tally_busy_seconds=[r["tally_busy_seconds"] for r in c],
                  add_alone_first_sight_reads_per_s=[r["add_alone_first_sight_reads_per_s"] for r in c],
                  add_alone_all_found_reads_per_s=[r["add_alone_all_found_reads_per_s"] for r in c], read_seconds=[r["read_seconds"] for r in c], slowdown_over_b=round(s["c"]["median"] / s["b"]["median"], 3))
    summary["shares"][str(share)] = s
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

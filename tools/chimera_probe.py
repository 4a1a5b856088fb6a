#!/usr/bin/env python3
"""What the chimera check (rtx_index_set_chimera, rtx_chimera.hip) costs and what its definition does at scale.
    off    `python bench.py` (--bench-args) in a built checkout of the parent commit (--parent TREE) and in this tree, interleaved, --repeats
           runs each, every run a process of its own: the option is off when this tree's median lies inside the parent's own spread.
    speed  rtx_chimera_run alone, inputs resident in host memory, in a process of its own, for 50 000 references (configs[1]'s database,
           100 000 reads) and 500 000 references (65 536 reads): the median of three blocks of --timed calls with the spread over the
           blocks; reads/s of the call, the scan kernels from HIP events (rtx_chimera_kernel_time), the bytes the scan requests
           (2 x padded rows x tiles x 1 KiB per read, from the shapes) and the resulting bytes/s.
           Beside it the yardstick: the classifier with tile pruning off on the same reads (upload once, then run + download: what bench.py's
           value_unpruned leg times; the counting path is the parent commit's, this change leaves it alone) and the ratio of the two times
           per read.
    scale  the share of flagged reads among 100 000 plain make_queries reads and among 10 000 planted chimeras (two random references,
           breakpoint 100 .. 558, 1 % substitutions) at 50 000 references.
    python tools/chimera_probe.py [--parent TREE] [--repeats 3] [--out profiles/chimera_probe.json]"""
import argparse
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
ap.add_argument("--timed", type=int, default=2, help="timed calls of a block (three blocks behind one warm-up call)")
ap.add_argument("--workloads", default="50000:100000,500000:65536", help="references:reads, comma separated")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()


def padded_rows(n_pos, S):
    b = [s * n_pos // S for s in range(S + 1)]
    return sum((b[s + 1] - b[s] + 7) // 8 * 8 for s in range(S))


def blocks(fn, timed):
    """Three blocks of `timed` calls behind one warm-up call: (median over the blocks of the block means, the block means)."""
    fn()
    means = []
    for _ in range(3):
        xs = [fn() for _ in range(timed)]
        means.append([float(np.mean([x[k] for x in xs])) for k in range(len(xs[0]))])
    return [float(np.median([m[k] for m in means])) for k in range(len(means[0]))], means


def child_speed(refs, reads):
    sys.path.insert(0, str(HERE))
    import raxtax_amd as rx
    from raxtax_amd import synth
    db = synth.make_db(refs)
    qs = synth.make_queries(db, reads)
    tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
    index = rx.Index(tree, tile_prune=False)
    stage = rx.Chimera(index)
    S, n_pos, tiles = 16, db.length - 7, (refs + 8191) // 8192
    got = {}

    def one():
        t0 = time.perf_counter()
        got["rec"] = stage.run(qs.bases, qs.base_off)
        return time.perf_counter() - t0, stage.kernel_ms() * 1e-3

    (dt, kt), means = blocks(one, args.timed)
    scan_bytes = 2 * padded_rows(n_pos, S) * tiles * 1024 * reads
    out = dict(references=refs, reads=reads, read_length=db.length, tiles=tiles, segments=S, padded_rows_per_read=padded_rows(n_pos, S),
               call_seconds=round(dt, 4), call_seconds_blocks=[round(m[0], 4) for m in means], reads_per_s=round(reads / dt),
               scan_kernel_seconds=round(kt, 4), scan_kernel_seconds_blocks=[round(m[1], 4) for m in means], scan_reads_per_s=round(reads / kt),
               scan_bytes_requested=scan_bytes, scan_bytes_per_s=round(scan_bytes / kt), flagged=int(got["rec"]["flag"].sum()),
               largest_delta=int(got["rec"]["delta"].max()))
    index.upload(qs.bases, qs.base_off)

    def plain():
        t0 = time.perf_counter()
        index.run(0)
        index.download(copy=False)
        return (time.perf_counter() - t0,)

    (ut,), umeans = blocks(plain, args.timed)
    out.update(unpruned_classify_seconds=round(ut, 4), unpruned_classify_seconds_blocks=[round(m[0], 4) for m in umeans], unpruned_reads_per_s=round(reads / ut),
               scan_over_unpruned_classify=round(kt / ut, 2), call_over_unpruned_classify=round(dt / ut, 2))
    if refs == 50_000:   # the definition at scale
        sys.path.insert(0, str(HERE / "tests"))
        import chimera_common as cc
        chim, _ = cc.planted_chimeras(db, n=10_000)
        rec = stage.run(*cc.concat(chim))
        out["scale"] = dict(plain_reads=reads, plain_flagged=int(got["rec"]["flag"].sum()), plain_largest_delta=int(got["rec"]["delta"].max()),
                            plain_delta_quantiles_50_99_999=[int(x) for x in np.quantile(got["rec"]["delta"], (0.5, 0.99, 0.999))],
                            chimeras=len(chim), chimeras_flagged=int(rec["flag"].sum()), chimeras_median_delta=int(np.median(rec["delta"])))
    print("PROBE " + json.dumps(out), flush=True)


if args.child:
    r, q = (int(x) for x in args.child.split(":"))
    child_speed(r, q)
    sys.exit(0)


def bench(root):
    p = subprocess.run([sys.executable, "bench.py"] + args.bench_args.split(), cwd=root, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
    if p.returncode != 0:   # (nothing more is started on the device behind a process that died)
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"bench.py in {root}: exit status {p.returncode}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["value"]


summary = dict(bench_args=args.bench_args, repeats=args.repeats)
if args.out and Path(args.out).exists():   # legs measured by an earlier call stay
    summary.update(json.loads(Path(args.out).read_text()))
if args.parent:
    legs = [("parent", str(Path(args.parent).resolve())), ("this", str(HERE))]
    runs = {name: [] for name, _ in legs}
    for rep in range(args.repeats):
        for name, root in legs:
            runs[name].append(bench(root))
            print(name, rep, runs[name][-1], flush=True)
    a, b = runs["parent"], runs["this"]
    summary["option_off"] = dict(parent=a, this=b, parent_min=min(a), parent_max=max(a), this_median=float(np.median(b)),
                                 this_inside_spread_of_parent=bool(min(a) <= float(np.median(b)) <= max(a)),
                                 this_over_parent_median=round(float(np.median(b)) / float(np.median(a)), 4))
for w in [x for x in args.workloads.split(",") if x]:
    p = subprocess.run([sys.executable, __file__, "--child", w, "--timed", str(args.timed)], capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=""))
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"workload {w}: exit status {p.returncode}")
    summary.setdefault("stage", {})[w] = json.loads([l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
    print(w, json.dumps(summary["stage"][w]), flush=True)
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

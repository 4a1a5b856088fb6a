#!/usr/bin/env python3
"""What paired-end merging (rtx_merge.hip, --reverse) costs: with the option off against the parent commit, and the stage itself.
    off    `python bench.py` (--bench-args) in a built checkout of the parent commit (--parent TREE) and in this tree, interleaved, --repeats
           runs each, every run a process of its own: the option is off when this tree's median lies inside the parent's own spread.
    stage  --pairs synthetic pairs of 2 x 250 bases whose overlap is uniform in 20 .. 230, Q falling along each mate from about 38 to about 12
           with noise and every base wrong with the probability its Q states, in a process of its own: rtx_merge_run alone, the kernel from HIP
           events (rtx_merge_kernel_time) and the call split into the host's staging pass, the copies with the wait around the kernel, and
           the kernel (rtx_merge_stage_times); the median of --timed calls behind a warm-up call; and rx.merge_pair, the same computation on
           ONE host thread called pair by pair from Python, over a sample of the same pairs.
    python tools/merge_probe.py [--parent TREE] [--repeats 3] [--pairs N] [--out profiles/merge_probe.json]"""
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
ap.add_argument("--pairs", type=int, default=1_000_000)
ap.add_argument("--timed", type=int, default=3, help="timed calls behind one warm-up call; their median is the figure")
ap.add_argument("--host-sample", type=int, default=5000, help="pairs the one-thread host function is timed on")
ap.add_argument("--out", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
W = 250


def pairs(rng, n):
    """F, QF, R, QR as [n, 250] arrays, and the true overlaps."""
    ov = rng.integers(20, 231, n)
    alen = 2 * W - ov
    amp = np.left_shift(np.uint8(1), rng.integers(0, 4, (n, 2 * W - 20), dtype=np.uint8))
    slope = (38 - (np.arange(W) * 26) // W).astype(np.int16)
    out = []
    for rev in (False, True):
        q = np.clip(slope[None, :] + rng.integers(-3, 4, (n, W), dtype=np.int16), 2, 41)
        idx = (alen[:, None] - 1 - np.arange(W)[None, :]) if rev else np.broadcast_to(np.arange(W)[None, :], (n, W))
        b = np.take_along_axis(amp, idx, axis=1)
        if rev:                                                # the complement: the four bits reversed
            b = ((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3)
        wrong = rng.random((n, W), dtype=np.float32) < np.float32(10.0) ** (-q.astype(np.float32) / np.float32(10.0))
        b = np.where(wrong, ((b << 1) | (b >> 3)) & 15, b).astype(np.uint8)   # another base
        out += [np.ascontiguousarray(b).reshape(-1), (33 + q).astype(np.uint8).reshape(-1)]
    return out, ov


def child():
    sys.path.insert(0, str(HERE))
    import raxtax_amd as rx
    n = args.pairs
    rng = np.random.default_rng(11)
    (fb, fq, rb, rq), ov = pairs(rng, n)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
    params = rx.MergeParams()
    stage = rx.Merge(0, params)
    ts, ks, parts = [], [], []
    for _ in range(1 + args.timed):
        t0 = time.perf_counter()
        got = stage.run(fb, fq, off, rb, rq, off)
        ts.append(time.perf_counter() - t0)
        ks.append(stage.kernel_ms())
        parts.append(stage.stage_seconds())
    mid = lambda xs: float(np.median(xs[1:]))
    overlap, diffs, verdict, mlen = got[:4]
    merged = verdict == 0
    m = min(args.host_sample, n)
    t0 = time.perf_counter()
    same = 0
    for i in range(m):
        r = rx.merge_pair(params, fb[i * W:(i + 1) * W], fq[i * W:(i + 1) * W], rb[i * W:(i + 1) * W], rq[i * W:(i + 1) * W])
        same += r[:3] == (int(overlap[i]), int(diffs[i]), int(verdict[i]))
    host = time.perf_counter() - t0
    out = dict(pairs=n, mate_bases=W, overlaps="uniform in 20 .. 230", params="defaults (min_overlap 16, max_diffs 10, max_diff_pct 100, q_cap 41)",
               python_call_seconds=round(mid(ts), 4), python_calls=[round(x, 4) for x in ts], kernel_ms=[round(x, 3) for x in ks],
               kernel_pairs_per_s=round(n / (mid(ks) * 1e-3)), kernel_input_bytes_per_s=round(n * 4 * W / (mid(ks) * 1e-3)),
               stage_seconds=round(mid([p[2] for p in parts]), 4), staging_seconds=round(mid([p[0] for p in parts]), 4),
               copies_and_wait_seconds=round(mid([p[1] for p in parts]), 4), kernel_seconds=round(mid(ks) * 1e-3, 5), stage_pairs_per_s=round(n / mid([p[2] for p in parts])),
               merged=int(merged.sum()), merged_at_the_true_overlap=int((merged & (overlap == ov)).sum()), merged_elsewhere=int((merged & (overlap != ov)).sum()),
               not_merged_by_verdict={name: int((verdict == (1 << b)).sum()) for b, name in enumerate(("bad_quality", "too_long", "too_short", "no_overlap"))},
               mean_diffs_of_merged=round(float(diffs[merged].mean()), 3),
               host_one_thread=dict(pairs=m, equal_to_the_device=int(same), seconds_through_python=round(host, 3), pairs_per_s_through_python=round(m / host)))
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
p = subprocess.run([sys.executable, __file__, "--child", "--pairs", str(args.pairs), "--timed", str(args.timed), "--host-sample", str(args.host_sample)], capture_output=True, text=True,
                   timeout=1500, env=dict(os.environ, PYTHONPATH=""))
if p.returncode != 0:
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    sys.exit(f"stage leg: exit status {p.returncode}")
summary["stage"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
print(json.dumps(summary, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

#!/usr/bin/env python3
"""What the taxon profile (rtx_index_profile_*, rtx_profile.hip) costs on the synthetic workload: the device step (run + sync + download,
inputs resident) of ONE handle, the median of K steps, with the profile closed and with it open; with it open also the time of the kernel
alone per download (HIP events around its launch, rtx_index_profile_time) and, with --check, the counters of one download against
checks.profile_expected.  One JSON line per condition; --out FILE appends them.
    python tools/profile_probe.py [--config 1|2] [--steps K] [--warmup W] [--repeat R] [--cutoff C] [--check] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import raxtax_amd as rx  # noqa: E402
from raxtax_amd import checks, synth  # noqa: E402

CONFIGS = {1: (50_000, 100_000), 2: (500_000, 1_000_000)}   # BASELINE.json configs[1] / configs[2]: references, queries

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS))
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeat", type=int, default=3, help="blocks of --steps steps per condition: the spread of their medians is the run-to-run spread")
ap.add_argument("--cutoff", type=float, default=0.8)
ap.add_argument("--check", action="store_true", help="hold the counters of one download against the numpy restatement (a Python loop over the queries)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
n_refs, n_q = CONFIGS[args.config]
db = synth.make_db(n_refs)
qs = synth.make_queries(db, n_q)
tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
index = rx.Index(tree, stage_timing=True)
index.upload(qs.bases, qs.base_off)
for _ in range(args.warmup):
    index.run(0)
    index.download(copy=False)
lines = []
for what in ("closed", "open", "closed again"):
    if what == "open":
        index.profile_begin(args.cutoff)
    blocks = []
    for _ in range(args.repeat):
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            index.run(0)
            index.sync()
            index.download(copy=False)
            ts.append(time.perf_counter() - t0)
        blocks.append(ts)
    medians = [float(np.median(b)) * 1e3 for b in blocks]
    line = dict(config=args.config, n_refs=n_refs, n_queries=n_q, condition=what, ms_per_step_median=round(float(np.median(medians)), 3),
                block_medians_ms=[round(m, 3) for m in medians], spread_ms=round(max(medians) - min(medians), 3),
                ms_per_step=[[round(t * 1e3, 3) for t in b] for b in blocks])
    if what == "open":
        ms, launches = index.profile_time()
        prof = index.profile_read()
        assert launches == args.repeat * args.steps and int(prof.totals[0]) == launches * n_q, (launches, prof.totals)
        line.update(profile_kernel_ms_per_download=round(ms / launches, 4), profile_kernel_launches=launches, totals_per_download=[int(t) // launches for t in prof.totals],
                    nodes=len(prof.clade), nodes_counted=int((prof.clade > 0).sum()),
                    share_of_step=round(ms / launches / float(np.median(medians)), 5))
        if args.check:
            index.profile_reset()
            index.run(0)
            res = index.download()
            ids, off = index.device_exact_matches()
            want = checks.profile_expected(tree.nodes(), res, off, ids, int(round(args.cutoff * 100)), True)
            got = index.profile_read()
            assert all(np.array_equal(g, w) for g, w in zip((got.clade, got.direct, got.conf_sum, got.totals), want[:4]))
            line.update(checked_against_numpy=True, kinds=want[4])
        index.profile_end()
    print(json.dumps(line), flush=True)
    lines.append(line)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))

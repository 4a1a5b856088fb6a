#!/usr/bin/env python3
"""What the alignment identity (RTX_OPT_IDENTITY) costs on the synthetic workload: the device step (run + sync + download, inputs resident),
the median of K steps, with RTX_OPT_NEAREST alone and with the identity on top; with it on also the time of the alignment kernels alone
(HIP events around their launches, rtx_batch_identity_time) and a check of a sample of queries against rtx_semiglobal_distance on the host.
One JSON line per condition; --out FILE appends them.
    python tools/identity_probe.py [--config 1|2] [--steps K] [--warmup W] [--repeat R] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import raxtax_amd as rx  # noqa: E402
from raxtax_amd import synth  # noqa: E402

CONFIGS = {1: (50_000, 100_000), 2: (500_000, 1_000_000)}   # BASELINE.json configs[1] / configs[2]: references, queries

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS))
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeat", type=int, default=3, help="blocks of --steps steps per condition: the spread of their medians is the run-to-run spread")
ap.add_argument("--out", default=None)
args = ap.parse_args()
n_refs, n_q = CONFIGS[args.config]
db = synth.make_db(n_refs)
qs = synth.make_queries(db, n_q)
tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
lines = []
for what, kw in (("nearest", {"nearest": True}), ("identity", {"identity": True})):
    index = rx.Index(tree, stage_timing=True, **kw)
    index.upload(qs.bases, qs.base_off)
    for _ in range(args.warmup):
        index.run(0)
        index.download(copy=False)
    blocks, kernel_ms = [], []
    for _ in range(args.repeat):
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            index.run(0)
            index.sync()
            if "identity" in kw:
                kernel_ms.append(index.identity_time()[0])
            index.download(copy=False)
            ts.append(time.perf_counter() - t0)
        blocks.append(ts)
    medians = [float(np.median(b)) * 1e3 for b in blocks]
    line = dict(config=args.config, n_refs=n_refs, n_queries=n_q, condition=what, ms_per_step_median=round(float(np.median(medians)), 3),
                block_medians_ms=[round(m, 3) for m in medians], spread_ms=round(max(medians) - min(medians), 3),
                ms_per_step=[[round(t * 1e3, 3) for t in b] for b in blocks], workspace_gb=round(index.workspace_bytes / 1e9, 3))
    if "identity" in kw:
        dist, qlen = index.identity()
        nearest, _ = index.nearest()
        orig = tree.original_index()   # reference id -> its place in db
        checked = 0
        for q in np.random.default_rng(1).choice(n_q, 24, replace=False):
            want = rx.NO_DIST if nearest[q] == rx.NO_REF else rx.semiglobal_distance(qs.seq(int(q)), db.seq(int(orig[int(nearest[q])])))
            assert int(dist[q]) == want and int(qlen[q]) == len(qs.seq(int(q))), (int(q), int(dist[q]), want)
            checked += 1
        have = dist != rx.NO_DIST
        line.update(identity_kernels_ms_median=round(float(np.median(kernel_ms)), 4), identity_kernels_ms_min=round(float(min(kernel_ms)), 4),
                    identity_kernels_ms_max=round(float(max(kernel_ms)), 4), with_distance=int(have.sum()),
                    dist_median=int(np.median(dist[have])) if have.any() else None, dist_max=int(dist[have].max()) if have.any() else None,
                    checked_against_host=checked)
    print(json.dumps(line), flush=True)
    lines.append(line)
    del index
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))

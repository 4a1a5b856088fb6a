#!/usr/bin/env python3
"""What naming the nearest reference (RTX_OPT_NEAREST) costs on the synthetic workload: the device step (run + sync + download, inputs
resident), the median of K steps, with the option off and with it on; with it on also the time of the new kernel alone (HIP events around
its launches, rtx_batch_nearest_time) and a check of the values of a sample of queries against counts recounted in full
(rtx_debug_hit_counts).  One JSON line per condition; --out FILE appends them.  RTX_PROBE_TREE=DIR measures the package of another checkout
(the parent commit, built there): a tree without the option gets the one condition it has, so that the three figures come from one script.
    python tools/nearest_probe.py [--config 1|2] [--steps K] [--warmup W] [--repeat R] [--out FILE]"""
import argparse
import inspect
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(os.environ.get("RTX_PROBE_TREE", Path(__file__).resolve().parent.parent))   # RTX_PROBE_TREE: the tree whose package is measured
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
has_option = "nearest" in inspect.signature(rx.Index.__init__).parameters
conditions = [("off", {}), ("on", {"nearest": True})] if has_option else [("parent", {})]
lines = []
for what, kw in conditions:
    index = rx.Index(tree, stage_timing=True, **kw)
    index.upload(qs.bases, qs.base_off)
    for _ in range(args.warmup):
        index.run(0)
        index.download(copy=False)
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
    line = dict(config=args.config, n_refs=n_refs, n_queries=n_q, condition=what, tree=str(ROOT.name), ms_per_step_median=round(float(np.median(medians)), 3),
                block_medians_ms=[round(m, 3) for m in medians], spread_ms=round(max(medians) - min(medians), 3),
                ms_per_step=[[round(t * 1e3, 3) for t in b] for b in blocks],
                stage_ms={s: round(v, 3) for s, (v, n) in index.stage_times().items() if n}, workspace_gb=round(index.workspace_bytes / 1e9, 3))
    if kw:
        ms, launches = index.nearest_time()
        nearest, ties = index.nearest()
        _, peak = index.strands()
        from raxtax_amd.checks import last_sub_batch_queries
        checked = 0
        for q in last_sub_batch_queries(index, n_q)[:24]:   # (the recounting tap reads the last sub-batch)
            counts = index.debug_hit_counts(int(q))
            m = int(counts.max())
            want = (int(np.argmax(counts)), int((counts == m).sum())) if m else (0xFFFFFFFF, 0)
            assert (int(nearest[q]), int(ties[q])) == want and int(peak[q]) == m, (int(q), int(nearest[q]), int(ties[q]), want)
            checked += 1
        line.update(nearest_kernel_ms=round(ms, 4), nearest_kernel_launches=launches, with_reference=int((nearest != 0xFFFFFFFF).sum()),
                    with_ties=int((ties >= 2).sum()), checked_against_recount=checked)
    print(json.dumps(line), flush=True)
    lines.append(line)
    del index
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))

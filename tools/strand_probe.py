#!/usr/bin/env python3
"""What both-strand mode (RTX_OPT_STRAND) costs on the synthetic workload: the device step (run + sync + download, inputs resident) with
stage times under strand plus, under strand both on the same all-forward queries, and under strand both on a copy with every second
query (seeded) reverse-complemented.  One JSON line per condition; --out FILE keeps them.
    python tools/strand_probe.py [--config 1|2] [--steps K] [--warmup W] [--out FILE]"""
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
ap.add_argument("--out", default=None)
args = ap.parse_args()
n_refs, n_q = CONFIGS[args.config]
db = synth.make_db(n_refs)
qs = synth.make_queries(db, n_q)
L = db.length
comp = np.arange(256, dtype=np.uint8)
comp[:16] = [int(f"{c:04b}"[::-1], 2) for c in range(16)]
flip = np.random.default_rng(17).random(n_q) < 0.5
mixed = qs.bases.reshape(n_q, L).copy()
mixed[flip] = comp[mixed[flip][:, ::-1]]
mixed = mixed.reshape(-1)
tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
lines = []
for what, strand, bases in (("plus", "plus", qs.bases), ("both, all forward", "both", qs.bases), ("both, half flipped", "both", mixed)):
    index = rx.Index(tree, stage_timing=True, strand=strand)
    index.upload(bases, qs.base_off)
    for _ in range(args.warmup):
        index.run(0)
        index.download(copy=False)
    ts = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        index.run(0)
        index.sync()
        index.download(copy=False)
        ts.append(time.perf_counter() - t0)
    strands, peaks = index.strands()
    if strand == "both":
        assert np.array_equal(strands.astype(bool), flip if bases is mixed else np.zeros(n_q, bool)), "a query was classified in the wrong orientation"
    ms = float(np.median(ts)) * 1e3
    line = dict(config=args.config, n_refs=n_refs, n_queries=n_q, condition=what, ms_per_step_median=round(ms, 2), ms_per_step=[round(t * 1e3, 2) for t in ts],
                queries_per_s=round(n_q / (ms / 1e3)), minus=int(strands.sum()), stage_ms={s: round(v, 2) for s, (v, n) in index.stage_times().items() if n},
                prune={k: round(v, 2) for k, v in index.debug_prune_stats().items() if k in ("queries_with_threshold", "record_queries", "live_tiles_per_query")},
                workspace_gb=round(index.workspace_bytes / 1e9, 2))
    print(json.dumps(line), flush=True)
    lines.append(line)
    del index
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(l) + "\n" for l in lines))

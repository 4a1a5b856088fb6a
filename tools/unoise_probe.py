#!/usr/bin/env python3
"""What denoising a run's distinct reads (rtx_otu_unoise, rtx_unoise.hip) costs, and what it finds.  The table is that of tools/otu_probe.py:
--centres random 658-base sequences with geometric abundances and their variants (one substitution, two substitutions, one deletion, one
insertion; 1 .. a few reads each), about --rows rows.
    device    one warm-up call, then the median of --repeats calls: the four times of the view (upload, pair kernels, bookkeeping, download),
              the wall time of the call, the status counts, the tiers and launches, the pairs handed to the kernel, dropped by the length
              test and run to the last column, and the microseconds of pair kernel per pair handed over
    quality   how many planted centres are ZOTUs; of the variants that the rule lets their own centre absorb (light enough for their
              distance), how many it did absorb into that centre; of the others, how many ended up anywhere else
    host      the wall time of rtx_otu_unoise_host, one thread, on a table of --host-rows rows made the same way (0: never) and its
              microseconds per pair (every pair is a full 658 x 658 table there), with the device's result on that table for equality
    python tools/unoise_probe.py [--rows 100000] [--centres 5000] [--repeats 3] [--host-rows 500] [--out profiles/unoise_probe.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))
import raxtax_amd as rx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000)
ap.add_argument("--centres", type=int, default=5000)
ap.add_argument("--length", type=int, default=658)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--host-rows", type=int, default=500, help="the host restatement runs on a table of this many rows (a full table per pair: seconds at 500)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.length
KIND_DIFFS = (1, 2, 1, 1)


def make_rows(n_rows, rng):
    """tools/otu_probe.py's rows: [(matrix of rows of one length, weights, centre of every row, differences)], the centres first"""
    nc = min(args.centres, max(1, n_rows // 20))
    centres = (1 << rng.integers(0, 4, (nc, L))).astype(np.uint8)
    out = [(centres, (10 + rng.geometric(0.02, nc)).astype(np.uint32), np.arange(nc), 0)]
    nv = n_rows - nc
    src = rng.integers(0, nc, nv)
    kind = rng.choice(4, nv, p=[0.60, 0.20, 0.12, 0.08])
    for k in range(4):
        c = centres[src[kind == k]]
        m = len(c)
        rows = np.arange(m)
        if k <= 1:
            v = c.copy()
            for _ in range(k + 1):
                pos = rng.integers(0, L, m)
                v[rows, pos] = np.roll(np.array([1, 2, 4, 8], np.uint8), 1 + int(rng.integers(0, 3)))[np.log2(v[rows, pos]).astype(np.int64)]
        elif k == 2:
            pos = rng.integers(0, L, m)
            idx = np.arange(L - 1)[None, :] + (np.arange(L - 1)[None, :] >= pos[:, None])
            v = np.take_along_axis(c, idx, axis=1)
        else:
            pos = rng.integers(0, L + 1, m)
            j = np.arange(L + 1)[None, :]
            v = np.take_along_axis(c, np.minimum(j - (j > pos[:, None]), L - 1), axis=1)
            v[rows, pos] = (1 << rng.integers(0, 4, m)).astype(np.uint8)
        out.append((np.ascontiguousarray(v), rng.geometric(0.6, m).astype(np.uint32), src[kind == k], KIND_DIFFS[k]))
    return out


def make_table(parts):
    table = None
    for m, w, _, _ in parts:
        n, length = m.shape
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
        if table is None:
            table = rx.tally_reads(m.reshape(-1), off, None, w)
        else:
            table.add(m.reshape(-1), off, None, w)
    return table


def quality(table, parts, got):
    """the planted rows looked up by their bytes (equal rows were summed by the table: such a row is judged by the table's weight)"""
    rank = {bytes(s): r for r, s in enumerate(table.seqs)}
    sizes, u = table.sizes, got.unoise
    centres = parts[0][0]
    crank = np.array([rank[bytes(c)] for c in centres])
    q = dict(centres=len(centres), centres_zotu=int((u["status"][crank] == 0).sum()), variants=0, allowed=0, allowed_absorbed_by_own_centre=0, not_allowed=0,
             not_allowed_absorbed=0)
    for m, _, src, d in parts[1:]:
        for row, c in zip(m, src):
            r = rank[bytes(row)]
            q["variants"] += 1
            ok = (int(sizes[crank[c]]) >> (2 * d + 1)) >= int(sizes[r])
            if ok:
                q["allowed"] += 1
                q["allowed_absorbed_by_own_centre"] += int(u["status"][r] == 1 and u["parent"][r] == crank[c])
            else:
                q["not_allowed"] += 1
                q["not_allowed_absorbed"] += int(u["status"][r] == 1)
    return q


rng = np.random.default_rng(args.rows)
parts = make_rows(args.rows, rng)
table = make_table(parts)
rows = len(table.sizes)
calls = []
for k in range(1 + args.repeats):
    t0 = time.perf_counter()
    z = rx.otu_unoise(table)
    calls.append(dict(wall=time.perf_counter() - t0, seconds=z.unoise["seconds"]))
timed = calls[1:]
med = [float(np.median([c["seconds"][i] for c in timed])) for i in range(4)]
u = z.unoise
line = dict(rows=rows, otus=int(z.n_otus), zotu=u["n_zotu"], absorbed=u["n_absorbed"], left=u["n_left"], long=u["n_long"], tiers=u["tiers"], launches=u["launches"],
            pairs=u["pairs"], pairs_dropped_by_length=u["pairs_length"], pairs_finished=u["pairs_finished"], upload_seconds=round(med[0], 5), pair_kernel_seconds=round(med[1], 5),
            bookkeeping_seconds=round(med[2], 5), download_seconds=round(med[3], 5), device_wall_seconds=round(float(np.median([c["wall"] for c in timed])), 5),
            device_wall_calls=[round(c["wall"], 5) for c in calls], pair_kernel_seconds_calls=[round(c["seconds"][1], 5) for c in calls],
            us_per_pair=round(med[1] * 1e6 / max(u["pairs"], 1), 5))
print(json.dumps(line), flush=True)
qual = quality(table, parts, z)
print(json.dumps(qual), flush=True)
summary = dict(workload=dict(rows_asked=args.rows, centres=args.centres, length=L, repeats=args.repeats, minsize=u["minsize"], alpha=u["alpha"], max_diffs=u["max_diffs"]),
               device=line, quality=qual)
if args.host_rows:
    small = make_table(make_rows(args.host_rows, np.random.default_rng(args.host_rows)))
    d = rx.otu_unoise(small)
    t0 = time.perf_counter()
    h = rx.otu_unoise_host(small)
    wall = time.perf_counter() - t0
    equal = all(np.array_equal(h.unoise[k], d.unoise[k]) for k in ("status", "parent", "dist", "lim")) and np.array_equal(h.otu, d.otu)
    summary["host"] = dict(rows=len(small.sizes), fraction_of_rows=round(len(small.sizes) / rows, 5), pairs=d.unoise["pairs"], wall_seconds=round(wall, 3),
                           us_per_pair=round(wall * 1e6 / max(d.unoise["pairs"], 1), 2), equal=bool(equal),
                           device_pair_kernel_seconds=round(d.unoise["seconds"][1], 6))
    print(json.dumps(summary["host"]), flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

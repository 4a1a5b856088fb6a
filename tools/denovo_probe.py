#!/usr/bin/env python3
"""What the de novo chimera check of a run (rtx_denovo_check, rtx_denovo.hip) costs.  The table is that of tools/otu_probe.py (--centres random
658-base sequences with geometric abundances and their variants, about --rows rows) with --chimeras planted chimeras of two centres, each at
a quarter of the rarer parent's abundance or less; it is clustered first (rx.otu_cluster) and the OTUs are checked.
    device    one warm-up call, then the median of --repeats calls: the four times of rtx_denovo_times (upload and bitmap, scans, the rounds'
              bookkeeping, download), the wall time of the call, rounds, scans, the share of the planted chimeras and of the centres that are
              flagged
    yardstick rx.Chimera on an Index of the same parents (the entries below the largest lim) over the same sequences: milliseconds of its
              scan kernels per (read, tile) wave pair, against the scan seconds of a de novo call that takes ONE round (mindelta above any
              count, so that nothing is flagged) per (entry, tile) wave pair.  Both are HIP events around the scan kernels alone; the
              masked checkpoint and the triangular grid are the only differences.
    host      the wall time of rtx_denovo_check_host, one thread (--host-entries: only up to that many entries; 0: never).  --host-only: no
              device at all -- the table is clustered and checked on the host, and only this part is reported
    python tools/denovo_probe.py [--rows 100000] [--centres 5000] [--chimeras 500] [--repeats 3] [--host-entries 100000] [--out profiles/denovo_probe.json]"""
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
ap.add_argument("--chimeras", type=int, default=500)
ap.add_argument("--length", type=int, default=658)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--host-entries", type=int, default=100_000, help="the host restatement runs on up to this many entries (minutes at the default workload)")
ap.add_argument("--host-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.length


def make_rows(n_rows, rng):
    """tools/otu_probe.py's rows: [(matrix of rows of one length, weights)], the centres first"""
    nc = min(args.centres, max(1, n_rows // 20))
    centres = (1 << rng.integers(0, 4, (nc, L))).astype(np.uint8)
    out = [(centres, (10 + rng.geometric(0.02, nc)).astype(np.uint32))]
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
        out.append((np.ascontiguousarray(v), rng.geometric(0.6, m).astype(np.uint32)))
    return out


def plant(parts, rng):
    centres, w = parts[0]
    nc = len(centres)
    a, b = rng.integers(0, nc, args.chimeras), rng.integers(0, nc, args.chimeras)
    b = np.where(a == b, (b + 1) % nc, b)
    bp = rng.integers(L // 4, 3 * L // 4, args.chimeras)
    chim = np.where(np.arange(L)[None, :] < bp[:, None], centres[a], centres[b])
    return np.ascontiguousarray(chim), np.maximum(1, np.minimum(w[a], w[b]) // 4).astype(np.uint32)


def make_table(parts):
    table = None
    for m, w in parts:
        n, length = m.shape
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(length)
        if table is None:
            table = rx.tally_reads(m.reshape(-1), off, None, w)
        else:
            table.add(m.reshape(-1), off, None, w)
    return table


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), off


rng = np.random.default_rng(args.rows)
parts = make_rows(args.rows, rng)
chim, chim_w = plant(parts, rng)
table = make_table(parts + [(chim, chim_w)])
rows = len(table.sizes)
if args.host_only:
    otus = rx.otu_cluster_host(table)
    t0 = time.perf_counter()
    h = rx.denovo_check_host(table, otus)
    host = dict(rows=rows, entries=h.n_entries, parents=int(h.lim.max()), flagged=h.n_flagged, wall_seconds=round(time.perf_counter() - t0, 3))
    print(json.dumps(host), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(dict(host=host), indent=1) + "\n")
    sys.exit(0)
otus = rx.otu_cluster(table)
calls = []
for k in range(1 + args.repeats):
    t0 = time.perf_counter()
    d = rx.denovo_check(table, otus)
    calls.append(dict(wall=time.perf_counter() - t0, seconds=d.seconds))
timed = calls[1:]
med = [float(np.median([c["seconds"][i] for c in timed])) for i in range(4)]
seqs = table.seqs
entry_seq = [seqs[int(r)] for r in d.row]
flag_of = {bytes(s): int(f) for s, f in zip(entry_seq, d.rec["flag"])}
planted = [flag_of.get(bytes(c)) for c in chim]      # (None: the chimera is not a seed -- it fell into an OTU)
centre_flags = [flag_of.get(bytes(c)) for c in parts[0][0]]
tiles = (d.lim.astype(np.int64) + 8191) // 8192
line = dict(rows=rows, otus=int(otus.n_otus), entries=d.n_entries, parents=int(d.lim.max()) if d.n_entries else 0, checked=d.n_checked, flagged=d.n_flagged, rounds=d.rounds,
            scans=d.scans, upload_bitmap_seconds=round(med[0], 5), scan_seconds=round(med[1], 5), bookkeeping_seconds=round(med[2], 5), download_seconds=round(med[3], 5),
            device_wall_seconds=round(float(np.median([c["wall"] for c in timed])), 5), device_wall_calls=[round(c["wall"], 5) for c in calls],
            planted=len(chim), planted_as_seeds=sum(f is not None for f in planted), planted_flagged=sum(f == 1 for f in planted),
            centres=len(centre_flags), centres_as_seeds=sum(f is not None for f in centre_flags), centres_flagged=sum(f == 1 for f in centre_flags))
print(json.dumps(line), flush=True)

# the yardstick: one round of the de novo scan against the reference-based scan of the same sequences over the same parents
one = [rx.denovo_check(table, otus, mindelta=5000) for _ in range(1 + args.repeats)][1:]
assert all(o.rounds == 1 and o.n_flagged == 0 for o in one)
pairs = int(tiles.sum())
n_par = int(d.lim.max())
bases, off = concat(entry_seq[:n_par])
index = rx.Index(rx.Tree.new_flat([f"p:P,c:C,o:O,f:F,g:G,s:S{i}" for i in range(n_par)], bases, off))
stage = rx.Chimera(index)
qb, qo = concat(entry_seq)
ms = []
for k in range(1 + args.repeats):
    stage.run(qb, qo)
    ms.append(stage.kernel_ms())
ref_pairs = len(entry_seq) * ((n_par + 8191) // 8192)
yard = dict(denovo_one_round_scan_seconds=round(float(np.median([o.seconds[1] for o in one])), 5), denovo_wave_pairs=pairs,
            chimera_scan_seconds=round(float(np.median(ms[1:])) * 1e-3, 5), chimera_wave_pairs=ref_pairs)
yard["denovo_us_per_pair"] = round(yard["denovo_one_round_scan_seconds"] * 1e6 / max(pairs, 1), 3)
yard["chimera_us_per_pair"] = round(yard["chimera_scan_seconds"] * 1e6 / max(ref_pairs, 1), 3)
yard["ratio"] = round(yard["denovo_us_per_pair"] / yard["chimera_us_per_pair"], 3) if yard["chimera_us_per_pair"] else None
print(json.dumps(yard), flush=True)
summary = dict(workload=dict(rows_asked=args.rows, centres=args.centres, chimeras=args.chimeras, length=L, repeats=args.repeats), device=line, yardstick=yard)
if args.host_entries and d.n_entries <= args.host_entries:
    t0 = time.perf_counter()
    h = rx.denovo_check_host(table, otus)
    summary["host"] = dict(wall_seconds=round(time.perf_counter() - t0, 3), equal=bool(np.array_equal(h.rec, d.rec)))
    summary["host"]["host_over_device"] = round(summary["host"]["wall_seconds"] / line["device_wall_seconds"], 1)
else:
    summary["host"] = dict(skipped=f"{d.n_entries} entries, above --host-entries {args.host_entries}")
print(json.dumps(summary["host"]), flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

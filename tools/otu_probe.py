#!/usr/bin/env python3
"""What the OTUs of a run (rtx_otu_cluster, rtx_otu.hip) cost, and what the host restatement (rtx_otu_cluster_host) costs on the same table.
The table: --centres random 658-base sequences with geometric abundances; each spawns variants -- one substitution (60 %), two substitutions
(20 %), one deletion (12 %), one insertion (8 %), abundances 1, 2, .. geometric -- until the table has about --rows rows (equal variants
collapse in the table: the row count is what the table says).  One column.
    device   one warm-up call, then the median of --repeats calls: the four times of rtx_otu_times (upload and table layout, link passes, label
             rounds and numbering, download and sort), the wall time of the call, rounds, links, OTUs, and probes per second: the variants
             the link kernel looks up (three or four substitutions per position, one deletion per run of equal codes) over the link time
    host     the wall time of one rtx_otu_cluster_host call, one thread (--host-rows: only for tables up to that many rows; 0: never)
    cli      (--cli READS) raxtax-hip --uniques with and without --otus on READS reads drawn from the table by abundance, against a database
             of --cli-refs of the centres, --cli-repeats times each, interleaved; wall seconds of the process
    python tools/otu_probe.py [--rows 100000,1000000] [--centres 50000] [--repeats 5] [--host-rows 200000] [--cli 1000000] [--out profiles/otu_probe.json]"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))
import raxtax_amd as rx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", default="100000,1000000")
ap.add_argument("--centres", type=int, default=50_000)
ap.add_argument("--length", type=int, default=658)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=200_000, help="the host restatement runs on tables up to this many rows (at 1 M rows it takes more than a quarter of an hour)")
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--cli-refs", type=int, default=5000)
ap.add_argument("--cli-repeats", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.length


def make_rows(n_rows, rng):
    """[(matrix of rows of one length, weights)]: the centres, then their variants"""
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


def probes(parts):
    """the lookups of the link kernel: per row 3 substitutions per position (the codes are plain) and one deletion per run"""
    return int(sum(3 * m.size + m.shape[0] + int((m[:, 1:] != m[:, :-1]).sum()) for m, _ in parts))


def measure(n_rows):
    rng = np.random.default_rng(n_rows)
    parts = make_rows(n_rows, rng)
    table = make_table(parts)
    rows = len(table.sizes)
    calls = []
    for k in range(1 + args.repeats):
        t0 = time.perf_counter()
        o = rx.otu_cluster(table)
        calls.append(dict(wall=time.perf_counter() - t0, seconds=o.seconds))
    timed = calls[1:]
    med = [float(np.median([c["seconds"][i] for c in timed])) for i in range(4)]
    n_probes = probes(parts)   # (of the rows given; the few that collapse in the table are counted: an upper bound within a fraction of a percent)
    line = dict(rows=rows, rows_asked=n_rows, links=int(len(o.links)), otus=int(o.n_otus), rounds=o.rounds, link_passes=o.link_passes,
                upload_seconds=round(med[0], 5), link_seconds=round(med[1], 5), label_seconds=round(med[2], 5), download_seconds=round(med[3], 5),
                device_wall_seconds=round(float(np.median([c["wall"] for c in timed])), 5), device_wall_calls=[round(c["wall"], 5) for c in calls],
                probes=n_probes, probes_per_second=round(n_probes / med[1]))
    if args.host_rows and rows <= args.host_rows:
        t0 = time.perf_counter()
        h = rx.otu_cluster_host(table)
        line["host_wall_seconds"] = round(time.perf_counter() - t0, 4)
        assert np.array_equal(h.otu, o.otu) and np.array_equal(h.links, o.links)
        line["host_over_device"] = round(line["host_wall_seconds"] / line["device_wall_seconds"], 2)
    return line, parts


def cli_leg(parts, n_reads):
    """raxtax-hip --uniques with and without --otus over reads drawn from the rows by abundance"""
    from raxtax_amd import synth
    rng = np.random.default_rng(7)
    dec = np.frombuffer(b"?AC?G???T??????N", dtype=np.uint8)
    cli = HERE / "raxtax_amd" / "raxtax-hip"
    out = dict(reads=n_reads, references=args.cli_refs, with_otus=[], without_otus=[])
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        centres = parts[0][0][:args.cli_refs]
        synth.write_fasta(d / "db.fasta", [f"r{i};tax=k,p,c,o,f{i % 50},g{i % 500},s{i};" for i in range(len(centres))], centres.reshape(-1),
                          np.arange(len(centres) + 1, dtype=np.uint64) * np.uint64(L))
        with open(d / "reads.fasta", "wb") as fh:
            total = sum(int(w.sum()) for _, w in parts)
            n = 0
            for m, w in parts:
                take = rng.choice(len(m), max(1, n_reads * int(w.sum()) // total), p=w / w.sum())
                for a in range(0, len(take), 50_000):
                    rows = dec[m[take[a:a + 50_000]]]
                    fh.write(b"".join(b">q%d\n" % (n + i) + rows[i].tobytes() + b"\n" for i in range(len(rows))))
                    n += len(rows)
        for rep in range(args.cli_repeats):
            for name, extra in (("without_otus", []), ("with_otus", ["--otus"])):
                t0 = time.perf_counter()
                p = subprocess.run([str(cli), "-d", str(d / "db.fasta"), "-i", str(d / "reads.fasta"), "-o", str(d / name), "--redo", "--uniques", *extra],
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:   # (nothing more is started on the device behind a process that failed)
                    sys.exit(f"raxtax-hip {name}: exit status {p.returncode}\n{p.stderr[-2000:]}")
                out[name].append(round(time.perf_counter() - t0, 3))
                if extra:
                    out["info"] = [l for l in p.stderr.splitlines() if "--otus:" in l][:1]
    out["otus_add_seconds"] = round(float(np.median(out["with_otus"]) - np.median(out["without_otus"])), 3)
    return out


summary = dict(workload=dict(centres=args.centres, length=L, repeats=args.repeats, columns=1), tables=[])
parts = None
for n_rows in [int(x) for x in args.rows.split(",")]:
    line, parts = measure(n_rows)
    summary["tables"].append(line)
    print(json.dumps(line), flush=True)
if args.cli:
    summary["cli"] = cli_leg(parts, args.cli)
    print(json.dumps(summary["cli"]), flush=True)
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

#!/usr/bin/env python3
"""What the consensus taxonomy of the OTUs (rtx_otu_taxonomy, rtx_otutax.hip) costs on the tables of tools/otu_probe.py.
The table: --centres random 658-base sequences with geometric abundances and their variants until the table has about --rows rows, drawn
exactly as tools/otu_probe.py draws them (the same generator, the same seeds: the same tables); its OTUs by rtx_otu_cluster, not timed here.
The records are synthetic, over the taxonomy of the benchmark's database (fan-outs 3, 4, 5, 6, 6, 6: 12 960 species, 15 556 nodes): every OTU
has a species of its own; a row reaches it with 6 levels (60 %), fewer (25 %, the cut drawn evenly), a sibling species of the same genus
(10 %) or nothing (5 %, either kind); hundredths 80 .. 100.
    device   one warm-up call, then the median of --repeats calls: the four times of the call (checks, plan and upload; path kernel; consensus
             kernels; download) and its wall time, the plan (packed waves, workgroups), the OTUs with a taxon
    host     the wall time of one rtx_otu_taxonomy_host call, one thread, the result held against the device's field by field
    cli      with --cli N: raxtax-hip --uniques --otus with and without --otus-tax 0.8 over N reads drawn from the first table by abundance
             against --cli-refs of the centres, --cli-repeats processes each, interleaved: wall seconds, and the seconds of the second pass as
             the run logs them
    python tools/otutax_probe.py [--rows 100000,1000000] [--centres 50000] [--repeats 5] [--cli 1000000] [--out profiles/otutax_probe.json]"""
import argparse
import json
import re
import sys
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
ap.add_argument("--cli", type=int, default=0)
ap.add_argument("--cli-refs", type=int, default=5000)
ap.add_argument("--cli-repeats", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.length
FANOUTS = (3, 4, 5, 6, 6, 6)


def make_rows(n_rows, rng):
    """[(matrix of rows of one length, weights)]: the centres, then their variants (tools/otu_probe.py, make_rows)"""
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


def taxonomy():
    """parent [nodes] of the complete tree with these fan-outs, breadth first, and the first node of every level"""
    parent, first = [0xFFFFFFFF], [0, 1]
    level = [0]
    for f in FANOUTS:
        nxt = []
        for v in level:
            for _ in range(f):
                nxt.append(len(parent))
                parent.append(v)
        level = nxt
        first.append(len(parent))
    return np.array(parent, np.uint32), first


def records(otus, parent, first, rng):
    n, depth = otus.n_rows, len(FANOUTS)
    n_species = first[depth + 1] - first[depth]
    species = first[depth] + rng.integers(0, n_species, otus.n_otus)[otus.otu]          # the OTU's own species, per row
    u = rng.random(n)
    sibling = (u >= 0.85) & (u < 0.95)
    genus = parent[species]
    species = np.where(sibling, first[depth] + (genus - first[depth - 1]) * FANOUTS[-1] + rng.integers(0, FANOUTS[-1], n), species).astype(np.uint32)
    lv = np.where(u < 0.60, depth, np.where(u < 0.85, rng.integers(1, depth, n), np.where(u < 0.95, depth, 0))).astype(np.uint8)
    node = species.copy()
    for d in range(depth, 0, -1):                                                          # up to level L
        node = np.where(lv < d, parent[node], node)
    node = np.where(lv == 0, 0, node).astype(np.uint32)
    kind = np.where(lv > 0, 2, rng.integers(0, 2, n)).astype(np.uint8)
    hund = rng.integers(80, 101, (n, depth)).astype(np.uint8)
    hund[np.arange(depth)[None, :] >= lv[:, None]] = 0
    return rx.Lineages(kind, lv, node, hund)


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("sizes", "members", "classified", "depth", "node", "seed_rel", "clade", "conf"))


def measure(n_rows, parent, first):
    rng = np.random.default_rng(n_rows)
    table = make_table(make_rows(n_rows, rng))
    otus = rx.otu_cluster(table)
    lin = records(otus, parent, first, np.random.default_rng(n_rows + 1))
    calls = []
    for _ in range(1 + args.repeats):
        t0 = time.perf_counter()
        tax = rx.otu_taxonomy(parent, otus, lin)
        calls.append(dict(wall=time.perf_counter() - t0, seconds=tax.seconds))
    med = [float(np.median([c["seconds"][i] for c in calls[1:]])) for i in range(4)]
    t0 = time.perf_counter()
    host = rx.otu_taxonomy_host(parent, otus, lin)
    host_wall = time.perf_counter() - t0
    assert same(tax, host), "device and host differ"
    return dict(rows=int(otus.n_rows), rows_asked=n_rows, otus=int(otus.n_otus), nodes=len(parent), largest_otu=int(otus.members.max()), singletons=int((otus.members == 1).sum()),
                packed_waves=tax.packed_waves, workgroups=tax.big_otus, otus_with_taxon=int((tax.depth > 0).sum()), otus_at_species=int((tax.depth == len(FANOUTS)).sum()),
                upload_and_plan_seconds=round(med[0], 5), path_kernel_seconds=round(med[1], 5), consensus_kernel_seconds=round(med[2], 5), download_seconds=round(med[3], 5),
                device_wall_seconds=round(float(np.median([c["wall"] for c in calls[1:]])), 5), device_wall_calls=[round(c["wall"], 5) for c in calls],
                host_wall_seconds=round(host_wall, 5), host_equals_device=True)


def cli_leg(n_rows, n_reads):
    """raxtax-hip --uniques --otus with and without --otus-tax 0.8, the processes interleaved (tools/otu_probe.py, cli_leg)"""
    import subprocess
    import tempfile
    from raxtax_amd import synth
    parts = make_rows(n_rows, np.random.default_rng(n_rows))
    rng = np.random.default_rng(7)
    dec = np.frombuffer(b"?AC?G???T??????N", dtype=np.uint8)
    cli = HERE / "raxtax_amd" / "raxtax-hip"
    out = dict(reads=n_reads, references=args.cli_refs, without_seconds=[], with_seconds=[], second_pass_seconds=[], info=[])
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
                rows = dec[m[take]]
                fh.write(b"".join(b">q%d\n" % (n + i) + rows[i].tobytes() + b"\n" for i in range(len(rows))))
                n += len(rows)
        for rep in range(args.cli_repeats):
            for name, extra in (("without", []), ("with", ["--otus-tax", "0.8"])):
                t0 = time.perf_counter()
                p = subprocess.run([str(cli), "-d", str(d / "db.fasta"), "-i", str(d / "reads.fasta"), "-o", str(d / name), "--redo", "--skip-db", "--uniques", "--otus", *extra],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:   # (nothing more is started on the device behind a process that failed)
                    sys.exit(f"raxtax-hip {name}: exit status {p.returncode}\n{p.stderr[-2000:]}")
                out[name + "_seconds"].append(round(time.perf_counter() - t0, 3))
                for line in p.stderr.splitlines():
                    m = re.search(r"--otus-tax: .* ([0-9.]+) s for the second pass", line)
                    if m:
                        out["second_pass_seconds"].append(float(m.group(1)))
                    if rep == 0 and ("--otus:" in line or "--otus-tax:" in line) and name == "with":
                        out["info"].append(line)
    out["second_pass_share_of_the_run"] = round(float(np.median(out["second_pass_seconds"])) / float(np.median(out["with_seconds"])), 4)
    return out


parent, first = taxonomy()
summary = dict(workload=dict(centres=args.centres, length=L, repeats=args.repeats, fanouts=FANOUTS, nodes=len(parent)), tables=[])
for n_rows in [int(x) for x in args.rows.split(",") if x]:
    line = measure(n_rows, parent, first)
    summary["tables"].append(line)
    print(json.dumps(line), flush=True)
    if args.out:   # (what is measured so far is kept: a later table may take long)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
if args.cli:
    summary["cli"] = cli_leg(int(args.rows.split(",")[0]), args.cli)
    print(json.dumps(summary["cli"]), flush=True)
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

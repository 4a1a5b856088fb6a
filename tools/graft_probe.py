#!/usr/bin/env python3
"""What the fastidious grafting (rtx_otu_graft, rtx_graft.hip) costs on the tables of tools/otu_probe.py, and what it leaves of their OTUs.
The table: --centres random 658-base sequences with geometric abundances; each spawns variants -- one substitution (60 %), two substitutions
(20 %), one deletion (12 %), one insertion (8 %) -- until the table has about --rows rows; drawn exactly as tools/otu_probe.py draws them (the
same generator, the same seeds: the same tables).  The clustering (rtx_otu_cluster) is made once per table and is not timed here.
    device   one warm-up call, then the median of --repeats calls: the five times of the graft (upload and table layout, Bloom, test, verify,
             resolve and download), the wall time of the call, the filter's bytes, the strings inserted, candidates and confirmed candidates
             and from them the measured false-positive rate (candidates that no heavy row stands behind, over the strings tested), OTUs before
             and after, and strings hashed per second: those inserted over the Bloom time, those tested over the test time
    host     the wall time of one rtx_otu_graft_host call, one thread, on the table of --host-rows rows -- when its map fits --host-bytes
             (every string of every heavy row's ball is kept as bytes: rows x 9 x length x length)
    python tools/graft_probe.py [--rows 100000,1000000] [--centres 50000] [--repeats 5] [--host-rows 20000] [--out profiles/graft_probe.json]"""
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
ap.add_argument("--rows", default="100000,1000000")
ap.add_argument("--centres", type=int, default=50_000)
ap.add_argument("--length", type=int, default=658)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=20_000, help="the host restatement runs on a table of this many rows (0: never)")
ap.add_argument("--host-bytes", type=int, default=8 << 30, help="... if the strings of its map stay below this many bytes")
ap.add_argument("--cli", type=int, default=0, help="raxtax-hip --uniques --otus --fastidious on this many reads drawn from the last table by abundance")
ap.add_argument("--cli-refs", type=int, default=5000)
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.length


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


def ball_size(lengths):
    """the strings of B1 of rows over A, C, G, T, within a run of equal codes per row: itself, 3 substitutions and at most one deletion per
    position, 3 insertions per place and one more at the end"""
    return int((1 + 3 * lengths + lengths + 3 * (lengths + 1) + 1).sum())


def measure(n_rows):
    rng = np.random.default_rng(n_rows)
    table = make_table(make_rows(n_rows, rng))
    before = rx.otu_cluster(table)
    calls = []
    for k in range(1 + args.repeats):
        t0 = time.perf_counter()
        g = rx.otu_graft(before)
        calls.append(dict(wall=time.perf_counter() - t0, seconds=g.graft_info["seconds"]))
    timed = calls[1:]
    med = [float(np.median([c["seconds"][i] for c in timed])) for i in range(5)]
    info = g.graft_info
    lengths = np.array([len(s) for s in table.seqs])
    light = g.parent != 0xFFFFFFFF
    light_rows = np.flatnonzero(before.sizes[before.otu] < info["boundary"])
    tested = ball_size(lengths[light_rows])     # (an upper bound: a deletion is taken once per run of equal codes)
    false = info["candidates"] - info["confirmed"]
    line = dict(rows=int(before.n_rows), rows_asked=n_rows, boundary=info["boundary"], otus_before=int(before.n_otus), otus_after=int(g.n_otus), grafts=info["grafts"],
                heavy_otus=info["heavy_otus"], light_otus=info["light_otus"], heavy_rows=info["heavy_rows"], light_rows=info["light_rows"], light_rows_with_parent=int(light.sum()),
                bloom_log2=info["bloom_log2"], filter_bytes=(1 << info["bloom_log2"]) // 8, bits_per_string=round((1 << info["bloom_log2"]) / max(1, info["variants"]), 2),
                strings_inserted=info["variants"], strings_tested_upper_bound=tested, candidates=info["candidates"], confirmed=info["confirmed"], test_passes=info["test_passes"],
                false_positive_rate=false / max(1, tested), false_positive_rate_estimate=0.0024,
                upload_seconds=round(med[0], 5), bloom_seconds=round(med[1], 5), test_seconds=round(med[2], 5), verify_seconds=round(med[3], 5), resolve_seconds=round(med[4], 5),
                device_wall_seconds=round(float(np.median([c["wall"] for c in timed])), 5), device_wall_calls=[round(c["wall"], 5) for c in calls],
                inserted_per_second=round(info["variants"] / max(med[1], 1e-9)), tested_per_second=round(tested / max(med[2], 1e-9)))
    return line


def cli_leg(n_rows, n_reads):
    """raxtax-hip --uniques --otus with and without --fastidious over reads drawn from the rows by abundance (tools/otu_probe.py, cli_leg): the
    [INFO ] lines of both stages and the wall seconds of the two processes"""
    import subprocess
    import tempfile
    from raxtax_amd import synth
    parts = make_rows(n_rows, np.random.default_rng(n_rows))
    rng = np.random.default_rng(7)
    dec = np.frombuffer(b"?AC?G???T??????N", dtype=np.uint8)
    cli = HERE / "raxtax_amd" / "raxtax-hip"
    out = dict(reads=n_reads, references=args.cli_refs)
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
        for name, extra in (("without_fastidious", []), ("with_fastidious", ["--fastidious"])):
            t0 = time.perf_counter()
            p = subprocess.run([str(cli), "-d", str(d / "db.fasta"), "-i", str(d / "reads.fasta"), "-o", str(d / name), "--redo", "--uniques", "--otus", *extra],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # (nothing more is started on the device behind a process that failed)
                sys.exit(f"raxtax-hip {name}: exit status {p.returncode}\n{p.stderr[-2000:]}")
            out[name + "_seconds"] = round(time.perf_counter() - t0, 3)
            out[name + "_info"] = [l for l in p.stderr.splitlines() if "--otus:" in l or "--fastidious:" in l]
            out[name + "_otus_written"] = (d / name / "raxtax.otus").read_text().count(">")
    return out


def host_leg(n_rows):
    rng = np.random.default_rng(n_rows)
    table = make_table(make_rows(n_rows, rng))
    before = rx.otu_cluster(table)
    heavy_rows = int((before.sizes[before.otu] >= 3).sum())
    need = heavy_rows * 9 * L * (L + 64)        # (a string, its map node and its rank)
    line = dict(rows=int(before.n_rows), heavy_rows=heavy_rows, map_bytes_estimate=need)
    if need > args.host_bytes:
        line["host_wall_seconds"] = None
        line["host_note"] = f"not run: the map of rtx_otu_graft_host would hold about {heavy_rows * 9 * L} strings of {L} bytes, {need >> 30} GiB"
        return line
    t0 = time.perf_counter()
    h = rx.otu_graft_host(before)
    line["host_wall_seconds"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    g = rx.otu_graft(before)
    line["device_wall_seconds"] = round(time.perf_counter() - t0, 5)
    assert np.array_equal(h.otu, g.otu) and np.array_equal(h.parent, g.parent) and np.array_equal(h.grafts, g.grafts)
    line["host_over_device"] = round(line["host_wall_seconds"] / line["device_wall_seconds"], 1)
    return line


summary = dict(workload=dict(centres=args.centres, length=L, repeats=args.repeats, columns=1), tables=[], host=[])
for n_rows in [int(x) for x in args.rows.split(",") if x]:
    line = measure(n_rows)
    summary["tables"].append(line)
    print(json.dumps(line), flush=True)
    if args.out:   # (what is measured so far is kept: a later table may take long)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
for n_rows in ([args.host_rows, 1000] if args.host_rows else []):
    line = host_leg(n_rows)
    summary["host"].append(line)
    print(json.dumps(line), flush=True)
if args.cli:
    summary["cli"] = cli_leg(int(args.rows.split(",")[0]), args.cli)
    print(json.dumps(summary["cli"]), flush=True)
if args.out:
    Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")

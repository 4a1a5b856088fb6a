#!/usr/bin/env python3
"""What the sample demultiplexing (rtx_demux.hip) and the per-sample counters beside the taxon profile cost on the device.
    stage    --reads reads of COI length (tag + spacer + 658 random bases + spacer + tag, one substitution in every fourth tag) through
             rx.Demux.run, for lists of 96 + 96 and of 1024 + 1024 tags of 12 bases, at max_offset 0 and 8 (max_mismatches 1): the kernel from
             HIP events (rtx_demux_kernel_time) and the whole call (staging of the ends on the host, copies, kernel, copy back) -- the busy
             time of the stage in rtx_raxtax -- one warm-up call, then the median of --timed calls.
    primers  rx.Trim.run with the LCO1490 / HCO2198 pair (10 % errors) on the same reads, beside them.
    profile  the time of a classify() step of --queries reads against --refs references with a plain profile open and with a profile of
             96 samples open and the samples staged (rtx_batch_prefetch_samples), interleaved; and the profile kernels' own time
             (rtx_index_profile_time, stage timing on).
    python tools/demux_probe.py [--reads N] [--refs N --queries N] [--out profiles/demux_probe.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(HERE))

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--refs", type=int, default=100_000)
ap.add_argument("--queries", type=int, default=131072)
ap.add_argument("--timed", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import raxtax_amd as rx  # noqa: E402
from raxtax_amd import synth  # noqa: E402

FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"
M, L = 12, 658


def pooled(rng, n, f, r, spacer):
    """[n, spacer + M + L + M + spacer] reads: read i carries the tags of pair i mod len(f); every fourth read one substitution in its 5' tag"""
    k = np.arange(n) % len(f)
    t5, t3 = f[k].copy(), r[k].copy()
    hit = np.arange(0, n, 4)
    t5[hit, rng.integers(0, M, len(hit))] = 0x20
    sp = lambda: (1 << rng.integers(0, 4, (n, spacer))).astype(np.uint8)
    return np.ascontiguousarray(np.hstack([sp(), t5, (1 << rng.integers(0, 4, (n, L))).astype(np.uint8), t3, sp()]))


def timed(call):
    ts = []
    for _ in range(1 + args.timed):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
    return res, float(np.median(ts[1:])), ts


out = dict(reads=args.reads, tag_bases=M, max_mismatches=1)
rng = np.random.default_rng(11)
n = args.reads
for per_end in (96, 1024):
    f, r = ((1 << rng.integers(0, 4, (per_end, M))).astype(np.uint8) for _ in range(2))
    tags = [(c, 0) for c in f] + [(c, 1) for c in r]
    pairs = [(i, per_end + i, i % 96) for i in range(per_end)]
    for max_offset in (0, 8):
        reads = pooled(rng, n, f, r, max_offset // 2)
        W = reads.shape[1]
        bases, off = reads.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(W)
        stage = rx.Demux(0, tags, pairs, rx.DemuxParams(1, max_offset))
        ks = []
        (sample, lo, hi, hit, info), dt, ts = timed(lambda: (lambda res: (ks.append(stage.kernel_ms()), res)[1])(stage.run(bases, off)))
        line = dict(read_bases=W, call_seconds=round(dt, 4), calls=[round(x, 4) for x in ts], reads_per_s=round(n / dt), kernel_ms=[round(x, 3) for x in ks],
                    kernel_ms_median=round(float(np.median(ks[1:])), 3), assigned=int((sample != rx.DEMUX_NONE).sum()),
                    placements_per_read=2 * per_end * (max_offset + 1))
        del stage
        if per_end == 96:   # the primer stage on the same reads, beside it
            trim = rx.Trim(0, rx.primer_patterns((FWD, REV)))
            tk = []
            _, tdt, tts = timed(lambda: (lambda res: (tk.append(trim.kernel_ms()), res)[1])(trim.run(bases, off)))
            line["primer_stage"] = dict(call_seconds=round(tdt, 4), calls=[round(x, 4) for x in tts], kernel_ms=[round(x, 3) for x in tk])
            del trim
        out[f"tags_{per_end}+{per_end}_offset_{max_offset}"] = line
        print(json.dumps({f"tags_{per_end}+{per_end}_offset_{max_offset}": line}), flush=True)

# the per-sample counters beside the profile: a classify() step with a plain profile and with 96 samples, interleaved
db = synth.make_db(args.refs)
qs = synth.make_queries(db, args.queries)
tree = rx.Tree.new_flat(db.lineages, db.seq_bytes, db.seq_off, kmer_map=False)
samples = (np.arange(args.queries) % 96).astype(np.uint32)
legs = {}
for name, ns in (("plain_profile", None), ("profile_96_samples", 96)):
    index = rx.Index(tree, stage_timing=True)
    index.profile_begin(0.8, n_samples=ns)
    legs[name] = (index, ns, [])
for k in range(1 + args.timed):
    for name, (index, ns, ts) in legs.items():
        t0 = time.perf_counter()
        if ns:
            index.prefetch_samples(samples)
        index.classify(qs.bases, qs.base_off)
        ts.append(time.perf_counter() - t0)
steps = {}
for name, (index, ns, ts) in legs.items():
    ms, launches = index.profile_time()
    steps[name] = dict(step_seconds=round(float(np.median(ts[1:])), 4), steps=[round(x, 4) for x in ts], profile_kernels_ms_per_step=round(ms / max(launches, 1), 4),
                       counted=int(index.profile_read().totals[0]))
    if ns:
        steps[name]["counted_in_samples"] = int(index.profile_read_samples().totals[:, 0].sum())
    index.profile_end()
out["profile_step"] = dict(refs=args.refs, queries=args.queries, **steps)
print(json.dumps(out, indent=1))
if args.out:
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")

"""raxtax-hip on paired FASTQ input (cli_main.cpp: --reverse; rtx_merge_queries on the reader's thread).  Mates cut from amplicons of the
golden database with planted errors: `-i R1 --reverse R2 --maxee 1` writes the raxtax.out and raxtax.qc of `-i merged.fastq --maxee 1`, where
merged.fastq holds what the plain-Python restatement (tests/merge_common.py) makes of every pair; raxtax.merge is the restatement's report;
the same in several blocks and with R2 gzipped; and what ends a run."""
import gzip
import random
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from merge_common import DEFAULT, VERDICT_NAMES, P, merge_ref, other_base, revcomp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
LETTER = {v: k for k, v in rx.api.IUPAC.items()}


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stderr
    return p


def fastq(records):
    return "".join(f"@{l}\n{''.join(LETTER[int(c)] for c in s)}\n+\n{bytes(q).decode()}\n" for l, s, q in records)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """200 pairs: amplicons of 150 .. 206 bases from the golden references (which have no more), mates of 97 .. 120 bases, Q falling along each
    mate, a few errors planted where Q is low; every ninth pair with mates too short to meet, every thirteenth with 14 errors."""
    d = tmp_path_factory.mktemp("paired")
    rng = random.Random(77)
    refs = [s for _, s in rx.parse_query_fasta_str(DB.read_text()) if set(s.tolist()) <= {1, 2, 4, 8}][:200]
    assert len(refs) == 200
    r1, r2, merged, report = [], [], [], []
    for i, ref in enumerate(refs):
        alen = len(ref) if i % 9 == 4 else rng.randint(150, len(ref))
        at = rng.randint(0, len(ref) - alen)
        amp = ref[at:at + alen]
        nf, nr = (rng.choice((90, 100)), rng.choice((85, 100))) if i % 9 == 4 else (rng.choice((120, 120, 110, 101)), rng.choice((120, 120, 97)))
        fb, rp = amp[:nf].copy(), amp[alen - nr:].copy()
        qf = np.clip(40 - (np.arange(nf) * 25) // nf - np.array([rng.randint(0, 3) for _ in range(nf)]), 2, 41)
        qr = np.clip(40 - (np.arange(nr) * 25) // nr - np.array([rng.randint(0, 3) for _ in range(nr)]), 2, 41)
        n_err = 14 if i % 13 == 6 else rng.choice((0, 0, 1, 2, 3))
        for _ in range(n_err):                                   # in the last third of a mate, where its Q is low
            if rng.random() < 0.5:
                k = rng.randint(2 * nf // 3, nf - 1)
                fb[k] = other_base(rng, fb[k])
            else:
                k = rng.randint(0, nr // 3)
                rp[k] = other_base(rng, rp[k])
        rb = revcomp(rp)
        fq, rq = (33 + qf).astype(np.uint8), (33 + qr[::-1].copy()).astype(np.uint8)
        if i == 3:
            fq[0] = rq[0] = ord("@")                             # quality lines that start like a header
        lf, lr = (f"p{i:03d}/1", f"p{i:03d}/2") if i == 5 else (f"p{i:03d} 1:N:0:7", f"p{i:03d} 2:N:0:7")
        ov, dd, v, mb, mq = merge_ref(DEFAULT, fb, fq, rb, rq)
        r1.append((lf, fb, fq))
        r2.append((lr, rb, rq))
        merged.append((lf, mb, mq))
        report.append("\t".join(map(str, (lf, nf, nr, ov, dd, len(mb), VERDICT_NAMES[v]))))
    (d / "R1.fastq").write_text(fastq(r1))
    (d / "R2.fastq").write_text(fastq(r2))
    with gzip.open(d / "R2.fastq.gz", "wt") as f:
        f.write(fastq(r2))
    (d / "merged.fastq").write_text(fastq(merged))
    (d / "R2_short.fastq").write_text(fastq(r2[:-1]))
    (d / "R2_label.fastq").write_text(fastq(r2[:120] + [("p12x 2:N:0:7",) + r2[120][1:]] + r2[121:]))
    (d / "R1.fasta").write_text("".join(f">{l}\n{''.join(LETTER[int(c)] for c in s)}\n" for l, s, _ in r1))
    return d, report, merged


@pytest.fixture(scope="module")
def single(tmp_path_factory, files):
    d, _, _ = files
    out = tmp_path_factory.mktemp("single") / "out"
    run("-d", DB, "-i", d / "merged.fastq", "-o", out, "--skip-db", "--batch", 128, "--maxee", 1)
    return out


def test_the_fixture_holds_what_it_should(files):
    _, report, merged = files
    verdicts = [r.split("\t")[6] for r in report]
    assert 120 <= verdicts.count("merged") <= 185 and verdicts.count("no_overlap") >= 20
    assert any(r.split("\t")[4] not in ("0",) for r in report if r.endswith("merged")) and any(len(m[1]) == 0 for m in merged)


@pytest.mark.parametrize("variant", ["one_block", "several_blocks", "gzipped"])
def test_paired_input_equals_the_run_on_the_merged_reads(tmp_path, files, single, variant):
    d, report, _ = files
    out = tmp_path / "paired"
    extra = {"one_block": (), "several_blocks": ("--block-bytes", 12000), "gzipped": ("--block-bytes", 17000)}[variant]
    p = run("-d", DB, "-i", d / "R1.fastq", "--reverse" if variant != "gzipped" else "-r", d / ("R2.fastq.gz" if variant == "gzipped" else "R2.fastq"), "-o", out, "--skip-db",
            "--batch", 128, "--maxee", 1, *extra)
    for f in ("raxtax.out", "raxtax.qc", "raxtax.ckp"):
        assert (out / f).read_bytes() == (single / f).read_bytes(), f
    assert (out / "raxtax.out").stat().st_size > 10_000 and not (single / "raxtax.merge").exists()
    lines = (out / "raxtax.merge").read_text().splitlines()
    assert lines[0] == "label\tforward_length\treverse_length\toverlap\tdiffs\tmerged_length\tverdict"
    assert lines[1:] == report
    m = re.search(r"\[INFO \] --reverse: (\d+) pairs, (\d+) merged; not merged for bad_quality (\d+), too_long (\d+), too_short (\d+), no_overlap (\d+)", p.stderr)
    assert m, p.stderr
    verdicts = [r.split("\t")[6] for r in report]
    assert [int(x) for x in m.groups()] == [200, verdicts.count("merged"), 0, 0, 0, verdicts.count("no_overlap")]
    assert '"merge"' in (out / "raxtax.json").read_text() and '"merge"' not in (single / "raxtax.json").read_text()


def test_merge_options_reach_the_stage(tmp_path, files):
    d, report, _ = files
    out = tmp_path / "strict"
    run("-d", DB, "-i", d / "R1.fastq", "--reverse", d / "R2.fastq", "-o", out, "--skip-db", "--batch", 128, "--merge-maxdiffs", 0, "--merge-minovlen", 40, "--merge-qcap", 30,
        "--merge-maxdiffpct", 50)
    r1, r2 = rx.parse_query_fastq_str((d / "R1.fastq").read_text()), rx.parse_query_fastq_str((d / "R2.fastq").read_text())
    p = P(min_overlap=40, max_diffs=0, max_diff_pct=50, q_cap=30)
    want = []
    for (lf, fb, fq), (_, rb, rq) in zip(r1, r2):
        ov, dd, v, mb, _ = merge_ref(p, fb, fq, rb, rq)
        want.append("\t".join(map(str, (lf, len(fb), len(rb), ov, dd, len(mb), VERDICT_NAMES[v]))))
    assert (out / "raxtax.merge").read_text().splitlines()[1:] == want and want != report


def test_what_ends_a_run(tmp_path, files):
    d, _, _ = files
    out = tmp_path / "out"
    p = run("-d", DB, "-i", d / "R1.fastq", "--reverse", d / "R2_short.fastq", "-o", out, "--skip-db", ok=False)                      # R2 one record short
    assert p.returncode == 66 and "R2_short.fastq ends after record 199" in p.stderr, p.stderr
    p = run("-d", DB, "-i", d / "R1.fastq", "--reverse", d / "R2_short.fastq", "-o", tmp_path / "out2", "--skip-db", "--block-bytes", 12000, ok=False)
    assert p.returncode == 66 and "R2_short.fastq ends after record 199" in p.stderr, p.stderr
    p = run("-d", DB, "-i", d / "R1.fastq", "--reverse", d / "R2_label.fastq", "-o", tmp_path / "out3", "--skip-db", ok=False)          # a label that does not pair
    assert p.returncode == 66 and "pair 121" in p.stderr and "p12x" in p.stderr, p.stderr
    p = run("-d", DB, "-i", d / "R1.fasta", "--reverse", d / "R2.fastq", "-o", tmp_path / "out4", ok=False)                             # --reverse with FASTA input
    assert p.returncode == 64 and "FASTQ" in p.stderr and not (tmp_path / "out4").exists()
    for bad in (("--merge-minovlen", 20), ("--merge-maxdiffs", 3), ("--merge-maxdiffpct", 10), ("--merge-qcap", 40)):                   # a merge option without --reverse
        p = run("-d", DB, "-i", d / "R1.fastq", "-o", tmp_path / "out5", *bad, ok=False)
        assert p.returncode == 64 and bad[0] in p.stderr and "--reverse" in p.stderr and not (tmp_path / "out5").exists(), bad
    for bad in (("--merge-minovlen", 0), ("--merge-maxdiffpct", 101), ("--merge-qcap", 94), ("--merge-maxdiffs", "x"), ("--merge-maxdiffs", -1)):   # a bad value
        p = run("-d", DB, "-i", d / "R1.fastq", "--reverse", d / "R2.fastq", "-o", tmp_path / "out6", *bad, ok=False)
        assert p.returncode == 64 and bad[0] in p.stderr and not (tmp_path / "out6").exists(), bad

"""raxtax-hip on FASTQ input with the quality filter (cli_main.cpp: --maxee, --truncq ...; rtx_index_set_quality on every handle).  On a
`.fastq.gz` the `.out` and `.tsv` files are byte for byte those of a run on the FASTA of the reads cut -- and left out -- as the plain-integer
restatement (tests/qual_common.py) says, raxtax.qc has one line per query, FASTQ without a filter option is the FASTA run, and the settings
are part of the checkpoint."""
import gzip
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from qual_common import ee_text, qual_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"
LETTER = {v: k for k, v in rx.api.IUPAC.items()}
PARAMS = rx.QualParams(trunc_qual=2, max_ee=1.5, min_len=100, max_ns=2)
OPTIONS = ("--truncq", 2, "--maxee", 1.5, "--minlen", 100, "--maxns", 2)


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stderr
    return p


def text(codes):
    return "".join(LETTER[int(c)] for c in codes)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """300 reads of the golden queries with quality strings: Q falls along the read, most have a base of Q <= 2 in their second half, every
    seventh is bad all along, some hold N bases.  reads.fastq.gz, the same reads as FASTA, and the FASTA of what the filter leaves."""
    d = tmp_path_factory.mktemp("fastq")
    rng = np.random.default_rng(61)
    reads = []
    for i, (label, seq) in enumerate(rx.parse_query_fasta_str(QUERIES.read_text())[:300]):
        n = len(seq)
        seq = seq.copy()
        q = np.clip(40 - (np.arange(n) * 10) // n - rng.integers(0, 4, n), 3, 41)
        if i % 7 == 3:
            q = rng.integers(3, 10, n)
        elif i % 3:
            q[int(rng.integers(n // 2, n))] = int(rng.integers(0, 3))
        if i % 19 == 2:
            seq[rng.integers(0, n // 3, 5)] = 15
        quals = (33 + q).astype(np.uint8)
        if i == 10:
            quals[0] = ord("@")                                     # a quality line that starts like a header
        reads.append((f"q{i:03d};{label.split()[0]}", seq, quals))
    rows = [qual_ref(PARAMS, s, q) for _, s, q in reads]
    with gzip.open(d / "reads.fastq.gz", "wt") as f:
        f.write("".join(f"@{l}\n{text(s)}\n+\n{q.tobytes().decode()}\n" for l, s, q in reads))
    (d / "reads.fasta").write_text("".join(f">{l}\n{text(s)}\n" for l, s, _ in reads))
    (d / "kept.fasta").write_text("".join(f">{l}\n{text(s[:h])}\n" for (l, s, _), (h, _, v) in zip(reads, rows) if v == 0))
    return d, reads, rows


def test_the_files_are_those_of_a_run_on_the_filtered_reads(tmp_path, files):
    d, reads, rows = files
    n_pass = sum(1 for r in rows if r[2] == 0)
    n_trunc = sum(1 for (_, s, _), r in zip(reads, rows) if r[2] == 0 and r[0] < len(s))
    assert 150 < n_pass < 280 and n_trunc > 100
    a, b = tmp_path / "filtered", tmp_path / "plain"
    pa = run("-d", DB, "-i", d / "reads.fastq.gz", "-o", a, "--skip-db", "--batch", 128, "--tsv", "--block-bytes", 60000, *OPTIONS)   # (several blocks)
    run("-d", DB, "-i", d / "kept.fasta", "-o", b, "--skip-db", "--batch", 128, "--tsv")
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert (a / "raxtax.out").stat().st_size > 10_000 and not (b / "raxtax.qc").exists()
    lines = (a / "raxtax.qc").read_text().splitlines()
    assert lines[0] == "label\tlength\tstart\tend\texpected_errors\tverdict"
    want = ["\t".join((l, str(len(s)), "0", str(h), ee_text(e), "+".join(rx.qual_verdict_names(v)) or "pass")) for (l, s, _), (h, e, v) in zip(reads, rows)]
    assert lines[1:] == want
    assert any("+" in w.split("\t")[5] for w in want) and any(w.endswith("\tpass") for w in want)
    m = re.search(r"\[INFO \] quality filter: (\d+) queries, (\d+) passed \((\d+) of them cut short\); discarded for bad_quality (\d+), short_for_trunc_len (\d+), "
                  r"too_short (\d+), too_long (\d+), too_many_n (\d+), max_ee (\d+), max_ee_rate (\d+)", pa.stderr)
    assert m, pa.stderr
    reasons = [sum((r[2] >> k) & 1 for r in rows) for k in range(7)]
    assert [int(x) for x in m.groups()] == [300, n_pass, n_trunc] + reasons
    # the settings are part of the checkpoint: the same command resumes, another setting starts over
    assert "quality" in (a / "raxtax.json").read_text() and "quality" not in (b / "raxtax.json").read_text()
    again = run("-d", DB, "-i", d / "reads.fastq.gz", "-o", a, "--skip-db", "--batch", 128, "--tsv", *OPTIONS)
    assert "Restarting from checkpoint" in again.stderr
    other = run("-d", DB, "-i", d / "reads.fastq.gz", "-o", a, "--skip-db", "--batch", 128, "--tsv", "--truncq", 30, "--maxee", 1.5, "--minlen", 100, "--maxns", 2)
    assert "Restarting from checkpoint" not in other.stderr
    assert (a / "raxtax.qc").read_text().splitlines() != lines and len((a / "raxtax.qc").read_text().splitlines()) == 301


def test_fastq_without_options_equals_the_fasta_run(tmp_path, files):
    d, reads, _ = files
    a, b = tmp_path / "fastq", tmp_path / "fasta"
    run("-d", DB, "-i", d / "reads.fastq.gz", "-o", a, "--skip-db", "--batch", 128, "--tsv", "--block-bytes", 70000)
    run("-d", DB, "-i", d / "reads.fasta", "-o", b, "--skip-db", "--batch", 128, "--tsv")
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.ckp", "raxtax.json"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert not (a / "raxtax.qc").exists()


def test_resume_after_a_partial_run(tmp_path, files):
    d, reads, rows = files
    full = tmp_path / "full"
    run("-d", DB, "-i", d / "reads.fastq.gz", "-o", full, "--skip-db", "--batch", 128, *OPTIONS)
    want = {f: (full / f).read_text().splitlines() for f in ("raxtax.out", "raxtax.qc", "raxtax.ckp")}
    part = tmp_path / "part"
    shutil.copytree(full, part)
    done = set(want["raxtax.ckp"][:120])
    (part / "raxtax.ckp").write_text("\n".join(want["raxtax.ckp"][:120]) + "\n")
    for f in ("raxtax.out", "raxtax.qc"):
        head = want[f][:1] if f == "raxtax.qc" else []
        keep = [l for l in want[f][len(head):] if l.split("\t")[0] in done]
        nxt = next(l for l in want[f][len(head):] if l.split("\t")[0] not in done)
        (part / f).write_text("\n".join(head + keep) + "\n" + nxt[: nxt.index("\t") + 2])   # cut in the middle of a line of an unfinished query
    p = run("-d", DB, "-i", d / "reads.fastq.gz", "-o", part, "--skip-db", "--batch", 128, *OPTIONS)
    assert "Restarting from checkpoint" in p.stderr
    for f, lines in want.items():
        got = (part / f).read_text().splitlines()
        if f == "raxtax.qc":
            assert got[0] == lines[0]
        assert sorted(got) == sorted(lines), f


def test_a_filter_option_on_fasta_input_and_bad_values_end_the_run(tmp_path, files):
    d, _, _ = files
    p = run("-d", DB, "-i", d / "reads.fasta", "-o", tmp_path / "out", "--maxee", 1, ok=False)
    assert p.returncode == 64 and "FASTQ" in p.stderr and not (tmp_path / "out").exists()
    for bad in (("--maxee", "-1"), ("--maxee", "x"), ("--truncq", 94), ("--trunclen", 0), ("--fastq-ascii", 50), ("--maxns", -1), ("--maxee-rate", "nan")):
        p = run("-d", DB, "-i", d / "reads.fastq.gz", "-o", tmp_path / "out", *bad, ok=False)
        assert p.returncode == 64 and bad[0] in p.stderr and not (tmp_path / "out").exists(), bad

"""raxtax-hip with a contaminant screen (cli_main.cpp: --contaminants FILE, --contam-minhits, --contam-minpct; rtx_index_set_screen on every
handle).  On FASTA and on FASTQ input the `.out` file is byte for byte that of a run on the passing reads alone, raxtax.screen has one line
per read, line for line what the plain-Python restatement (tests/screen_common.py) says, and the setting with the set's fingerprint is
part of the checkpoint: the same command resumes, another contaminant file starts over."""
import gzip
import random
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from screen_common import NONE, make_set, random_codes, revcomp, screen_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"
LETTER = {v: k for k, v in rx.api.IUPAC.items()}
DEFAULT = rx.ScreenParams()


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stderr
    return p


def text(codes):
    return "".join(LETTER[int(c)] for c in codes)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """300 reads: golden queries, every fifth one a read cut from one of two contaminant records (a 5 386-base "phage" and a 900-base
    "vector", either orientation), one query that carries 30 phage bases (hits, no contaminant).  The reads as FASTA and as FASTQ, the
    contaminants as FASTA (gzip-compressed), a second contaminant file, and the FASTA of the passing reads."""
    d = tmp_path_factory.mktemp("screen")
    rng = random.Random(71)
    contam = [("phage genome of 5386 bases", random_codes(random.Random(5386), 5386)), ("vector", random_codes(rng, 900))]
    sset = make_set([c for _, c in contam])
    reads = []
    for i, (label, seq) in enumerate(rx.parse_query_fasta_str(QUERIES.read_text())[:300]):
        seq = seq.copy()
        if i % 5 == 2:
            src = contam[(i // 5) % 2][1]
            n = rng.randint(150, 300)
            at = rng.randrange(0, len(src) - n)
            seq = src[at:at + n].copy()
            if i % 10 == 2:
                seq = revcomp(seq)
        if i == 33:
            seq[40:70] = contam[0][1][1000:1030]
        reads.append((f"q{i:03d};{label.split()[0]}", seq))
    rows = [screen_ref(sset, DEFAULT, s) for _, s in reads]
    with gzip.open(d / "contaminants.fasta.gz", "wt") as f:
        f.write("".join(f">{l}\n{text(c)}\n" for l, c in contam))
    (d / "other.fasta").write_text(f">phage\n{text(contam[0][1])}\n")
    (d / "reads.fasta").write_text("".join(f">{l}\n{text(s)}\n" for l, s in reads))
    (d / "reads.fastq").write_text("".join(f"@{l}\n{text(s)}\n+\n{'I' * len(s)}\n" for l, s in reads))
    (d / "kept.fasta").write_text("".join(f">{l}\n{text(s)}\n" for (l, s), r in zip(reads, rows) if r[4] == 0))
    return d, reads, rows


def screen_lines(reads, rows, names=("phage", "vector")):
    return ["\t".join((l, str(len(s)), str(w), str(h), "-" if f == NONE else str(f), "-" if src == NONE else names[src], "contaminant" if v else "pass"))
            for (l, s), (w, h, f, src, v) in zip(reads, rows)]


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_the_files_are_those_of_a_run_on_the_passing_reads(tmp_path, files, kind):
    d, reads, rows = files
    n_contam = sum(r[4] for r in rows)
    assert n_contam == 60 and rows[33][1] >= 15 and rows[33][4] == 0 and {r[3] for r in rows} == {0, 1, NONE}
    a, b = tmp_path / "screened", tmp_path / "plain"
    pa = run("-d", DB, "-i", d / f"reads.{kind}", "-o", a, "--skip-db", "--batch", 128, "--block-bytes", 60000, "--contaminants", d / "contaminants.fasta.gz")   # (several blocks)
    run("-d", DB, "-i", d / "kept.fasta", "-o", b, "--skip-db", "--batch", 128)
    for f in ("raxtax.out", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert (a / "raxtax.out").stat().st_size > 10_000 and not (b / "raxtax.screen").exists() and not (a / "raxtax.qc").exists()
    lines = (a / "raxtax.screen").read_text().splitlines()
    assert lines[0] == "label\tlength\twindows\thits\tfirst\tsource\tverdict"
    assert lines[1:] == screen_lines(reads, rows)
    m = re.search(r"\[INFO \] --contaminants: (\d+) queries, (\d+) screened, (\d+) contaminants", pa.stderr)
    assert m and [int(x) for x in m.groups()] == [300, 300, n_contam], pa.stderr
    assert "contaminants" in (a / "raxtax.json").read_text() and "contaminants" not in (b / "raxtax.json").read_text()


def test_thresholds_on_the_command_line(tmp_path, files):
    d, reads, rows = files
    sset = make_set([random_codes(random.Random(5386), 5386)])
    p = rx.ScreenParams(min_hits=1, min_pct=2)
    want = [screen_ref(sset, p, s) for _, s in reads]
    assert want[33][4] == 1 and sum(r[4] for r in want) == 31          # the read with the short stretch now counts; the vector is not in this file
    run("-d", DB, "-i", d / "reads.fasta", "-o", tmp_path / "o", "--skip-db", "--contaminants", d / "other.fasta", "--contam-minhits", 1, "--contam-minpct", 2)
    assert (tmp_path / "o" / "raxtax.screen").read_text().splitlines()[1:] == screen_lines(reads, want)
    for bad in (("--contam-minhits", 0), ("--contam-minpct", 101), ("--contam-minpct", "x")):
        q = run("-d", DB, "-i", d / "reads.fasta", "-o", tmp_path / "bad", "--contaminants", d / "other.fasta", *bad, ok=False)
        assert q.returncode == 64 and bad[0] in q.stderr and not (tmp_path / "bad").exists(), bad
    q = run("-d", DB, "-i", d / "reads.fasta", "-o", tmp_path / "bad", "--contam-minhits", 3, ok=False)
    assert q.returncode == 64 and "--contaminants" in q.stderr
    (tmp_path / "short.fasta").write_text(">s\nACGTACGTACGT\n")
    q = run("-d", DB, "-i", d / "reads.fasta", "-o", tmp_path / "bad", "--contaminants", tmp_path / "short.fasta", ok=False)
    assert q.returncode == 64 and "no valid window" in q.stderr and not (tmp_path / "bad").exists()


def test_resume_after_a_partial_run_and_another_file_starts_over(tmp_path, files):
    d, reads, rows = files
    full = tmp_path / "full"
    args = ("-d", DB, "-i", d / "reads.fasta", "--skip-db", "--batch", 128)
    run(*args, "-o", full, "--contaminants", d / "contaminants.fasta.gz")
    want = {f: (full / f).read_text().splitlines() for f in ("raxtax.out", "raxtax.screen", "raxtax.ckp")}
    part = tmp_path / "part"
    shutil.copytree(full, part)
    done = set(want["raxtax.ckp"][:100])
    (part / "raxtax.ckp").write_text("\n".join(want["raxtax.ckp"][:100]) + "\n")
    for f in ("raxtax.out", "raxtax.screen"):
        head = want[f][:1] if f == "raxtax.screen" else []
        keep = [l for l in want[f][len(head):] if l.split("\t")[0] in done]
        nxt = next(l for l in want[f][len(head):] if l.split("\t")[0] not in done)
        (part / f).write_text("\n".join(head + keep) + "\n" + nxt[: nxt.index("\t") + 2])   # cut in the middle of a line of an unfinished query
    p = run(*args, "-o", part, "--contaminants", d / "contaminants.fasta.gz")
    assert "Restarting from checkpoint" in p.stderr
    for f, lines in want.items():
        got = (part / f).read_text().splitlines()
        if f == "raxtax.screen":
            assert got[0] == lines[0]
        assert sorted(got) == sorted(lines), f
    # another contaminant file: no resuming, the run starts over and writes every line again
    other = run(*args, "-o", part, "--contaminants", d / "other.fasta")
    assert "Restarting from checkpoint" not in other.stderr
    got = (part / "raxtax.screen").read_text().splitlines()
    assert len(got) == 301 and got != want["raxtax.screen"] and sum(l.endswith("\tcontaminant") for l in got) == 30
    # ... and so does a run without the option, which leaves no screen file behind
    plain = run(*args, "-o", part)
    assert "Restarting from checkpoint" not in plain.stderr and not (part / "raxtax.screen").exists()

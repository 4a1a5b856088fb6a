"""raxtax-hip --primers (cli_main.cpp): rtx_index_set_primers on every handle.  On a FASTA of primer-carrying reads the `.out` and `.tsv` files
are byte for byte those of a run without the option on the FASTA of the reads cut at the positions of the numpy recurrence
(tests/trim_common.py), raxtax.trim has one line per query, and the run says how many primers it found."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from trim_common import trim_many

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"
FWD, REV = "GGTCAACAAATCATAAAGAYATYGG", "TAAACTTCAGGGTGACCAAARAAYCA"
LETTER = {v: k for k, v in rx.api.IUPAC.items()}


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stderr
    return p


def text(codes):
    return "".join(LETTER[int(c)] for c in codes)


def fasta(path, queries):
    path.write_text("".join(f">{label}\n{text(seq)}\n" for label, seq in queries))


@pytest.mark.parametrize("strand", ["plus", "both"])
def test_the_files_are_those_of_a_run_on_the_trimmed_reads(tmp_path, strand):
    both = strand == "both"
    amplicons = rx.parse_query_fasta_str(QUERIES.read_text())[:300]
    rng = np.random.default_rng(51)
    inst = lambda t: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(t)], np.uint8)
    queries = []
    for i, (label, amp) in enumerate(amplicons):
        f, r = inst(FWD), rx.api.revcomp(inst(REV))
        if i % 4 == 1:
            f = np.delete(f, int(rng.integers(0, len(f))))                    # one primer error
        if i % 4 == 2:
            r = np.insert(r, int(rng.integers(0, len(r))), 2)
        read = amp if (128 <= i < 256 or i % 9 == 0) else np.concatenate([f, amp] if i % 11 == 0 else [f, amp, r])   # (a whole chunk of 128 without primers)
        if both and i % 2:
            read = rx.api.revcomp(read)
        queries.append((f"q{i:03d};{label.split()[0]}", read.astype(np.uint8)))
    pats = rx.primer_patterns((FWD, REV), both_strands=both)                  # 10 %: two errors each
    assert [p.max_errors for p in pats] == [2, 2] * (2 if both else 1)
    lo, hi, hit = trim_many(pats, [r for _, r in queries])
    assert (hi > lo).all()
    raw, cut = tmp_path / "raw.fasta", tmp_path / "cut.fasta"
    fasta(raw, queries)
    fasta(cut, [(l, r[int(a):int(b)]) for (l, r), a, b in zip(queries, lo, hi)])
    a, b = tmp_path / "primers", tmp_path / "plain"
    pa = run("-d", DB, "-i", raw, "-o", a, "--skip-db", "--batch", 128, "--tsv", "--strand", strand, "--primers", f"{FWD}:{REV}")
    run("-d", DB, "-i", cut, "-o", b, "--skip-db", "--batch", 128, "--tsv", "--strand", strand)
    for f in ("raxtax.out", "raxtax.tsv") + (("raxtax.strand",) if both else ()):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert (a / "raxtax.out").stat().st_size > 10_000 and not (b / "raxtax.trim").exists()
    lines = (a / "raxtax.trim").read_text().splitlines()
    assert lines[0] == "label\tlength\tstart\tend\tprimer5\terrors5\tprimer3\terrors3"
    col = lambda p, e: ("-", "-") if p == 0xFF else (str(p), str(e))
    want = ["\t".join((l, str(len(r)), str(int(x)), str(int(y)), *col(int(h) & 0xFF, int(h) >> 8 & 0xFF), *col(int(h) >> 16 & 0xFF, int(h) >> 24)))
            for (l, r), x, y, h in zip(queries, lo, hi, hit)]
    assert lines[1:] == want
    n5, n3 = int(((hit & 0xFF) != 0xFF).sum()), int((((hit >> 16) & 0xFF) != 0xFF).sum())
    assert 100 < n5 < 300 and 100 < n3 < 300
    m = re.search(r"\[INFO \] --primers: (\d+) queries, (\d+) with a 5' primer, (\d+) with a 3' primer, (\d+) left empty", pa.stderr)
    assert m, pa.stderr
    assert tuple(int(x) for x in m.groups()) == (300, n5, n3, 0)
    # the option is part of the checkpoint: the same command resumes (nothing left to do), another primer setting refuses the folder's state and starts over
    again = run("-d", DB, "-i", raw, "-o", a, "--skip-db", "--batch", 128, "--tsv", "--strand", strand, "--primers", f"{FWD}:{REV}")
    assert "Restarting from checkpoint" in again.stderr
    assert (a / "raxtax.trim").read_text().splitlines()[0] == lines[0]


def test_a_bad_primer_ends_the_run_before_any_device_work(tmp_path):
    for spec, named in (("ACGTXACGT:ACGT", "ACGTXACGT"), ("ACGT:AC-GT", "AC-GT"), ("A" * 65 + ":", "A" * 65)):
        p = run("-d", DB, "-i", QUERIES, "-o", tmp_path / "out", "--primers", spec, ok=False)
        assert named in p.stderr and "--primers" in p.stderr
        assert not (tmp_path / "out").exists()
    many = [x for k in range(5) for x in ("--primers", "ACGTACGTAC" + "ACGT"[k % 4] + ":TTGACCA")]
    p = run("-d", DB, "-i", QUERIES, "-o", tmp_path / "out", *many, ok=False)           # ten patterns
    assert "at most 8" in p.stderr and "TTGACCA" in p.stderr and not (tmp_path / "out").exists()
    p = run("-d", DB, "-i", QUERIES, "-o", tmp_path / "out", "--primers", "ACGTACGT", ok=False)   # no colon
    assert "FWD:REV" in p.stderr

"""raxtax-hip --derep (cli_main.cpp): RTX_OPT_DEREP on every handle.  On a FASTA with injected duplicates the `.out`, `.tsv` and `.profile`
files are byte for byte those of the run without the option, and the run says how many of its queries were distinct."""
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"


def run(*args):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def test_the_files_are_those_of_a_run_without_the_option(tmp_path):
    records = [r for r in QUERIES.read_text().split(">") if r][:300]
    seqs = []
    for r in records:
        _, _, body = r.partition("\n")
        seqs.append(body.replace("\n", "").upper())
    # 700 queries from 300 reads: record i again as query 300 + i when i is even, and record 7 a hundred times in a row; every label its own
    order = list(range(300)) + list(range(0, 300, 2)) + [7] * 100 + list(range(1, 300, 2))
    assert len(order) == 700
    path = tmp_path / "dups.fasta"
    path.write_text("".join(f">query{k:04d};record={i}\n{seqs[i]}\n" for k, i in enumerate(order)))
    a, b = tmp_path / "derep", tmp_path / "plain"
    pa = run("-d", DB, "-i", path, "-o", a, "--skip-db", "--batch", 128, "--tsv", "--profile", 0.8, "--derep")
    run("-d", DB, "-i", path, "-o", b, "--skip-db", "--batch", 128, "--tsv", "--profile", 0.8)
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.profile"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert (a / "raxtax.out").stat().st_size > 10_000 and (a / "raxtax.profile").read_text().startswith("# cutoff=0.80\tqueries=700\t")
    m = re.search(r"--derep: (\d+) queries, (\d+) distinct", pa.stderr)
    assert m, pa.stderr
    n_distinct = sum(len({seqs[i] for i in order[c:c + 128]}) for c in range(0, 700, 128))   # per chunk of 128
    assert (int(m.group(1)), int(m.group(2))) == (700, n_distinct) and n_distinct < 700

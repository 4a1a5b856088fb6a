"""raxtax-hip --strand both (cli_main.cpp, RTX_OPT_STRAND): a query file with every third record reverse-complemented gives, byte for byte,
the raxtax.out and raxtax.tsv of the file as it was; raxtax.strand says which records were flipped, with the oracle's peak; the file takes
part in resume, and the setting in the checkpoint."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"
_COMPLEMENT = str.maketrans("ACGTRYKMSWBVDHNacgtrykmswbvdhn", "TGCAYRMKSWVBHDNtgcayrmkswvbhdn")


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The first 600 records as they are, and with every third one reverse-complemented (as text: the complement of the letters, reversed)."""
    d = tmp_path_factory.mktemp("strand_queries")
    records = [r for r in QUERIES.read_text().split(">") if r][:600]
    assert len(records) == 600
    plain, mixed = [], []
    for i, r in enumerate(records):
        header, _, body = r.partition("\n")
        seq = body.replace("\n", "")
        plain.append(f">{header}\n{seq}\n")
        mixed.append(f">{header}\n{seq.translate(_COMPLEMENT)[::-1] if i % 3 == 0 else seq}\n")
    (d / "plain.fasta").write_text("".join(plain))
    (d / "mixed.fasta").write_text("".join(mixed))
    return d / "plain.fasta", d / "mixed.fasta"


@pytest.mark.parametrize("skip", [False, True])
def test_flipped_records_give_the_files_of_the_oriented_ones(tmp_path, oracle, files, skip):
    plain, mixed = files
    a, b = tmp_path / "plus", tmp_path / "both"
    extra = ["--skip-exact-matches"] if skip else []
    run("-d", DB, "-i", plain, "-o", a, "--skip-db", "--tsv", "--batch", 128, *extra)
    run("-d", DB, "-i", mixed, "-o", b, "--skip-db", "--tsv", "--batch", 128, "--strand", "both", *extra)
    assert not (a / "raxtax.strand").exists() and "strand" not in (a / "raxtax.json").read_text()
    assert '"strand": "both"' in (b / "raxtax.json").read_text()
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # raxtax.strand: one line per query in the order of raxtax.out, - exactly at the flipped records, the oracle's peak and t
    otree = oracle.parse_reference_fasta_str(DB.read_text())
    queries = oracle.parse_query_fasta_str(plain.read_text())
    assert len(queries) == 600
    lines = [l.split("\t") for l in (b / "raxtax.strand").read_text().splitlines()]
    assert [l[0] for l in lines] == (b / "raxtax.ckp").read_text().splitlines() == [q[0] for q in queries]
    margin = None
    for i, ((label, seq), l) in enumerate(zip(queries, lines)):
        seq = np.asarray(seq, dtype=np.uint8)
        t, counts = otree.hit_counts(seq, skip_exact=skip)
        comp = np.arange(256, dtype=np.uint8)
        comp[:16] = [int(f"{c:04b}"[::-1], 2) for c in range(16)]
        _, counts_rc = otree.hit_counts(comp[seq[::-1]], skip_exact=skip)
        m = int(counts.max()) - int(counts_rc.max())
        margin = m if margin is None else min(margin, m)
        assert l == [label, "-" if i % 3 == 0 else "+", str(int(counts.max())), str(int(t))], (i, l)
    print(f"skip {skip}: smallest margin between the peaks of the two orientations: {margin}")
    assert margin > 0


def test_resume_and_the_setting_in_the_checkpoint(tmp_path, files):
    plain, mixed = files
    full = tmp_path / "full"
    run("-d", DB, "-i", mixed, "-o", full, "--skip-db", "--tsv", "--batch", 128, "--strand", "both")
    want = {f: (full / f).read_text().splitlines() for f in ("raxtax.out", "raxtax.tsv", "raxtax.strand", "raxtax.ckp")}
    assert len(want["raxtax.strand"]) == 600
    # interrupted: 250 queries finished, every output cut in the middle of a line of an unfinished query
    part = tmp_path / "part"
    shutil.copytree(full, part)
    done = set(want["raxtax.ckp"][:250])
    (part / "raxtax.ckp").write_text("\n".join(want["raxtax.ckp"][:250]) + "\n")
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.strand"):
        keep = [l for l in want[f] if l.split("\t")[0] in done]
        nxt = next(l for l in want[f] if l.split("\t")[0] not in done)
        (part / f).write_text("\n".join(keep) + "\n" + nxt[: max(len(nxt) // 2, nxt.index("\t") + 2)])
    p = run("-d", DB, "-i", mixed, "-o", part, "--skip-db", "--tsv", "--batch", 128, "--strand", "both")
    assert "Restarting from checkpoint" in p.stderr
    for f, lines in want.items():
        assert sorted((part / f).read_text().splitlines()) == sorted(lines), f
    # the other setting: the checkpoint does not apply, the run starts over
    p = run("-d", DB, "-i", mixed, "-o", part, "--skip-db", "--tsv", "--batch", 128, "--strand", "plus")
    assert "Restarting from checkpoint" not in p.stderr
    assert (part / "raxtax.ckp").read_text().splitlines() == want["raxtax.ckp"]
    assert "strand" not in (part / "raxtax.json").read_text() and not (part / "raxtax.strand").exists()
    assert (part / "raxtax.out").read_text().splitlines() != want["raxtax.out"]   # the flipped records as they are given: other lines
    p = run("-d", DB, "-i", mixed, "-o", part, "--skip-db", "--tsv", "--batch", 128, "--strand", "both")
    assert "Restarting from checkpoint" not in p.stderr
    for f, lines in want.items():
        assert (part / f).read_text().splitlines() == lines, f
    # --device-format has no effect under both strands: one notice, the same files
    dev = tmp_path / "dev"
    p = run("-d", DB, "-i", mixed, "-o", dev, "--skip-db", "--tsv", "--batch", 128, "--strand", "both", "--device-format")
    assert p.stderr.count("--device-format has no effect") == 1
    for f, lines in want.items():
        assert (dev / f).read_text().splitlines() == lines, f

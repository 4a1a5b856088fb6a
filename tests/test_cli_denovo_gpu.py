"""raxtax-hip --uniques --otus --denovo (cli_main.cpp): PREFIX/raxtax.otus.denovo, raxtax.otus.clean and, with --tags, raxtax.otus.clean.tsv are
byte for byte the rx.denovo_* texts of the table of the reads the run classified (rx.tally_reads, clustered and checked on the host);
raxtax.otus, .map and .tsv are what a run without the option writes; the option is a key of raxtax.json only when it is on."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth
from tally_common import concat

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
COMMON = ("--skip-db", "--batch", 16, "--block-bytes", 6000)
OTU_FILES = ("raxtax.otus", "raxtax.otus.map", "raxtax.otus.tsv")
NEW_FILES = ("raxtax.otus.denovo", "raxtax.otus.clean", "raxtax.otus.clean.tsv")
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A database of 48 references of 160 bases; 12 centres taken from it with 6 .. 9 copies and a single-substitution variant each, and 8
    chimeras of two centres, one or two copies each, between the tags of a sheet of two samples."""
    d = tmp_path_factory.mktemp("denovo")
    db = synth.make_db(48, length=160, fanouts=(2, 2, 2, 1, 1, 1))
    (d / "db.fasta").write_text(db.fasta())
    rng = np.random.default_rng(23)
    letters = "ACGT"
    centres = ["".join("?AC?G???T"[b] for b in db.seq(int(ref))) for ref in rng.choice(db.n, 12, replace=False)]
    reads = []
    for c, centre in enumerate(centres):
        i = int(rng.integers(0, len(centre)))
        reads += [centre] * (6 + c % 4) + [centre[:i] + letters[(letters.index(centre[i]) + 1) % 4] + centre[i + 1:]]
    for c in range(8):
        a, b = (int(x) for x in rng.choice(12, 2, replace=False))
        bp = int(rng.integers(50, 110))
        reads += [centres[a][:bp] + centres[b][bp:]] * (1 + c % 2)
    reads = [reads[int(p)] for p in rng.permutation(len(reads))]
    ftag, rtag = ["ACGTTGCA", "TTGACCAT"], ["CATGGTCA", "AGCTAGGT"]
    (d / "sheet.tsv").write_text("".join(f"s{k}\t{ftag[k]}\t{rtag[k]}\n" for k in range(2)))
    sample = [n % 2 for n in range(len(reads))]
    tagged = [ftag[k] + s + rtag[k].translate(_COMPLEMENT)[::-1] for s, k in zip(reads, sample)]
    (d / "tagged.fasta").write_text("".join(f">read{n:03d}\n{s}\n" for n, s in enumerate(tagged)))
    (d / "plain.fasta").write_text("".join(f">read{n:03d}\n{s}\n" for n, s in enumerate(reads)))
    return dict(db=d / "db.fasta", tagged=d / "tagged.fasta", plain=d / "plain.fasta", sheet=d / "sheet.tsv", reads=reads, sample=sample)


def expected(reads, sample=None, samples=0, **params):
    seqs = [np.array([CODE[c] for c in s], np.uint8) for s in reads]
    table = rx.tally_reads(*concat(seqs), None if sample is None else np.array(sample, np.uint32), samples=samples)
    otus = rx.otu_cluster_host(table)
    return table, otus, rx.denovo_check_host(table, otus, **params)


def test_the_three_files_are_the_library_s_texts(tmp_path, files):
    a, b = tmp_path / "on", tmp_path / "off"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--denovo", "--tags", files["sheet"], *COMMON)
    q = run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--tags", files["sheet"], *COMMON)
    table, otus, d = expected(files["reads"], files["sample"], samples=2)
    assert 4 <= d.n_flagged <= 8 and d.n_checked > d.n_flagged
    assert (a / "raxtax.otus.denovo").read_text() == rx.denovo_records_text(d)
    assert (a / "raxtax.otus.clean").read_text() == rx.denovo_fasta(d) != rx.otu_fasta(otus)
    assert (a / "raxtax.otus.clean.tsv").read_text() == rx.denovo_table_text(d, ["s0", "s1"])
    assert f"--denovo: {d.n_entries} OTUs, {d.n_checked} checked, {d.n_flagged} flagged, " in p.stderr and "--denovo" not in q.stderr
    for f in OTU_FILES + ("raxtax.uniques", "raxtax.out"):   # unchanged by the option
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    assert not any((b / f).exists() for f in NEW_FILES)
    assert json.loads((a / "raxtax.json").read_text())["denovo"] == "abskew=2;mindelta=24;segments=16" and "denovo" not in json.loads((b / "raxtax.json").read_text())
    # the settings reach the check, --otus-minsize the two clean files; a run that starts over without the option removes its files
    c = tmp_path / "set"
    run("-d", files["db"], "-i", files["tagged"], "-o", c, "--uniques", "--otus", "--otus-minsize", 2, "--denovo", "--denovo-abskew", 4, "--denovo-mindelta", 30,
        "--denovo-segments", 8, "--tags", files["sheet"], *COMMON)
    _, _, d2 = expected(files["reads"], files["sample"], samples=2, abskew=4, mindelta=30, segments=8)
    assert (c / "raxtax.otus.denovo").read_text() == rx.denovo_records_text(d2) != rx.denovo_records_text(d)
    assert (c / "raxtax.otus.clean").read_text() == rx.denovo_fasta(d2, minsize=2) and (c / "raxtax.otus.clean.tsv").read_text() == rx.denovo_table_text(d2, ["s0", "s1"], minsize=2)
    run("-d", files["db"], "-i", files["tagged"], "-o", c, "--uniques", "--otus", "--tags", files["sheet"], "--redo", *COMMON)
    assert (c / "raxtax.otus").exists() and not any((c / f).exists() for f in NEW_FILES)


def test_without_tags_no_table(tmp_path, files):
    a = tmp_path / "plain"
    run("-d", files["db"], "-i", files["plain"], "-o", a, "--uniques", "--otus", "--denovo", *COMMON)
    _, _, d = expected(files["reads"])
    assert (a / "raxtax.otus.denovo").read_text() == rx.denovo_records_text(d) and (a / "raxtax.otus.clean").read_text() == rx.denovo_fasta(d)
    assert not (a / "raxtax.otus.clean.tsv").exists()

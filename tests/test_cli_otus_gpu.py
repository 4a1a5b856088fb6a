"""raxtax-hip --uniques --otus (cli_main.cpp): PREFIX/raxtax.otus, raxtax.otus.map and, with --tags, raxtax.otus.tsv are byte for byte the
rx.otu_* texts of the table of the reads the run classified (rx.tally_reads, clustered on the host); --otus without --uniques is refused; a run
without --otus writes none of the three files."""
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
FILES = ("raxtax.otus", "raxtax.otus.map", "raxtax.otus.tsv")
CODE = {"A": 1, "C": 2, "G": 4, "T": 8}


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A database of 48 references of 160 bases; 190 reads: 20 centres taken from it, each with copies and with planted variants -- a
    substitution, a deletion, an insertion, and a variant of the substitution (two steps from the centre) -- between the tags of a sheet of
    three samples, every seventh read without tags."""
    d = tmp_path_factory.mktemp("otus")
    db = synth.make_db(48, length=160, fanouts=(2, 2, 2, 1, 1, 1))
    (d / "db.fasta").write_text(db.fasta())
    rng = np.random.default_rng(17)
    letters = "ACGT"
    reads = []
    for c, ref in enumerate(rng.choice(db.n, 20, replace=False)):
        centre = "".join("?AC?G???T"[b] for b in db.seq(int(ref)))
        i, j, k, m = (int(x) for x in rng.choice(len(centre), 4, replace=False))
        sub = centre[:i] + letters[(letters.index(centre[i]) + 1) % 4] + centre[i + 1:]
        far = sub[:j] + letters[(letters.index(sub[j]) + 2) % 4] + sub[j + 1:]
        reads += [centre] * (3 + c % 4) + [sub] * 2 + [centre[:k] + centre[k + 1:], centre[:m] + "G" + centre[m:], far]
    reads = [reads[int(p)] for p in rng.permutation(len(reads))]
    assert len(reads) == 190
    ftag, rtag = ["ACGTTGCA", "TTGACCAT", "GGATCTAC"], ["CATGGTCA", "AGCTAGGT", "TCCAGTGA"]
    (d / "sheet.tsv").write_text("".join(f"s{k}\t{ftag[k]}\t{rtag[k]}\n" for k in range(3)))
    tagged, sample = [], []
    for n, s in enumerate(reads):
        k = None if n % 7 == 6 else n % 3
        sample.append(k)
        tagged.append(s if k is None else ftag[k] + s + rtag[k].translate(_COMPLEMENT)[::-1])
    (d / "tagged.fasta").write_text("".join(f">read{n:03d}\n{s}\n" for n, s in enumerate(tagged)))
    (d / "plain.fasta").write_text("".join(f">read{n:03d}\n{s}\n" for n, s in enumerate(reads)))
    return dict(db=d / "db.fasta", tagged=d / "tagged.fasta", plain=d / "plain.fasta", sheet=d / "sheet.tsv", reads=reads, sample=sample)


def expected(reads, sample=None, samples=0):
    """the table of these reads and its OTUs, from the definition on the host"""
    seqs = [np.array([CODE[c] for c in s], np.uint8) for s in reads]
    table = rx.tally_reads(*concat(seqs), None if sample is None else np.array(sample, np.uint32), samples=samples)
    return table, rx.otu_cluster_host(table)


def test_the_three_files_are_the_library_s_texts(tmp_path, files):
    a = tmp_path / "tagged"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--tags", files["sheet"], *COMMON)
    kept = [(s, k) for s, k in zip(files["reads"], files["sample"]) if k is not None]        # the reads the run classified
    table, otus = expected([s for s, _ in kept], [k for _, k in kept], samples=3)
    assert 8 <= otus.n_otus < otus.n_rows and len(otus.links) >= 40 and otus.members.max() >= 4
    assert (a / "raxtax.uniques").read_text() == rx.tally_fasta(table)
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(otus)
    assert (a / "raxtax.otus.map").read_text() == rx.otu_map_text(otus)
    assert (a / "raxtax.otus.tsv").read_text() == rx.otu_table_text(otus, ["s0", "s1", "s2"])
    assert f"--otus: {otus.n_rows} distinct reads, {len(otus.links)} links, {otus.n_otus} OTUs, " in p.stderr
    assert json.loads((a / "raxtax.json").read_text())["otus"] == "minsize=1"
    # --otus-minsize leaves small OTUs out of the FASTA and the table, not out of the map; --uniques-minsize does not touch the clustering
    b = tmp_path / "minsize"
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--uniques-minsize", 3, "--otus", "--otus-minsize", 5, "--tags", files["sheet"], *COMMON)
    assert (b / "raxtax.otus").read_text() == rx.otu_fasta(otus, minsize=5) != rx.otu_fasta(otus)
    assert (b / "raxtax.otus.tsv").read_text() == rx.otu_table_text(otus, ["s0", "s1", "s2"], minsize=5)
    assert (b / "raxtax.otus.map").read_text() == rx.otu_map_text(otus)
    assert (b / "raxtax.uniques").read_text() == rx.tally_fasta(table, minsize=3)
    # a run that starts over in that folder without --otus removes the files
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--tags", files["sheet"], "--redo", *COMMON)
    assert (b / "raxtax.uniques").exists() and not any((b / f).exists() for f in FILES)


def test_without_tags_no_table_and_without_otus_no_file(tmp_path, files):
    a, b = tmp_path / "plain", tmp_path / "none"
    run("-d", files["db"], "-i", files["plain"], "-o", a, "--uniques", "--otus", *COMMON)
    table, otus = expected(files["reads"])
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(otus) and (a / "raxtax.otus.map").read_text() == rx.otu_map_text(otus)
    assert not (a / "raxtax.otus.tsv").exists()
    p = run("-d", files["db"], "-i", files["plain"], "-o", b, "--uniques", *COMMON)
    assert (b / "raxtax.uniques").read_text() == (a / "raxtax.uniques").read_text()
    assert not any((b / f).exists() for f in FILES) and "--otus" not in p.stderr
    assert "otus" not in json.loads((b / "raxtax.json").read_text())
    for f in ("raxtax.out", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def test_otus_needs_uniques(tmp_path, files):
    for args in (("--otus",), ("--uniques", "--otus-minsize", 2), ("--uniques", "--otus", "--otus-minsize", 0)):
        p = run("-d", files["db"], "-i", files["plain"], "-o", tmp_path / "bad", *args, *COMMON, ok=False)
        assert p.returncode == 64, (args, p.returncode, p.stderr)
    assert not (tmp_path / "bad" / "raxtax.out").exists()

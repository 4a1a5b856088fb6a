"""raxtax-hip --uniques --otus --unoise (cli_main.cpp) on a small FASTQ: PREFIX/raxtax.otus, raxtax.otus.map, raxtax.otus.tsv and
raxtax.otus.unoise are byte for byte the library's texts of the denoised table of the reads the run classified (denoised on the host), under
the larger of the two minsizes; with --denovo the chimera files are those of rx.denovo_check on that object; the refusals exit 64; a run
without the option writes what the clustering writes."""
import json

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth
from test_cli_otus_gpu import _COMPLEMENT, COMMON, expected, run
from unoise_common import tiers_of

pytestmark = pytest.mark.gpu
NAMES = ["s0", "s1", "s2"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """12 centres taken from a database of 48 references (10 distinct ones, some a single substitution apart: real variants, both abundant, both
    kept), 24 .. 28 copies each, with two reads one substitution away (twice each: light enough
    to be errors of the centre), a read with one base deleted and a read two substitutions away (once: too heavy for two differences, too small
    for a ZOTU); as FASTQ, between the tags of a sheet of three samples, every seventh read without tags."""
    d = tmp_path_factory.mktemp("unoise")
    db = synth.make_db(48, length=160, fanouts=(2, 2, 2, 1, 1, 1))
    (d / "db.fasta").write_text(db.fasta())
    rng = np.random.default_rng(29)
    letters = "ACGT"

    def sub(s, i, step=1):
        return s[:i] + letters[(letters.index(s[i]) + step) % 4] + s[i + 1:]

    reads, centres = [], set()
    for c, ref in enumerate(rng.choice(db.n, 12, replace=False)):
        centre = "".join("?AC?G???T"[b] for b in db.seq(int(ref)))
        centres.add(centre)
        i, j, k, m, n = (int(x) for x in rng.choice(len(centre), 5, replace=False))
        reads += [centre] * (24 + c % 5) + [sub(centre, i)] * 2 + [sub(centre, j, 2)] * 2 + [centre[:k] + centre[k + 1:], sub(sub(centre, m), n, 3)]
    reads = [reads[int(p)] for p in rng.permutation(len(reads))]
    ftag, rtag = ["ACGTTGCA", "TTGACCAT", "GGATCTAC"], ["CATGGTCA", "AGCTAGGT", "TCCAGTGA"]
    (d / "sheet.tsv").write_text("".join(f"s{k}\t{ftag[k]}\t{rtag[k]}\n" for k in range(3)))
    tagged, sample = [], []
    for n, s in enumerate(reads):
        k = None if n % 7 == 6 else n % 3
        sample.append(k)
        tagged.append(s if k is None else ftag[k] + s + rtag[k].translate(_COMPLEMENT)[::-1])
    (d / "tagged.fastq").write_text("".join(f"@read{n:03d}\n{s}\n+\n{'I' * len(s)}\n" for n, s in enumerate(tagged)))
    (d / "plain.fastq").write_text("".join(f"@read{n:03d}\n{s}\n+\n{'I' * len(s)}\n" for n, s in enumerate(reads)))
    return dict(db=d / "db.fasta", tagged=d / "tagged.fastq", plain=d / "plain.fastq", sheet=d / "sheet.tsv", reads=reads, sample=sample, centres=centres)


def denoised(files, **params):
    kept = [(s, k) for s, k in zip(files["reads"], files["sample"]) if k is not None]        # the reads the run classified
    table, otus = expected([s for s, _ in kept], [k for _, k in kept], samples=3)
    return table, otus, rx.otu_unoise_host(table, **params)


def test_the_four_files_are_the_library_s_texts(tmp_path, files):
    a = tmp_path / "tagged"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--unoise", "--denovo", "--tags", files["sheet"], *COMMON)
    table, otus, z = denoised(files)
    u = z.unoise
    n_centres = len(files["centres"])
    assert u["n_zotu"] == n_centres == 10 and u["n_absorbed"] >= 20 and u["n_left"] >= 6 and z.n_otus == u["n_zotu"] + u["n_left"] < otus.n_rows
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(z, minsize=8) != rx.otu_fasta(otus)
    assert len((a / "raxtax.otus").read_text().splitlines()) == 2 * n_centres
    assert (a / "raxtax.otus.map").read_text() == rx.otu_map_text(z)
    assert (a / "raxtax.otus.tsv").read_text() == rx.otu_table_text(z, NAMES, minsize=8)
    assert (a / "raxtax.otus.unoise").read_text() == rx.unoise_text(z)
    dn = rx.denovo_check(table, z)
    assert (a / "raxtax.otus.denovo").read_text() == rx.denovo_records_text(dn)
    assert (a / "raxtax.otus.clean").read_text() == rx.denovo_fasta(dn, minsize=8) and (a / "raxtax.otus.clean.tsv").read_text() == rx.denovo_table_text(dn, NAMES, minsize=8)
    tiers = len(tiers_of(table.sizes, 2)) - 1
    assert f"--unoise: {z.n_rows} distinct reads, {u['n_zotu']} ZOTUs, {u['n_absorbed']} absorbed, {u['n_left']} left, 0 long, {tiers} tiers\n" in p.stderr and tiers >= 2
    assert "--otus:" not in p.stderr
    assert json.loads((a / "raxtax.json").read_text())["unoise"] == "minsize=8;alpha=2;maxdiffs=16"
    # other settings are another run; --otus-minsize above --unoise-minsize wins
    b = tmp_path / "settings"
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--unoise", "--unoise-minsize", 2, "--unoise-alpha", 1, "--unoise-maxdiffs", 1,
        "--otus-minsize", 3, "--tags", files["sheet"], *COMMON)
    _, _, z2 = denoised(files, minsize=2, alpha=1, max_diffs=1)
    assert (b / "raxtax.otus.unoise").read_text() == rx.unoise_text(z2) != rx.unoise_text(z)
    assert (b / "raxtax.otus").read_text() == rx.otu_fasta(z2, minsize=3) and (b / "raxtax.otus.tsv").read_text() == rx.otu_table_text(z2, NAMES, minsize=3)
    assert json.loads((b / "raxtax.json").read_text())["unoise"] == "minsize=2;alpha=1;maxdiffs=1"
    # a run that starts over in that folder without the option removes the file and writes the files of the clustering
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--tags", files["sheet"], "--redo", *COMMON)
    assert not (b / "raxtax.otus.unoise").exists() and (b / "raxtax.otus").read_text() == rx.otu_fasta(otus)
    assert "unoise" not in json.loads((b / "raxtax.json").read_text())


def test_without_the_option_every_file_is_what_it_was(tmp_path, files):
    a = tmp_path / "plain"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--denovo", "--tags", files["sheet"], *COMMON)
    table, otus, _ = denoised(files)
    dn = rx.denovo_check_host(table, otus)
    want = {"raxtax.uniques": rx.tally_fasta(table), "raxtax.otus": rx.otu_fasta(otus), "raxtax.otus.map": rx.otu_map_text(otus), "raxtax.otus.tsv": rx.otu_table_text(otus, NAMES),
            "raxtax.otus.denovo": rx.denovo_records_text(dn), "raxtax.otus.clean": rx.denovo_fasta(dn), "raxtax.otus.clean.tsv": rx.denovo_table_text(dn, NAMES)}
    for name, text in want.items():
        assert (a / name).read_text() == text, name
    assert not (a / "raxtax.otus.unoise").exists() and "unoise" not in p.stderr
    assert "unoise" not in json.loads((a / "raxtax.json").read_text())
    # the per-read files do not know the option
    b = tmp_path / "unoise"
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--unoise", "--tags", files["sheet"], *COMMON)
    for f in ("raxtax.out", "raxtax.ckp", "raxtax.demux", "raxtax.uniques", "raxtax.uniques.tsv"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def test_the_refusals_exit_64(tmp_path, files):
    for args in (("--uniques", "--unoise"), ("--uniques", "--otus", "--unoise-alpha", 2), ("--uniques", "--otus", "--unoise-minsize", 2), ("--uniques", "--otus", "--unoise-maxdiffs", 2),
                 ("--uniques", "--otus", "--unoise", "--fastidious"), ("--uniques", "--otus", "--unoise", "--unoise-alpha", 9), ("--uniques", "--otus", "--unoise", "--unoise-maxdiffs", 17)):
        p = run("-d", files["db"], "-i", files["plain"], "-o", tmp_path / "bad", *args, *COMMON, ok=False)
        assert p.returncode == 64, (args, p.returncode, p.stderr)
    assert not (tmp_path / "bad" / "raxtax.out").exists()

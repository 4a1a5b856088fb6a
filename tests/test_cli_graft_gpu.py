"""raxtax-hip --uniques --otus --fastidious (cli_main.cpp): PREFIX/raxtax.otus, raxtax.otus.map, raxtax.otus.tsv and raxtax.otus.grafts are byte for
byte the rx.otu_* texts of the grafted OTUs of the table of the reads the run classified (clustered and grafted on the host); without the option
every file is the file of a run that never knew it; --fastidious without --otus is refused."""
import json

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import synth
from test_cli_otus_gpu import _COMPLEMENT, COMMON, expected, run

pytestmark = pytest.mark.gpu
NAMES = ["s0", "s1", "s2"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The reads of test_cli_otus_gpu.py with other variants: 20 centres taken from a database of 48 references, each with copies, a
    substitution, a deletion, and two reads that are TWO steps from the centre with nothing in between -- two substitutions; a substitution
    and an insertion -- which the clustering leaves alone and the graft takes.  Tags of three samples, every seventh read without."""
    d = tmp_path_factory.mktemp("grafts")
    db = synth.make_db(48, length=160, fanouts=(2, 2, 2, 1, 1, 1))
    (d / "db.fasta").write_text(db.fasta())
    rng = np.random.default_rng(23)
    letters = "ACGT"

    def sub(s, i, step=1):
        return s[:i] + letters[(letters.index(s[i]) + step) % 4] + s[i + 1:]

    reads = []
    for c, ref in enumerate(rng.choice(db.n, 20, replace=False)):
        centre = "".join("?AC?G???T"[b] for b in db.seq(int(ref)))
        i, j, k, m, n = (int(x) for x in rng.choice(len(centre), 5, replace=False))
        far = sub(sub(centre, j, 2), m)
        reads += [centre] * (3 + c % 4) + [sub(centre, i)] * 2 + [centre[:k] + centre[k + 1:], far, sub(centre, n, 3)[:k] + "G" + sub(centre, n, 3)[k:]]
    reads = [reads[int(p)] for p in rng.permutation(len(reads))]
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


def test_the_four_files_are_the_library_s_texts(tmp_path, files):
    a = tmp_path / "tagged"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--fastidious", "--denovo", "--tags", files["sheet"], *COMMON)
    kept = [(s, k) for s, k in zip(files["reads"], files["sample"]) if k is not None]        # the reads the run classified
    table, otus = expected([s for s, _ in kept], [k for _, k in kept], samples=3)
    grafted = rx.otu_graft_host(otus)
    info = grafted.graft_info
    assert info["grafts"] >= 5 and grafted.n_otus == otus.n_otus - info["grafts"]            # (the reads two steps from their centres)
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(grafted) != rx.otu_fasta(otus)
    assert (a / "raxtax.otus.map").read_text() == rx.otu_map_text(grafted)
    assert (a / "raxtax.otus.tsv").read_text() == rx.otu_table_text(grafted, NAMES)
    assert (a / "raxtax.otus.grafts").read_text() == rx.otu_grafts_text(grafted)
    assert (a / "raxtax.otus.denovo").read_text() == rx.denovo_records_text(rx.denovo_check_host(table, grafted))
    assert f"--otus: {otus.n_rows} distinct reads, {len(otus.links)} links, {otus.n_otus} OTUs, " in p.stderr
    assert (f"--fastidious: boundary 3, {info['heavy_otus']} heavy and {info['light_otus']} light OTUs, {info['grafts']} grafts, {grafted.n_otus} OTUs left\n") in p.stderr
    assert json.loads((a / "raxtax.json").read_text())["fastidious"] == "boundary=3"
    # another boundary is another run
    b = tmp_path / "boundary"
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--fastidious", "--fastidious-boundary", 4, "--tags", files["sheet"], *COMMON)
    four = rx.otu_graft_host(otus, boundary=4)
    assert (b / "raxtax.otus.grafts").read_text() == rx.otu_grafts_text(four) and (b / "raxtax.otus").read_text() == rx.otu_fasta(four)
    assert json.loads((b / "raxtax.json").read_text())["fastidious"] == "boundary=4"
    # a run that starts over in that folder without the option removes the file and writes the files of the clustering
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--tags", files["sheet"], "--redo", *COMMON)
    assert not (b / "raxtax.otus.grafts").exists() and (b / "raxtax.otus").read_text() == rx.otu_fasta(otus)
    assert "fastidious" not in json.loads((b / "raxtax.json").read_text())


def test_without_the_option_every_file_is_what_it_was(tmp_path, files):
    a = tmp_path / "plain"
    p = run("-d", files["db"], "-i", files["tagged"], "-o", a, "--uniques", "--otus", "--denovo", "--tags", files["sheet"], *COMMON)
    kept = [(s, k) for s, k in zip(files["reads"], files["sample"]) if k is not None]
    table, otus = expected([s for s, _ in kept], [k for _, k in kept], samples=3)
    dn = rx.denovo_check_host(table, otus)
    want = {"raxtax.uniques": rx.tally_fasta(table), "raxtax.otus": rx.otu_fasta(otus), "raxtax.otus.map": rx.otu_map_text(otus), "raxtax.otus.tsv": rx.otu_table_text(otus, NAMES),
            "raxtax.otus.denovo": rx.denovo_records_text(dn), "raxtax.otus.clean": rx.denovo_fasta(dn), "raxtax.otus.clean.tsv": rx.denovo_table_text(dn, NAMES)}
    for name, text in want.items():
        assert (a / name).read_text() == text, name
    assert not (a / "raxtax.otus.grafts").exists() and "fastidious" not in p.stderr
    assert "fastidious" not in json.loads((a / "raxtax.json").read_text())
    # the per-read files do not know the option
    b = tmp_path / "fastidious"
    run("-d", files["db"], "-i", files["tagged"], "-o", b, "--uniques", "--otus", "--fastidious", "--tags", files["sheet"], *COMMON)
    for f in ("raxtax.out", "raxtax.ckp", "raxtax.demux", "raxtax.uniques", "raxtax.uniques.tsv"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def test_fastidious_needs_otus(tmp_path, files):
    for args in (("--uniques", "--fastidious"), ("--uniques", "--otus", "--fastidious-boundary", 2), ("--uniques", "--otus", "--fastidious", "--fastidious-boundary", 0)):
        p = run("-d", files["db"], "-i", files["plain"], "-o", tmp_path / "bad", *args, *COMMON, ok=False)
        assert p.returncode == 64, (args, p.returncode, p.stderr)
    assert not (tmp_path / "bad" / "raxtax.out").exists()

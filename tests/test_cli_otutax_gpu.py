"""raxtax-hip --uniques --otus --otus-tax CUTOFF (cli_main.cpp): PREFIX/raxtax.otus.tax is byte for byte OtuTaxonomy.text of rx.otu_taxonomy_host,
fed by rx.best_lineages of a Python Index.classify over the rows of the table that raxtax.uniques describes -- with --fastidious of the grafted
OTUs; --otus-tax without --otus is refused; a run without the option writes no such file and has no such key in raxtax.json."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from tally_common import concat

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def python_side():
    """the table of the query file's reads, its rows classified once in Python, and the records of that at a cutoff of 0.8 -- made once"""
    tree = rx.parse_reference_fasta_str(DB.read_text())
    queries = rx.parse_query_fasta_str(QUERIES.read_text())
    table = rx.tally_reads(*concat([s for _, s in queries]))
    bases, off = concat(table.seqs)
    index = rx.Index(tree, device=0)
    res = index.classify(bases, off)
    lin = rx.best_lineages(tree, res, cutoff=80, exact=index.device_exact_matches())
    assert len(lin) == len(table.sizes) > 1000 and int((lin.L > 0).sum()) > len(lin) // 2
    return tree, table, lin


def test_the_file_is_the_library_s_text(tmp_path, python_side):
    tree, table, lin = python_side
    a, b = tmp_path / "tax", tmp_path / "none"
    p = run("-d", DB, "-i", QUERIES, "-o", a, "--skip-db", "--uniques", "--otus", "--otus-tax", 0.8)
    assert (a / "raxtax.uniques").read_text() == rx.tally_fasta(table)      # the table the file describes is the one classified here
    otus = rx.otu_cluster(table)
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(otus)
    tax = rx.otu_taxonomy_host(tree, otus, lin)
    got = (a / "raxtax.otus.tax").read_text()
    assert got == tax.text(tree, minsize=1)
    named = int((tax.depth > 0).sum())
    assert 0 < named <= tax.n_otus == otus.n_otus and len(got.splitlines()) == otus.n_otus + 1 and len(set(tax.seed_rel.tolist())) >= 2
    assert f"--otus-tax: {otus.n_otus} OTUs, {named} with a taxon, " in p.stderr
    assert json.loads((a / "raxtax.json").read_text())["otus_tax"] == "cutoff=80;agree=51"
    # a higher agreement and --otus-minsize: other lines, the same numbers; --batch 512: the second pass in many chunks
    c = tmp_path / "agree"
    run("-d", DB, "-i", QUERIES, "-o", c, "--skip-db", "--batch", 512, "--uniques", "--otus", "--otus-minsize", 3, "--otus-tax", 0.8, "--otus-tax-agree", 90)
    assert (c / "raxtax.otus.tax").read_text() == rx.otu_taxonomy_host(tree, otus, lin, agree=90).text(tree, minsize=3) != got
    # without the option: no file, no key, and the other files are what they are with it
    q = run("-d", DB, "-i", QUERIES, "-o", b, "--skip-db", "--uniques", "--otus")
    assert not (b / "raxtax.otus.tax").exists() and "otus_tax" not in json.loads((b / "raxtax.json").read_text()) and "--otus-tax" not in q.stderr
    for f in ("raxtax.out", "raxtax.uniques", "raxtax.otus", "raxtax.otus.map"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # a run that starts over in that folder without the option removes the file
    run("-d", DB, "-i", QUERIES, "-o", a, "--skip-db", "--uniques", "--otus", "--redo")
    assert (a / "raxtax.otus").exists() and not (a / "raxtax.otus.tax").exists()


def test_with_fastidious_the_grafted_otus_are_named(tmp_path, python_side):
    tree, table, lin = python_side
    a = tmp_path / "grafted"
    run("-d", DB, "-i", QUERIES, "-o", a, "--skip-db", "--uniques", "--otus", "--fastidious", "--otus-tax", 0.8)
    before = rx.otu_cluster(table)
    otus = rx.otu_graft(before)
    assert otus.n_otus < before.n_otus
    assert (a / "raxtax.otus").read_text() == rx.otu_fasta(otus)
    assert (a / "raxtax.otus.tax").read_text() == rx.otu_taxonomy_host(tree, otus, lin).text(tree, minsize=1)


def test_otus_tax_needs_otus(tmp_path):
    for args in (("--otus-tax", 0.8), ("--uniques", "--otus-tax", 0.8), ("--uniques", "--otus", "--otus-tax-agree", 60), ("--uniques", "--otus", "--otus-tax", 0),
                 ("--uniques", "--otus", "--otus-tax", 0.8, "--otus-tax-agree", 50)):
        p = run("-d", DB, "-i", QUERIES, "-o", tmp_path / "bad", "--skip-db", *args, ok=False)
        assert p.returncode == 64, (args, p.returncode, p.stderr)
    assert not (tmp_path / "bad" / "raxtax.out").exists()

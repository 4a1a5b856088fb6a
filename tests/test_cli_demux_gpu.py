"""raxtax-hip --tags (cli_main.cpp): rtx_index_set_tags on every handle.  On a FASTA of tagged, primer-carrying reads raxtax.demux and -- with
--profile -- raxtax.samples are byte for byte what the Python API gives on the same input (the demux callback of rx.raxtax, and
rx.sample_table_text of the handle's per-sample counters); `.out` is that of the API run as well."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from demux_common import NONE, other, spaced_tags

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


@pytest.fixture(scope="module")
def pooled(tmp_path_factory):
    """300 reads of four samples (one line of the sheet receives nothing): tag + primer + amplicon + revcomp(primer) + tag, some with a spacer, a
    tag error, a missing tag or a pair of tags that is no pair."""
    d = tmp_path_factory.mktemp("pooled")
    amplicons = rx.parse_query_fasta_str(QUERIES.read_text())[:300]
    rng = np.random.default_rng(52)
    ftag, rtag = spaced_tags(rng, 5, 8), spaced_tags(rng, 5, 8)
    owner = ["north", "south", "south", "blank", "east"]
    sheet = d / "tags.tsv"
    sheet.write_text("# sample\tfwd\trev\n" + "".join(f"{owner[k]}\t{text(ftag[k])}\t{text(rtag[k])}\n" for k in range(5)))
    inst = lambda t: np.array([rng.choice([b for b in (1, 2, 4, 8) if c & b]) for c in rx.encode_iupac(t)], np.uint8)
    queries = []
    for i, (label, amp) in enumerate(amplicons):
        k = (0, 1, 2, 4)[i % 4]
        t5, t3 = ftag[k].copy(), rx.api.revcomp(rtag[k])
        if i % 5 == 1:
            t5[int(rng.integers(0, 8))] = 15                                 # N in the read: it matches whatever the tag holds there
        if i % 5 == 2:
            pos = int(rng.integers(0, 8))
            t3[pos] = other(t3[pos])                                         # a substitution
        body = np.concatenate([inst(FWD), amp, rx.api.revcomp(inst(REV))])
        sp = (1 << rng.integers(0, 4, i % 3)).astype(np.uint8)
        if 128 <= i < 192:
            read = body                                                      # no tags
        elif i % 13 == 0:
            read = np.concatenate([sp, t5, body])                            # no 3' tag
        elif i % 17 == 0:
            read = np.concatenate([ftag[0], body, rx.api.revcomp(rtag[1])])  # no such pair
        else:
            read = np.concatenate([sp, t5, body, t3, sp])
        queries.append((f"q{i:03d};{label.split()[0]}", read.astype(np.uint8)))
    raw = d / "raw.fasta"
    raw.write_text("".join(f">{label}\n{text(seq)}\n" for label, seq in queries))
    return d, sheet, raw, queries


def test_the_files_are_what_the_api_gives(pooled, tmp_path):
    d, sheet, raw, queries = pooled
    tags, pairs, names = rx.sample_sheet(sheet.read_text())
    assert names == ["north", "south", "blank", "east"]
    tree = rx.parse_reference_fasta_str(DB.read_text())
    index = rx.Index(tree, tags=(tags, pairs, rx.DemuxParams(1, 2)), primers=rx.primer_patterns((FWD, REV)))
    index.profile_begin(0.8, n_samples=len(names))
    sent, rows = [], []
    rx.raxtax(queries, index, False, False, 128, lambda label, out, tsv: sent.append(out), False, demux=lambda *a: rows.append(a))
    table = rx.sample_table_text(tree, names, index.profile_read_samples())
    a = tmp_path / "tagged"
    p = run("-d", DB, "-i", raw, "-o", a, "--skip-db", "--batch", 128, "--tags", sheet, "--tag-mismatches", 1, "--tag-offset", 2, "--primers", f"{FWD}:{REV}",
            "--profile", 0.8)
    assert (a / "raxtax.out").read_text() == "".join(s + "\n" for s in sent) and len(sent) > 100
    verdicts = rx.demux_verdict_names()
    want = ["label\tsample\tverdict\ttag5\tmm5\toff5\ttag3\tmm3\toff3\tlo\thi"]
    for label, _raw_len, sample, lo, hi, hit, info in rows:
        v, t5, m5, o5, t3, m3, o3 = rx.demux_hit(hit, info)
        end = lambda t, m, o: ("-", "-", "-") if t is None else (str(t), str(m), str(o))
        want.append("\t".join((label, "*" if sample == NONE else names[sample], verdicts[v], *end(t5, m5, o5), *end(t3, m3, o3), str(lo), str(hi))))
    assert (a / "raxtax.demux").read_text().splitlines() == want
    seen = {l.split("\t")[2] for l in want[1:]}
    assert seen == {"ok", "no_tag5", "no_tag3", "unknown_pair"} and {l.split("\t")[1] for l in want[1:]} == {"north", "south", "east", "*"}
    assert (a / "raxtax.samples").read_text() == table
    assert table.splitlines()[5] == "depth\ttaxon\tlineage\tnorth\tsouth\tblank\teast" and len(table.splitlines()) > 10
    n_ok = sum(1 for r in rows if r[2] != NONE)
    m = re.search(r"\[INFO \] --tags: (\d+) queries, (\d+) assigned to a sample", p.stderr)
    assert m and (int(m.group(1)), int(m.group(2))) == (300, n_ok) and 150 < n_ok < 300, p.stderr
    assert (a / "raxtax.profile").exists() and (a / "raxtax.trim").exists()
    # a run without --tags writes neither file
    b = tmp_path / "plain"
    run("-d", DB, "-i", raw, "-o", b, "--skip-db", "--batch", 128, "--profile", 0.8)
    assert (b / "raxtax.profile").exists() and not (b / "raxtax.demux").exists() and not (b / "raxtax.samples").exists()


def test_refusals_come_before_any_device_work(pooled, tmp_path):
    d, sheet, raw, _ = pooled
    p = run("-d", DB, "-i", raw, "-o", tmp_path / "out", "--tags", sheet, "--derep", "--profile", 0.8, ok=False)
    assert "--derep" in p.stderr and "--profile" in p.stderr and "copies from different samples" in p.stderr and not (tmp_path / "out").exists()
    p = run("-d", DB, "-i", raw, "-o", tmp_path / "out", "--tag-mismatches", 1, ok=False)
    assert "--tags SHEET" in p.stderr
    p = run("-d", DB, "-i", raw, "-o", tmp_path / "out", "--tags", sheet, "--tag-offset", 16, ok=False)
    assert "0 .. 15" in p.stderr
    bad = tmp_path / "bad.tsv"
    bad.write_text("a\tACGT\tTTGA\nb\tACGT\tTTGA\n")
    p = run("-d", DB, "-i", raw, "-o", tmp_path / "out", "--tags", bad, ok=False)
    assert "twice" in p.stderr and not (tmp_path / "out").exists()
    bad.write_text("a\tACXT\tTTGA\n")
    p = run("-d", DB, "-i", raw, "-o", tmp_path / "out", "--tags", bad, ok=False)
    assert "IUPAC" in p.stderr

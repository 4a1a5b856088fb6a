"""raxtax-hip --hits (cli_main.cpp, RTX_OPT_NEAREST): PREFIX/raxtax.hits has one line per query in the order of raxtax.out --
label, strand, peak, t, ties, id and lineage of the nearest reference -- every one of them held against the oracle's hit counts (the lowest
index of the maximum, the number of entries equal to it, `-` twice and 0 ties where the maximum is 0); the file takes part in resume and
the flag in the checkpoint, and a run without the flag writes what it always wrote."""
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
_COMP = np.arange(256, dtype=np.uint8)
_COMP[:16] = [int(f"{c:04b}"[::-1], 2) for c in range(16)]


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The first 600 records as they are, and with every third one reverse-complemented (as text: the complement of the letters, reversed)."""
    d = tmp_path_factory.mktemp("hits_queries")
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


@pytest.fixture(scope="module")
def expected(oracle, files):
    """Per skip mode: the lines of raxtax.hits without the strand column, from the oracle -- (label, peak, t, ties, id, lineage) per query."""
    plain, _ = files
    otree = oracle.parse_reference_fasta_str(DB.read_text())
    lineages = otree.lineages
    queries = oracle.parse_query_fasta_str(plain.read_text())
    assert len(queries) == 600
    out = {}
    for skip in (False, True):
        lines, rev_peaks = [], []
        for label, seq in queries:
            seq = np.asarray(seq, dtype=np.uint8)
            t, counts = otree.hit_counts(seq, skip_exact=skip)
            try:
                otree.classify(seq, skip_exact=skip, raw_confidence=True)
                m = int(counts.max())
            except ArithmeticError:
                m = 0
            if m == 0:
                lines.append([label, "0", str(int(t)), "0", "-", "-"])
            else:
                r = int(np.argmax(counts))
                lines.append([label, str(m), str(int(t)), str(int((counts == m).sum())), str(r), lineages[r]])
            rev_peaks.append(m - int(otree.hit_counts(_COMP[seq[::-1]], skip_exact=skip)[1].max()))
        out[skip] = (lines, min(rev_peaks))
    return out


@pytest.mark.parametrize("skip", [False, True])
def test_every_line_against_the_oracle(tmp_path, expected, files, skip):
    plain, mixed = files
    want, margin = expected[skip]
    extra = ["--skip-exact-matches"] if skip else []
    a, b = tmp_path / "hits", tmp_path / "none"
    run("-d", DB, "-i", plain, "-o", a, "--skip-db", "--tsv", "--batch", 128, "--hits", *extra)
    run("-d", DB, "-i", plain, "-o", b, "--skip-db", "--tsv", "--batch", 128, *extra)
    # a run without the flag: no file, no word of it in the checkpoint; with it: the same result files
    assert not (b / "raxtax.hits").exists() and "hits" not in (b / "raxtax.json").read_text()
    assert '"hits": true' in (a / "raxtax.json").read_text() and not (a / "raxtax.strand").exists()
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    lines = [l.split("\t") for l in (a / "raxtax.hits").read_text().splitlines()]
    assert [l[0] for l in lines] == (a / "raxtax.ckp").read_text().splitlines()
    by_label = {w[0]: w for w in want}
    assert len(lines) == len(set(l[0] for l in lines)) and len(lines) > 500
    for l in lines:   # (a query without a message has no line; every other one has exactly its own)
        w = by_label[l[0]]
        assert l == [w[0], "+", *w[1:]], (l, w)
    n_ties = sum(int(l[4]) >= 2 for l in lines)
    print(f"skip {skip}: {len(lines)} lines, {n_ties} with ties, {sum(l[5] == '-' for l in lines)} without a reference")
    # --device-format: the same file
    c = tmp_path / "dev"
    run("-d", DB, "-i", plain, "-o", c, "--skip-db", "--tsv", "--batch", 128, "--hits", "--device-format", *extra)
    assert (c / "raxtax.hits").read_bytes() == (a / "raxtax.hits").read_bytes() and (c / "raxtax.out").read_bytes() == (a / "raxtax.out").read_bytes()
    if not skip:   # --strand both on the flipped records: the lines of the oriented file, - at every third
        assert margin > 0, margin   # (the orientation that lost is below everywhere: no tie between the strands on this fixture)
        d = tmp_path / "both"
        run("-d", DB, "-i", mixed, "-o", d, "--skip-db", "--batch", 128, "--hits", "--strand", "both")
        both = [l.split("\t") for l in (d / "raxtax.hits").read_text().splitlines()]
        order = {w[0]: i for i, w in enumerate(want)}
        assert [l[0] for l in both] == [l[0] for l in lines]
        for l in both:
            w = by_label[l[0]]
            assert l == [w[0], "-" if order[l[0]] % 3 == 0 else "+", *w[1:]], (l, w)
        assert (d / "raxtax.strand").exists() and '"hits": true' in (d / "raxtax.json").read_text() and '"strand": "both"' in (d / "raxtax.json").read_text()


def test_resume_and_the_flag_in_the_checkpoint(tmp_path, files):
    plain, _ = files
    full = tmp_path / "full"
    run("-d", DB, "-i", plain, "-o", full, "--skip-db", "--batch", 128, "--hits")
    want = {f: (full / f).read_text().splitlines() for f in ("raxtax.out", "raxtax.hits", "raxtax.ckp")}
    assert len(want["raxtax.hits"]) == len(want["raxtax.ckp"]) > 500
    # interrupted: 250 queries finished, every output cut in the middle of a line of an unfinished query
    part = tmp_path / "part"
    shutil.copytree(full, part)
    done = set(want["raxtax.ckp"][:250])
    (part / "raxtax.ckp").write_text("\n".join(want["raxtax.ckp"][:250]) + "\n")
    for f in ("raxtax.out", "raxtax.hits"):
        keep = [l for l in want[f] if l.split("\t")[0] in done]
        nxt = next(l for l in want[f] if l.split("\t")[0] not in done)
        (part / f).write_text("\n".join(keep) + "\n" + nxt[: max(len(nxt) // 2, nxt.index("\t") + 2)])
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--hits")
    assert "Restarting from checkpoint" in p.stderr
    for f, lines in want.items():
        assert sorted((part / f).read_text().splitlines()) == sorted(lines), f
    # without the flag the checkpoint does not apply: the run starts over and removes the file
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128)
    assert "Restarting from checkpoint" not in p.stderr
    assert not (part / "raxtax.hits").exists() and "hits" not in (part / "raxtax.json").read_text()
    assert (part / "raxtax.out").read_text().splitlines() == want["raxtax.out"]
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--hits")
    assert "Restarting from checkpoint" not in p.stderr
    for f, lines in want.items():
        assert (part / f).read_text().splitlines() == lines, f

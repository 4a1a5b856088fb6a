"""raxtax-hip --uniques (cli_main.cpp): PREFIX/raxtax.uniques is the FASTA of the distinct reads of the whole run with their abundances -- byte for
byte what a Python dict over the file's sequences gives, although the file is read in several blocks; --tags adds the sequence x sample table;
--uniques-minsize drops small entries and keeps the ranks; a run without the option writes neither file and the checkpoint it always wrote; a
run that would resume a checkpoint with processed queries is refused, because its table would miss them."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "raxtax_amd" / "raxtax-hip"
DB = ROOT / "tests" / "golden" / "diptera_subset.fasta"
QUERIES = ROOT / "tests" / "golden" / "diptera_queries.fasta"
_COMPLEMENT = str.maketrans("ACGT", "TGCA")
BLOCK = 8000
COMMON = ("--skip-db", "--batch", 16, "--block-bytes", BLOCK)


def run(*args, ok=True):
    p = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr
    return p


def expected(reads, minsize=1, samples=None):
    """(the FASTA, the table) of (sequence, sample or None) reads: a dict, sorted by size descending and then by the codes of the sequence"""
    code = {"A": 1, "C": 2, "G": 4, "T": 8}
    table = {}
    for seq, sample in reads:
        if seq and sample is not None:
            table.setdefault(seq, [0] * (len(samples) if samples else 1))[sample] += 1
    rows = sorted(table.items(), key=lambda kv: (-sum(kv[1]), [code[c] for c in kv[0]]))
    fasta = "".join(f">uniq{r + 1};size={sum(v)}\n{k}\n" for r, (k, v) in enumerate(rows) if sum(v) >= minsize)
    text = "#uniq\t" + "\t".join(samples or ["all"]) + "\n" + "".join(f"uniq{r + 1}\t" + "\t".join(map(str, v)) + "\n" for r, (k, v) in enumerate(rows) if sum(v) >= minsize)
    return fasta, text


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """240 reads of plain A C G T from the first records of the query file -- every fifth a copy of an earlier one, far enough back for another
    block of the file -- as they are, and with the tags of a sheet of three samples around them (every seventh without tags)."""
    d = tmp_path_factory.mktemp("uniques_queries")
    seqs = []
    for r in [r for r in QUERIES.read_text().split(">") if r]:
        seq = r.partition("\n")[2].replace("\n", "").upper()
        if re.fullmatch("[ACGT]+", seq) and seq not in seqs:
            seqs.append(seq)
        if len(seqs) == 200:
            break
    assert len(seqs) == 200
    reads = []
    for i in range(240):
        reads.append(seqs[(i * 7) % 60] if i % 5 == 4 else seqs[i - i // 5])
    assert 150 < len(set(reads)) < 240
    ftag, rtag = ["ACGTTGCA", "TTGACCAT", "GGATCTAC"], ["CATGGTCA", "AGCTAGGT", "TCCAGTGA"]
    (d / "plain.fasta").write_text("".join(f">read{i:03d}\n{s}\n" for i, s in enumerate(reads)))
    (d / "sheet.tsv").write_text("".join(f"s{k}\t{ftag[k]}\t{rtag[k]}\n" for k in range(3)))
    tagged, sample = [], []
    for i, s in enumerate(reads):
        k = None if i % 7 == 6 else i % 3
        sample.append(k)
        tagged.append(s if k is None else ftag[k] + s + rtag[k].translate(_COMPLEMENT)[::-1])
    (d / "tagged.fasta").write_text("".join(f">read{i:03d}\n{s}\n" for i, s in enumerate(tagged)))
    assert (d / "plain.fasta").stat().st_size > 4 * BLOCK      # the file takes several calls, a call several chunks
    return dict(plain=d / "plain.fasta", tagged=d / "tagged.fasta", sheet=d / "sheet.tsv", reads=reads, sample=sample)


def test_the_fasta_is_the_dict_s(tmp_path, files):
    a, b, c, e = tmp_path / "uniques", tmp_path / "none", tmp_path / "two", tmp_path / "capped"
    p = run("-d", DB, "-i", files["plain"], "-o", a, "--uniques", *COMMON)
    want, _ = expected([(s, 0) for s in files["reads"]])
    assert (a / "raxtax.uniques").read_text() == want
    assert want.startswith(">uniq1;size=") and int(want.split("size=")[1].split("\n")[0]) >= 3
    assert f"--uniques: 240 reads, {len(set(files['reads']))} distinct" in p.stderr and "beyond the caps" not in p.stderr
    assert not (a / "raxtax.uniques.tsv").exists()             # (no --tags: no table)
    # without the option: neither file, and the checkpoint it always wrote; the result files are the same
    run("-d", DB, "-i", files["plain"], "-o", b, *COMMON)
    assert not (b / "raxtax.uniques").exists() and not (b / "raxtax.uniques.tsv").exists()
    ckp = (b / "raxtax.json").read_text()
    assert list(json.loads(ckp)) == ["db_fingerprint", "raw_confidence", "skip_exact_matches", "tsv"] and "uniques" not in ckp
    assert json.loads((a / "raxtax.json").read_text())["uniques"] == "minsize=1 max_entries=0 max_bytes=0"
    assert {k: v for k, v in json.loads((a / "raxtax.json").read_text()).items() if k != "uniques"} == json.loads(ckp)
    for f in ("raxtax.out", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # two handles on the device, with --derep: one object each, summed at the end; --uniques-minsize 2 drops the singletons, the ranks stay
    run("-d", DB, "-i", files["plain"], "-o", c, "--uniques", "--uniques-minsize", 2, "--devices", "0,0", "--derep", *COMMON)
    small, _ = expected([(s, 0) for s in files["reads"]], minsize=2)
    assert (c / "raxtax.uniques").read_text() == small and 0 < small.count(">") < want.count(">") and want.startswith(small)
    # a run that starts over in the folder of a --uniques run removes its file
    run("-d", DB, "-i", files["plain"], "-o", c, "--redo", *COMMON)
    assert not (c / "raxtax.uniques").exists()
    # beyond the caps: the log says how many reads are in no entry
    p = run("-d", DB, "-i", files["plain"], "-o", e, "--uniques", "--uniques-max-entries", 5, *COMMON)
    first5 = list(dict.fromkeys(files["reads"]))[:5]
    capped, _ = expected([(s, 0) for s in files["reads"] if s in first5])
    assert (e / "raxtax.uniques").read_text() == capped
    assert f"--uniques: {240 - sum(s in first5 for s in files['reads'])} of 240 reads belong to sequences beyond the caps" in p.stderr
    for bad in (("--uniques-minsize", "0"), ("--uniques-max-entries", "x"), ("--uniques-minsize", "2")):    # (the last: without --uniques)
        args = ("--uniques",) + bad if bad[1] != "2" else bad
        assert run("-d", DB, "-i", files["plain"], "-o", tmp_path / "bad", *args, ok=False).returncode == 64


def test_tags_add_the_table(tmp_path, files):
    a = tmp_path / "tagged"
    run("-d", DB, "-i", files["tagged"], "-o", a, "--uniques", "--tags", files["sheet"], *COMMON)
    fasta, table = expected(list(zip(files["reads"], files["sample"])), samples=["s0", "s1", "s2"])
    assert (a / "raxtax.uniques").read_text() == fasta
    assert (a / "raxtax.uniques.tsv").read_text() == table
    rows = [list(map(int, l.split("\t")[1:])) for l in table.splitlines()[1:]]
    assert any(sum(1 for x in r if x) > 1 for r in rows) and sum(map(sum, rows)) == sum(k is not None for k in files["sample"])
    # --tags with --derep and --uniques is allowed: every read counts in its own sample
    b = tmp_path / "derep"
    run("-d", DB, "-i", files["tagged"], "-o", b, "--uniques", "--tags", files["sheet"], "--derep", *COMMON)
    assert (b / "raxtax.uniques.tsv").read_text() == table and (b / "raxtax.uniques").read_text() == fasta


def test_a_resumed_run_is_refused_and_redo_runs(tmp_path, files):
    full = tmp_path / "full"
    run("-d", DB, "-i", files["plain"], "-o", full, "--uniques", *COMMON)
    want = (full / "raxtax.uniques").read_text()
    ckp = (full / "raxtax.ckp").read_text().splitlines()
    part = tmp_path / "part"
    shutil.copytree(full, part)
    (part / "raxtax.ckp").write_text("\n".join(ckp[:100]) + "\n")
    out_before = (part / "raxtax.out").read_bytes()
    p = run("-d", DB, "-i", files["plain"], "-o", part, "--uniques", *COMMON, ok=False)
    assert p.returncode == 64 and "--redo" in p.stderr and "--uniques" in p.stderr, (p.returncode, p.stderr)
    assert (part / "raxtax.out").read_bytes() == out_before    # (refused before anything was touched)
    run("-d", DB, "-i", files["plain"], "-o", part, "--uniques", "--redo", *COMMON)
    assert (part / "raxtax.uniques").read_text() == want and (part / "raxtax.out").read_bytes() == (full / "raxtax.out").read_bytes()
    # other settings are another checkpoint: the run starts over instead of resuming
    p = run("-d", DB, "-i", files["plain"], "-o", part, "--uniques", "--uniques-minsize", 3, *COMMON)
    assert "Restarting from checkpoint" not in p.stderr and (part / "raxtax.uniques").read_text() == expected([(s, 0) for s in files["reads"]], minsize=3)[0]

"""raxtax-hip up to the creation of the index handles (raxtax_amd/csrc/cli_main.cpp), on a machine without a GPU: everything the command line
decides before it touches a device -- the refusals and their order, the text of the checkpoint raxtax.json byte for byte, resume with the purge
of every per-read report, a changed option starting over.  Under --only-db the whole run finishes on the CPU (the database is parsed and
cached, no handle is created), so every case here is one or two such runs on the 600 references of tests/golden/diptera_subset.fasta."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FASTA = ROOT / "tests" / "golden" / "diptera_subset.fasta"
FASTQ_TEXT = "@r1\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n"
SHEET_TEXT = "# sample\tfwd_tag\trev_tag\ns1\tACGTAC\tTTGACA\ns2\tGGATCC\t-\n"
CONTAM_TEXT = ">c1 first record\nACGTACGTTAGCCGATAGGCTAACGTTAGC\n>c2\nTTGACCGGTAACGGTTAACCGGATCGATCG\n"
CONTAM_KEYS = "7ae75993b90f5d50"   # the fingerprint of the 16-mers of CONTAM_TEXT (rtx_screen_set_info), as the command line prints it into raxtax.json


@pytest.fixture(scope="module")
def cli():
    from raxtax_amd import _build
    exe = _build.build_cli()
    assert exe is not None and exe.exists()
    return exe


@pytest.fixture()
def files(tmp_path):
    """The small inputs of the option groups: a one-record FASTQ (and its reverse mates), a sample sheet, a contaminant FASTA."""
    d = tmp_path / "in"
    d.mkdir()
    for name, text in (("r1.fastq", FASTQ_TEXT), ("r2.fastq", FASTQ_TEXT), ("sheet.tsv", SHEET_TEXT), ("contam.fasta", CONTAM_TEXT)):
        (d / name).write_text(text)
    return d


def run(cli, *args):
    return subprocess.run([str(cli), *map(str, args)], capture_output=True, text=True, timeout=120)


def fingerprint(path):
    st = os.stat(path)
    return f"{os.path.realpath(path)}|{st.st_size}|{int(st.st_mtime)}"


def every_group(files, whole_run=True):
    """Every option group on (--chimera aside: it conflicts with --strand both); without the options of the whole run (--profile, --uniques,
    --otus) where a checkpoint with finished labels is to be resumed."""
    a = ["-i", files / "r1.fastq", "--tsv", "--strand", "both", "--identity"]
    if whole_run:
        a += ["--profile", "0.8"]
    a += ["--primers", "ACGT:TTGA", "--maxee", "1.5", "--minlen", "10", "--reverse", files / "r2.fastq", "--merge-qcap", "40", "--tags", files / "sheet.tsv",
          "--tag-mismatches", "1", "--contaminants", files / "contam.fasta"]
    if whole_run:
        a += ["--uniques", "--uniques-minsize", "2", "--otus"]
    return a


def chimera_group(files):
    return ["-i", files / "r1.fastq", "--chimera", "--primers", "ACGT:TTGA", "--truncq", "5"]


# ---- the checkpoint text, byte for byte

FIXED = '{{\n  "db_fingerprint": "{fp}",\n  "raw_confidence": {raw},\n  "skip_exact_matches": {skip},\n  "tsv": {tsv}'


def test_checkpoint_text_plain(cli, tmp_path):
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out)
    assert p.returncode == 0, p.stderr
    assert (out / "raxtax.json").read_text() == FIXED.format(fp=fingerprint(FASTA), raw="false", skip="false", tsv="false") + "\n}\n"
    assert (out / "diptera_subset.bin").exists() and not (out / "raxtax.out").exists() and not (out / "raxtax.ckp").exists()


def test_checkpoint_text_flags(cli, tmp_path):
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, "--skip-exact-matches", "--raw-confidence")
    assert p.returncode == 0, p.stderr
    assert (out / "raxtax.json").read_text() == FIXED.format(fp=fingerprint(FASTA), raw="true", skip="true", tsv="false") + "\n}\n"


def test_checkpoint_text_every_group(cli, tmp_path, files):
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *every_group(files))
    assert p.returncode == 0, p.stderr
    want = (FIXED.format(fp=fingerprint(FASTA), raw="false", skip="false", tsv="true")
            + ',\n  "strand": "both"'
            + ',\n  "hits": true'
            + ',\n  "identity": true'
            + ',\n  "profile": 80'
            + ',\n  "primers": "ACGT:TTGA;errors=10;window=0"'
            + ',\n  "quality": "maxee=1.5;minlen=10;ascii=33"'
            + f',\n  "merge": "reverse={files / "r2.fastq"};minovlen=16;maxdiffs=10;maxdiffpct=100;qcap=40;ascii=33"'
            + f',\n  "tags": "{fingerprint(files / "sheet.tsv")};mismatches=1;offset=0;both=0"'
            + f',\n  "contaminants": "file={files / "contam.fasta"};minhits=2;minpct=50;keys={CONTAM_KEYS}"'
            + ',\n  "uniques": "minsize=2 max_entries=0 max_bytes=0"'
            + ',\n  "otus": "minsize=1"'
            + "\n}\n")
    assert (out / "raxtax.json").read_text() == want
    # the set is built and described before the database is read
    assert re.search(r"\[INFO \] --contaminants: 2 record\(s\) of \S+contam\.fasta, \d+ distinct 16-mers in \d+ slots; a read is a contaminant from 2 hit\(s\) "
                     r"and 50 % of its windows on\n", p.stderr), p.stderr


def test_checkpoint_text_chimera(cli, tmp_path, files):
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *chimera_group(files))
    assert p.returncode == 0, p.stderr
    want = (FIXED.format(fp=fingerprint(FASTA), raw="false", skip="false", tsv="false")
            + ',\n  "primers": "ACGT:TTGA;errors=10;window=0"'
            + ',\n  "quality": "truncq=5;ascii=33"'
            + ',\n  "chimera": "segments=16;mindelta=24"'
            + "\n}\n")
    assert (out / "raxtax.json").read_text() == want


def test_checkpoint_text_settings_as_given(cli, tmp_path, files):
    """The settings of the groups as the run uses them: two primer pairs, --fastq-ascii in the quality and merge entries, the flipped sheet."""
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, "-i", files / "r1.fastq", "--hits", "--primers", "ACGT:", "--primers", ":TTGA", "--primer-errors", "20",
            "--primer-window", "40", "--fastq-ascii", "64", "--truncee", "0.5", "--maxns", "0", "-r", files / "r2.fastq", "--tags", files / "sheet.tsv",
            "--tag-offset", "2", "--chimera", "--chimera-segments", "8", "--chimera-mindelta", "30", "--contaminants", files / "contam.fasta",
            "--contam-minhits", "3", "--contam-minpct", "60", "--uniques", "--uniques-max-entries", "1000", "--uniques-max-bytes", "4096", "--otus",
            "--otus-minsize", "3")
    assert p.returncode == 0, p.stderr
    want = (FIXED.format(fp=fingerprint(FASTA), raw="false", skip="false", tsv="false")
            + ',\n  "hits": true'
            + ',\n  "primers": "ACGT:,:TTGA;errors=20;window=40"'
            + ',\n  "quality": "truncee=0.5;maxns=0;ascii=64"'
            + f',\n  "merge": "reverse={files / "r2.fastq"};minovlen=16;maxdiffs=10;maxdiffpct=100;qcap=41;ascii=64"'
            + ',\n  "chimera": "segments=8;mindelta=30"'
            + f',\n  "tags": "{fingerprint(files / "sheet.tsv")};mismatches=0;offset=2;both=0"'
            + f',\n  "contaminants": "file={files / "contam.fasta"};minhits=3;minpct=60;keys={CONTAM_KEYS}"'
            + ',\n  "uniques": "minsize=1 max_entries=1000 max_bytes=4096"'
            + ',\n  "otus": "minsize=3"'
            + "\n}\n")
    assert (out / "raxtax.json").read_text() == want


def test_only_db_log_lines(cli, tmp_path):
    """--device-format gives way to --derep and to --strand both with a line each; --timing prints the seconds of the two stages of an --only-db run."""
    p = run(cli, "-d", FASTA, "--only-db", "-o", tmp_path / "a", "--device-format", "--derep", "--strand", "both", "--timing")
    assert p.returncode == 0, p.stderr
    assert "[INFO ] --derep: the result lines are formatted on the host (--device-format has no effect)\n" in p.stderr
    assert "--strand both: the result lines are formatted on the host" not in p.stderr
    assert re.search(r'^\{"database": [-+.e\d]+, "database_cache": [-+.e\d]+\}$', p.stderr, re.M), p.stderr
    p = run(cli, "-d", FASTA, "--only-db", "-o", tmp_path / "b", "--device-format", "--strand", "both")
    assert "[INFO ] --strand both: the result lines are formatted on the host (--device-format has no effect)\n" in p.stderr


# ---- resume: the purge of every per-read report

REPORTS = {"raxtax.out": None, "raxtax.tsv": None, "raxtax.strand": None, "raxtax.hits": None,   # name under PREFIX: its header line or none
           "raxtax.trim": "label\tlength\tstart\tend\tprimer5\terrors5\tprimer3\terrors3",
           "raxtax.qc": "label\tlength\tstart\tend\texpected_errors\tverdict",
           "raxtax.merge": "label\tforward_length\treverse_length\toverlap\tdiffs\tmerged_length\tverdict",
           "raxtax.chimera": "label\tstatus\twindows\tsingle\tparent_id\tseg\tpos\tleft\ta_id\tright\tb_id\tdelta\tchimera\tparent\ta\tb",
           "raxtax.demux": "label\tsample\tverdict\ttag5\tmm5\toff5\ttag3\tmm3\toff3\tlo\thi",
           "raxtax.screen": "label\tlength\twindows\thits\tfirst\tsource\tverdict"}
EVERY_ON = {"raxtax.out", "raxtax.tsv", "raxtax.strand", "raxtax.hits", "raxtax.trim", "raxtax.qc", "raxtax.merge", "raxtax.demux", "raxtax.screen"}
CHIMERA_ON = {"raxtax.out", "raxtax.trim", "raxtax.qc", "raxtax.chimera"}


def interrupted(out):
    """A folder as a killed run leaves it: two finished labels, and in every report a finished line, an unfinished one, another finished one and a
    half-written last line."""
    (out / "raxtax.ckp").write_text("q1\nq2\n")
    for name, header in REPORTS.items():
        (out / name).write_text((header + "\n" if header else "") + "q1\t1\ta\nq3\t3\tc\nq2\t2\tb\nq4\t4")


@pytest.mark.parametrize("which", ["every", "chimera", "plain"])
def test_resume_purges_every_report_that_is_on(cli, tmp_path, files, which):
    args, on = {"every": (every_group(files, whole_run=False), EVERY_ON), "chimera": (chimera_group(files), CHIMERA_ON), "plain": ([], {"raxtax.out"})}[which]
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *args)
    assert p.returncode == 0 and "Restarting from checkpoint" not in p.stderr, p.stderr
    json_text = (out / "raxtax.json").read_text()
    interrupted(out)
    before = {name: (out / name).read_text() for name in REPORTS}
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *args)
    assert p.returncode == 0, p.stderr
    assert f"[INFO ] Restarting from checkpoint {out / 'raxtax.json'}\n" in p.stderr
    assert (out / "raxtax.json").read_text() == json_text and (out / "raxtax.ckp").read_text() == "q1\nq2\n"
    for name, header in REPORTS.items():
        if name in on:
            assert (out / name).read_text() == (header + "\n" if header else "") + "q1\t1\ta\nq2\t2\tb\n", name
        else:
            assert (out / name).read_text() == before[name], name
    assert not (out / "raxtax.out.tmp").exists()


def test_changed_option_starts_over(cli, tmp_path, files):
    out = tmp_path / "out"
    assert run(cli, "-d", FASTA, "--only-db", "-o", out, *chimera_group(files)).returncode == 0
    interrupted(out)
    before = {name: (out / name).read_text() for name in REPORTS}
    changed = chimera_group(files)[:-1] + ["6"]
    # the checkpoint no longer matches: nothing is resumed or purged, and the database cache of the first run stands in the way (without --redo)
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *changed)
    assert "Restarting from checkpoint" not in p.stderr
    assert p.returncode == 73 and "[ERROR] Output database file" in p.stderr, p.stderr
    assert {name: (out / name).read_text() for name in REPORTS} == before
    (out / "diptera_subset.bin").unlink()
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *changed)
    assert p.returncode == 0 and "Restarting from checkpoint" not in p.stderr, p.stderr
    assert '"quality": "truncq=6;ascii=33"' in (out / "raxtax.json").read_text()
    assert {name: (out / name).read_text() for name in REPORTS} == before
    # ... and --redo ignores a checkpoint that matches
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, "--redo", *changed)
    assert p.returncode == 0 and "Restarting from checkpoint" not in p.stderr, p.stderr
    assert {name: (out / name).read_text() for name in REPORTS} == before


@pytest.mark.parametrize("option, what", [(["--profile", "0.8"], "the profile would miss them"), (["--uniques"], "the table would miss them")])
def test_whole_run_options_refuse_finished_labels(cli, tmp_path, option, what):
    out = tmp_path / "out"
    assert run(cli, "-d", FASTA, "--only-db", "-o", out, *option).returncode == 0
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *option)   # no label finished yet: resumes
    assert p.returncode == 0 and "Restarting from checkpoint" in p.stderr, p.stderr
    interrupted(out)
    before = (out / "raxtax.out").read_text()
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, *option)
    assert p.returncode == 64, p.stderr
    assert f"raxtax-hip: {option[0]} cannot resume a checkpoint with processed queries (2 in {out / 'raxtax.ckp'}): {what}; run with --redo" in p.stderr
    assert "Restarting from checkpoint" not in p.stderr and (out / "raxtax.out").read_text() == before


# ---- refusals: exit code, message, no output folder

RANGE = "raxtax-hip: {} takes a whole number, {} .. {}, not '{}'\n"
REAL = "raxtax-hip: {} takes a number that is not negative, not '{}'\n"
POSITIVE = "raxtax-hip: {} takes a positive integer\n"
FQ, FA = "FQ", "FA"   # the -i of the case: the one-record FASTQ or the FASTA of the database
REFUSALS = [
    # the options with a message of their own
    (FA, ["--strand", "sideways"], 64, "raxtax-hip: --strand takes plus or both\n"),
    (FA, ["--primers", "ACGT"], 64, "raxtax-hip: --primers takes FWD:REV (either side may be empty), not 'ACGT'\n"),
    (FA, ["--primer-errors", "100"], 64, "raxtax-hip: --primer-errors takes a percentage, 0 .. 99\n"),
    (FA, ["--primer-window", "257"], 64, "raxtax-hip: --primer-window takes 1 .. 256 bases\n"),
    (FQ, ["--fastq-ascii", "50"], 64, "raxtax-hip: --fastq-ascii takes 33 or 64, not '50'\n"),
    (FA, ["--profile", "1.5"], 64, "raxtax-hip: --profile takes a confidence cutoff in (0, 1], such as 0.8\n"),
    (FA, ["--profile", "0.8x"], 64, "raxtax-hip: --profile takes a confidence cutoff in (0, 1], such as 0.8\n"),
    (FA, ["--no-such-option"], 64, "usage: raxtax-hip -d DB.(fasta|bin) [-i QUERIES.(fasta|fastq)] [-o PREFIX]"),
    # whole numbers in a range: the quality group (name=value in the checkpoint) ...
    (FQ, ["--truncq", "94"], 64, RANGE.format("--truncq", 0, 93, "94")),
    (FQ, ["--truncq", "5x"], 64, RANGE.format("--truncq", 0, 93, "5x")),
    (FQ, ["--maxns", "-1"], 64, RANGE.format("--maxns", 0, 1048576, "-1")),
    (FQ, ["--trunclen", "0"], 64, RANGE.format("--trunclen", 1, 1048576, "0")),
    (FQ, ["--minlen", "1048577"], 64, RANGE.format("--minlen", 1, 1048576, "1048577")),
    (FQ, ["--maxlen", "long"], 64, RANGE.format("--maxlen", 1, 1048576, "long")),
    # ... and the groups that record the names of their options
    (FQ, ["--merge-minovlen", "0"], 64, RANGE.format("--merge-minovlen", 1, 1024, "0")),
    (FQ, ["--merge-maxdiffs", "1025"], 64, RANGE.format("--merge-maxdiffs", 0, 1024, "1025")),
    (FQ, ["--merge-maxdiffpct", "101"], 64, RANGE.format("--merge-maxdiffpct", 0, 100, "101")),
    (FQ, ["--merge-qcap", "94"], 64, RANGE.format("--merge-qcap", 0, 93, "94")),
    (FQ, ["--merge-qcap", "4 0"], 64, RANGE.format("--merge-qcap", 0, 93, "4 0")),
    (FA, ["--chimera-segments", "1"], 64, RANGE.format("--chimera-segments", 2, 32, "1")),
    (FA, ["--chimera-mindelta", "4097"], 64, RANGE.format("--chimera-mindelta", 0, 4096, "4097")),
    (FA, ["--chimera", "--chimera-mindelta"], 64, RANGE.format("--chimera-mindelta", 0, 4096, "")),   # the value is missing
    (FA, ["--contam-minhits", "0"], 64, RANGE.format("--contam-minhits", 1, 2147483647, "0")),
    (FA, ["--contam-minpct", "101"], 64, RANGE.format("--contam-minpct", 0, 100, "101")),
    (FA, ["--contam-minpct", "half"], 64, RANGE.format("--contam-minpct", 0, 100, "half")),
    (FA, ["--tag-mismatches", "9"], 64, RANGE.format("--tag-mismatches", 0, 8, "9")),
    (FA, ["--tag-offset", "16"], 64, RANGE.format("--tag-offset", 0, 15, "16")),
    (FA, ["--tag-offset", "x"], 64, RANGE.format("--tag-offset", 0, 15, "x")),
    # numbers that are not negative
    (FQ, ["--maxee", "-1"], 64, REAL.format("--maxee", "-1")),
    (FQ, ["--maxee", "abc"], 64, REAL.format("--maxee", "abc")),
    (FQ, ["--truncee", "1.5e"], 64, REAL.format("--truncee", "1.5e")),
    (FQ, ["--maxee-rate", "nan"], 64, REAL.format("--maxee-rate", "nan")),
    # positive integers
    (FA, ["--uniques", "--uniques-minsize", "0"], 64, POSITIVE.format("--uniques-minsize")),
    (FA, ["--uniques", "--uniques-minsize", "two"], 64, POSITIVE.format("--uniques-minsize")),
    (FA, ["--uniques", "--uniques-max-entries", "2147483647"], 64, POSITIVE.format("--uniques-max-entries")),
    (FA, ["--uniques", "--uniques-max-bytes", "1k"], 64, POSITIVE.format("--uniques-max-bytes")),
    (FA, ["--uniques", "--otus", "--otus-minsize", "0"], 64, POSITIVE.format("--otus-minsize")),
    (FA, ["--uniques", "--otus", "--otus-minsize", "2.5"], 64, POSITIVE.format("--otus-minsize")),
    # an option of a group without the option that turns the group on
    (FQ, ["--merge-qcap", "40", "--merge-maxdiffs", "5"], 64, "raxtax-hip: --merge-qcap --merge-maxdiffs sets how pairs are merged and needs --reverse FILE (the reverse mates)\n"),
    (FA, ["--chimera-mindelta", "3"], 64, "raxtax-hip: --chimera-mindelta sets how reads are checked for chimeras and needs --chimera\n"),
    (FA, ["--tag-offset", "1", "--tags-both-orientations"], 64, "raxtax-hip: --tag-offset --tags-both-orientations sets how reads are assigned to samples and needs --tags SHEET\n"),
    (FA, ["--contam-minhits", "3"], 64, "raxtax-hip: --contam-minhits sets how reads are screened and needs --contaminants FILE\n"),
    (FA, ["--uniques-minsize", "2", "--uniques-max-bytes", "9"], 64, "raxtax-hip: --uniques-minsize --uniques-max-bytes sets how the distinct reads are kept and written and needs --uniques\n"),
    (FA, ["--uniques", "--otus-minsize", "2"], 64, "raxtax-hip: --otus-minsize sets what is written of the OTUs and needs --otus\n"),
    (FA, ["--otus"], 64, "raxtax-hip: --otus clusters the distinct reads of the run and needs --uniques\n"),
    # options that cannot go together, or not with this input
    (FA, ["--chimera", "--strand", "both"], 64, "raxtax-hip: --chimera checks a read in the orientation given and cannot go with --strand both\n"),
    (FA, ["--maxee", "1", "--minlen", "5"], 64, "raxtax-hip: the quality filter (maxee=1;minlen=5) needs FASTQ input: {FA} does not start with '@'\n"),
    (FA, ["--reverse", "{FQ}"], 64, "raxtax-hip: --reverse needs FASTQ input: {FA} does not start with '@'\n"),
    (FA, ["--tags", "{SHEET}", "--derep", "--profile", "0.8"], 64, "raxtax-hip: --tags cannot go with --derep and --profile together: copies from different samples would be counted as one read\n"),
    # oligos and files
    (FA, ["--primers", "ACXT:TTGA"], 64, "raxtax-hip: --primers: 'X' in primer ACXT is no IUPAC code\n"),
    (FA, ["--primers", "ACGT:" + "A" * 65], 64, "raxtax-hip: --primers: primer " + "A" * 65 + " has 65 bases (at most 64)\n"),
    (FA, ["--strand", "both", "--primers", "ACGT:TTGA", "--primers", "GGCC:AATT", "--primers", "CCGG:TTAA"], 64,
     "raxtax-hip: --primers: CCGG:TTAA makes 12 patterns (at most 8; --strand both registers every oligo at both ends)\n"),
    (FA, ["--tags", "{BAD_SHEET}"], 64, "raxtax-hip: --tags: {BAD_SHEET} line 2: 'X' is no IUPAC code\n"),
    (FA, ["--tags", "{SHORT_SHEET}"], 64, "raxtax-hip: --tags: {SHORT_SHEET} line 1: expected sample<TAB>fwd_tag<TAB>rev_tag\n"),
    (FA, ["--tags", "{SHEET}", "--tags-both-orientations"], 64, "raxtax-hip: --tags: {SHEET} line 3: --tags-both-orientations needs a rev_tag\n"),
    (FA, ["--tags", "{MISSING}"], 66, "raxtax-hip: --tags: cannot read {MISSING}\n"),
    (FA, ["--contaminants", "{MISSING}"], 66, "raxtax-hip: --contaminants: cannot read {MISSING}\n"),
    # the run itself
    (FA, ["--gpus", "0"], 64, "raxtax-hip: --gpus / --devices need at least one device\n"),
    (FA, ["--devices", ","], 64, "raxtax-hip: --gpus / --devices need at least one device\n"),
    (FA, ["--only-db", "--skip-db"], 64, "raxtax-hip: -d is required, -i unless --only-db; --only-db conflicts with --skip-db\n"),
    # two mistakes at once: the one that is looked at first is the one reported
    (FQ, ["--merge-qcap", "40", "--chimera", "--strand", "both"], 64, "sets how pairs are merged and needs --reverse FILE"),
    (FA, ["--chimera-mindelta", "3", "--primers", "ACXT:"], 64, "sets how reads are checked for chimeras and needs --chimera\n"),
    (FA, ["--tag-offset", "1", "--primers", "ACXT:"], 64, "raxtax-hip: --primers: 'X' in primer ACXT is no IUPAC code\n"),
    (FA, ["--contam-minhits", "3", "--tags", "{MISSING}"], 66, "raxtax-hip: --tags: cannot read {MISSING}\n"),
    (FA, ["--uniques-minsize", "2", "--contaminants", "{MISSING}"], 66, "raxtax-hip: --contaminants: cannot read {MISSING}\n"),
    (FA, ["--uniques-minsize", "2", "--otus-minsize", "2"], 64, "and needs --uniques\n"),
    (FA, ["--otus", "--otus-minsize", "2"], 64, "raxtax-hip: --otus clusters the distinct reads of the run and needs --uniques\n"),
    (FA, ["--maxee", "1", "--strand", "sideways"], 64, "raxtax-hip: --strand takes plus or both\n"),
    (FA, ["--maxee", "1", "--gpus", "0"], 64, "raxtax-hip: --gpus / --devices need at least one device\n"),
]


@pytest.mark.parametrize("kind, args, code, message", REFUSALS, ids=[" ".join(r[1]) for r in REFUSALS])
def test_refusals(cli, tmp_path, files, kind, args, code, message):
    (files / "bad_sheet.tsv").write_text("s1\tACGTAC\tTTGACA\ns2\tGGAXCC\n")
    (files / "short_sheet.tsv").write_text("s1\n")
    names = {"FA": str(FASTA), "FQ": str(files / "r1.fastq"), "SHEET": str(files / "sheet.tsv"), "BAD_SHEET": str(files / "bad_sheet.tsv"),
             "SHORT_SHEET": str(files / "short_sheet.tsv"), "MISSING": str(files / "no_such_file")}
    out = tmp_path / "out"
    p = run(cli, "-d", FASTA, "-i", names[kind], "-o", out, *[a.format(**names) for a in args])
    assert p.returncode == code, p.stderr
    assert message.format(**names) in p.stderr, p.stderr
    assert p.stderr.count("raxtax-hip: ") <= 1 and "[ERROR]" not in p.stderr, p.stderr   # one refusal, and nothing behind it
    assert not out.exists()


def test_refusals_of_the_run(cli, tmp_path):
    out = tmp_path / "out"
    p = run(cli, "-i", FASTA, "-o", out)
    assert p.returncode == 64 and "raxtax-hip: -d is required, -i unless --only-db; --only-db conflicts with --skip-db\n" in p.stderr and not out.exists()
    p = run(cli, "-d", FASTA, "-o", out)
    assert p.returncode == 64 and "raxtax-hip: -d is required, -i unless --only-db" in p.stderr and not out.exists()
    # an existing folder without a checkpoint is refused without --redo (io.rs:241-243) and taken with it
    out.mkdir()
    p = run(cli, "-d", FASTA, "--only-db", "-o", out)
    assert p.returncode == 73, p.stderr
    assert f"[ERROR] Output folder {out} already exists! Please specify another folder with -o <PATH> or run with --redo to force overriding existing files!\n" in p.stderr
    assert list(out.iterdir()) == []
    p = run(cli, "-d", FASTA, "--only-db", "-o", out, "--redo")
    assert p.returncode == 0 and (out / "raxtax.json").exists() and (out / "diptera_subset.bin").exists(), p.stderr
    # a database that cannot be parsed: exit 66, the folder is there by then
    bad = tmp_path / "bad.fasta"
    bad.write_text("no fasta\n")
    p = run(cli, "-d", bad, "--only-db", "-o", tmp_path / "out2")
    assert p.returncode == 66 and f"[ERROR] Failed to parse {bad}: " in p.stderr, p.stderr

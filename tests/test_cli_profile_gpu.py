"""raxtax-hip --profile CUTOFF (cli_main.cpp): PREFIX/raxtax.profile is the report of the taxon profile of the whole run (rtx_profile_format over
the sum of the handles' profiles) -- byte for byte what rx.profile_text gives for a Python run of the same inputs; the result files are
what they are without the option; the cutoff takes part in the checkpoint, and a run that would resume a checkpoint with processed
queries is refused, because its profile would miss them."""
import shutil
import subprocess
from pathlib import Path

import pytest

import raxtax_amd as rx

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
    """The first 600 records as they are, and with every third one reverse-complemented."""
    d = tmp_path_factory.mktemp("profile_queries")
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


def _python_report(path, strand, skip):
    tree = rx.parse_reference_fasta_str(DB.read_text())
    queries = rx.parse_query_fasta_str(path.read_text())
    index = rx.Index(tree, strand=strand)
    index.profile_begin(0.8, skip_exact_matches=skip)
    rx.raxtax(queries, index, skip, False, 128, lambda *a: None, False)
    prof = index.profile_read()
    assert int(prof.totals[0]) == len(queries) == 600 and int(prof.totals[1]) > 300
    return rx.profile_text(tree, prof)


@pytest.mark.parametrize("strand, skip", [("plus", False), ("both", True)])
def test_the_report_is_the_python_run_s(tmp_path, files, strand, skip):
    path = files[0] if strand == "plus" else files[1]
    extra = (["--strand", "both"] if strand == "both" else []) + (["--skip-exact-matches"] if skip else [])
    a, b = tmp_path / "profile", tmp_path / "none"
    run("-d", DB, "-i", path, "-o", a, "--skip-db", "--batch", 128, "--profile", 0.8, *extra)
    run("-d", DB, "-i", path, "-o", b, "--skip-db", "--batch", 128, *extra)
    want = _python_report(path, strand, skip)
    got = (a / "raxtax.profile").read_text()
    assert got == want
    lines = got.splitlines()
    assert lines[0].startswith("# cutoff=0.80\tqueries=600\t") and lines[1].startswith("clade\tdirect\t") and len(lines) > 10
    # without the option: no file, no word of it in the checkpoint; the result files are the same
    assert not (b / "raxtax.profile").exists() and "profile" not in (b / "raxtax.json").read_text()
    assert '"profile": 80' in (a / "raxtax.json").read_text()
    for f in ("raxtax.out", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    if strand == "plus":   # two handles on the device, the lines formatted on the device: the same report
        c = tmp_path / "two"
        run("-d", DB, "-i", path, "-o", c, "--skip-db", "--batch", 128, "--profile", "0.80", "--devices", "0,0", "--device-format")
        assert (c / "raxtax.profile").read_text() == want and (c / "raxtax.out").read_bytes() == (a / "raxtax.out").read_bytes()


def test_a_resumed_run_is_refused_and_redo_runs(tmp_path, files):
    plain, _ = files
    full = tmp_path / "full"
    run("-d", DB, "-i", plain, "-o", full, "--skip-db", "--batch", 128, "--profile", 0.8)
    want = (full / "raxtax.profile").read_text()
    ckp = (full / "raxtax.ckp").read_text().splitlines()
    part = tmp_path / "part"
    shutil.copytree(full, part)
    (part / "raxtax.ckp").write_text("\n".join(ckp[:250]) + "\n")
    out_before = (part / "raxtax.out").read_bytes()
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--profile", 0.8, ok=False)
    assert p.returncode == 64 and "--redo" in p.stderr and "--profile" in p.stderr, (p.returncode, p.stderr)
    assert (part / "raxtax.out").read_bytes() == out_before    # (refused before anything was touched)
    run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--profile", 0.8, "--redo")
    assert (part / "raxtax.profile").read_text() == want and (part / "raxtax.out").read_bytes() == (full / "raxtax.out").read_bytes()
    # another cutoff is another checkpoint: the run starts over instead of resuming
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--profile", 0.5)
    assert "Restarting from checkpoint" not in p.stderr and (part / "raxtax.profile").read_text().startswith("# cutoff=0.50\t")
    for bad in ("0", "1.5", "abc"):
        assert run("-d", DB, "-i", plain, "-o", tmp_path / "bad", "--profile", bad, ok=False).returncode == 64

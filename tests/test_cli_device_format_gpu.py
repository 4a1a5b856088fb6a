"""raxtax-hip --device-format (RTX_OPT_DEVICE_TEXT on every handle): the output files are byte for byte those of a run without it, with and
without --tsv, and a run resumed from a checkpoint (a half-written line of an unfinished query in the output) ends with the same files."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FASTA = ROOT / "tests" / "golden" / "diptera_subset.fasta"
CLI = ROOT / "raxtax_amd" / "raxtax-hip"

pytestmark = pytest.mark.gpu


def run(*args):
    p = subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


@pytest.mark.parametrize("tsv", [False, True])
def test_device_format_writes_the_same_files(tmp_path, tsv):
    extra = ["--tsv"] if tsv else []
    run("-d", FASTA, "-i", FASTA, "-o", tmp_path / "host", "--batch", 128, *extra)
    run("-d", FASTA, "-i", FASTA, "-o", tmp_path / "dev", "--batch", 128, "--device-format", *extra)
    names = ["raxtax.out", "raxtax.ckp"] + (["raxtax.tsv"] if tsv else [])
    for n in names:
        assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n
    assert (tmp_path / "dev" / "raxtax.tsv").exists() == tsv


def test_device_format_resumes(tmp_path):
    out = tmp_path / "full"
    run("-d", FASTA, "-i", FASTA, "-o", out, "--tsv", "--batch", 128)
    lines = (out / "raxtax.out").read_text().splitlines()
    tsv_lines = (out / "raxtax.tsv").read_text().splitlines()
    labels = (out / "raxtax.ckp").read_text().splitlines()
    out2 = tmp_path / "resumed"
    shutil.copytree(out, out2)
    done = set(labels[:250])
    (out2 / "raxtax.ckp").write_text("\n".join(labels[:250]) + "\n")
    keep = [l for l in lines if l.split("\t")[0] in done]
    (out2 / "raxtax.out").write_text("\n".join(keep) + "\n" + lines[-1][: len(lines[-1]) // 2] + "\n")
    (out2 / "raxtax.tsv").write_text("\n".join(l for l in tsv_lines if l.split("\t")[0] in done) + "\n")
    p = run("-d", FASTA, "-i", FASTA, "-o", out2, "--tsv", "--batch", 128, "--device-format")
    assert "Restarting from checkpoint" in p.stderr
    assert sorted((out2 / "raxtax.out").read_text().splitlines()) == sorted(lines)
    assert sorted((out2 / "raxtax.tsv").read_text().splitlines()) == sorted(tsv_lines)
    assert sorted((out2 / "raxtax.ckp").read_text().splitlines()) == sorted(labels)

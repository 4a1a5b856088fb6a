"""raxtax-hip --identity (cli_main.cpp, RTX_OPT_IDENTITY): PREFIX/raxtax.hits carries two more columns at the end of every line -- the
semi-global edit distance of the query to the reference the line names, and the identity in percent with two decimals (`-` twice where
there is no distance).  The first seven columns are those of --hits alone; the two new ones are held against rx.semiglobal_distance and
the integer formula on the named reference's bytes; --hits alone writes what it always wrote (the expectations of test_cli_hits_gpu.py);
the flag takes part in the checkpoint and in resume."""
import shutil

import numpy as np
import pytest

import raxtax_amd as rx
from test_cli_hits_gpu import DB, _COMP, expected, files, run  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sequences(oracle, files):
    """label -> bases of every query; reference id -> bases of every reference (ids are the order of the tree's lineages)."""
    plain, _ = files
    otree = oracle.parse_reference_fasta_str(DB.read_text())
    records = oracle.parse_query_fasta_str(DB.read_text())      # the references as they stand in the file ...
    orig = otree.original_index()                               # ... which reference id r is record orig[r] of
    refs = [np.asarray(records[int(orig[r])][1], np.uint8) for r in range(otree.num_tips)]
    for r in range(0, otree.num_tips, 41):
        assert r in otree.exact_matches(refs[r])
    queries = {label: np.asarray(seq, np.uint8) for label, seq in oracle.parse_query_fasta_str(plain.read_text())}
    return queries, refs


def _columns(seq, ref):
    d = rx.semiglobal_distance(seq, ref)
    h = ((len(seq) - d) * 10000 + len(seq) // 2) // len(seq)
    return [str(d), f"{h // 100}.{h % 100:02d}"]


def test_two_more_columns(tmp_path, files, sequences, expected):
    plain, mixed = files
    queries, refs = sequences
    want, _ = expected[False]
    a, b = tmp_path / "identity", tmp_path / "hits"
    run("-d", DB, "-i", plain, "-o", a, "--skip-db", "--tsv", "--batch", 128, "--identity")
    run("-d", DB, "-i", plain, "-o", b, "--skip-db", "--tsv", "--batch", 128, "--hits")
    # --hits alone: the file and the checkpoint of before (every line against the oracle, as test_cli_hits_gpu.py holds it)
    hits = [l.split("\t") for l in (b / "raxtax.hits").read_text().splitlines()]
    by_label = {w[0]: w for w in want}
    assert len(hits) > 500 and all(len(l) == 7 and l == [by_label[l[0]][0], "+", *by_label[l[0]][1:]] for l in hits)
    ckp_hits, ckp_id = (b / "raxtax.json").read_text(), (a / "raxtax.json").read_text()
    assert "identity" not in ckp_hits and ckp_hits.endswith(',\n  "hits": true\n}\n')
    assert ckp_id == ckp_hits.replace(',\n  "hits": true\n}\n', ',\n  "hits": true,\n  "identity": true\n}\n')
    for f in ("raxtax.out", "raxtax.tsv", "raxtax.ckp"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # --identity: the same seven columns, then dist and identity of the query against the named reference
    lines = [l.split("\t") for l in (a / "raxtax.hits").read_text().splitlines()]
    assert [l[:7] for l in lines] == hits and all(len(l) == 9 for l in lines)
    n_dash = 0
    for l in lines:
        if l[5] == "-":
            assert l[7:] == ["-", "-"], l
            n_dash += 1
        else:
            assert l[7:] == _columns(queries[l[0]], refs[int(l[5])]), l
    dists = [int(l[7]) for l in lines if l[7] != "-"]
    print(f"{len(lines)} lines, {n_dash} without a distance; distances: min {min(dists)}, median {int(np.median(dists))}, max {max(dists)}")
    # --skip-exact-matches: the nearest reference is no copy of the query any more, and the distances are those to whatever it names
    e = tmp_path / "skip"
    run("-d", DB, "-i", plain, "-o", e, "--skip-db", "--batch", 128, "--identity", "--skip-exact-matches")
    want_skip = {w[0]: w for w in expected[True][0]}
    skipped = [l.split("\t") for l in (e / "raxtax.hits").read_text().splitlines()]
    assert len(skipped) > 500
    for l in skipped:
        w = want_skip[l[0]]
        assert l[:7] == [w[0], "+", *w[1:]], (l, w)
        assert l[7:] == (["-", "-"] if l[5] == "-" else _columns(queries[l[0]], refs[int(l[5])])), l
    d_skip = [int(l[7]) for l in skipped if l[7] != "-"]
    print(f"skip: {len(skipped)} lines; distances: min {min(d_skip)}, median {int(np.median(d_skip))}, max {max(d_skip)}")
    assert max(d_skip) > 0
    # --strand both on the flipped records: the distance is that of the orientation that was classified -- the same figures
    c = tmp_path / "both"
    run("-d", DB, "-i", mixed, "-o", c, "--skip-db", "--batch", 128, "--identity", "--strand", "both")
    both = [l.split("\t") for l in (c / "raxtax.hits").read_text().splitlines()]
    assert [l[:1] + l[2:] for l in both] == [l[:1] + l[2:] for l in lines]
    assert sum(l[1] == "-" for l in both) >= len(both) // 3 - 1


def test_resume_and_the_flag_in_the_checkpoint(tmp_path, files):
    plain, _ = files
    full = tmp_path / "full"
    run("-d", DB, "-i", plain, "-o", full, "--skip-db", "--batch", 128, "--identity")
    want = {f: (full / f).read_text().splitlines() for f in ("raxtax.out", "raxtax.hits", "raxtax.ckp")}
    assert len(want["raxtax.hits"]) == len(want["raxtax.ckp"]) > 500 and all(l.count("\t") == 8 for l in want["raxtax.hits"])
    # interrupted: 250 queries finished, every output cut in the middle of a line of an unfinished query
    part = tmp_path / "part"
    shutil.copytree(full, part)
    done = set(want["raxtax.ckp"][:250])
    (part / "raxtax.ckp").write_text("\n".join(want["raxtax.ckp"][:250]) + "\n")
    for f in ("raxtax.out", "raxtax.hits"):
        keep = [l for l in want[f] if l.split("\t")[0] in done]
        nxt = next(l for l in want[f] if l.split("\t")[0] not in done)
        (part / f).write_text("\n".join(keep) + "\n" + nxt[: max(len(nxt) // 2, nxt.index("\t") + 2)])
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--identity")
    assert "Restarting from checkpoint" in p.stderr
    for f, lines in want.items():
        assert sorted((part / f).read_text().splitlines()) == sorted(lines), f
    # with --hits alone the checkpoint does not apply: the run starts over and writes the file of seven columns
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--hits")
    assert "Restarting from checkpoint" not in p.stderr
    assert "identity" not in (part / "raxtax.json").read_text()
    assert (part / "raxtax.hits").read_text().splitlines() == ["\t".join(l.split("\t")[:7]) for l in want["raxtax.hits"]]
    assert (part / "raxtax.out").read_text().splitlines() == want["raxtax.out"]
    p = run("-d", DB, "-i", plain, "-o", part, "--skip-db", "--batch", 128, "--identity")
    assert "Restarting from checkpoint" not in p.stderr
    for f, lines in want.items():
        assert (part / f).read_text().splitlines() == lines, f

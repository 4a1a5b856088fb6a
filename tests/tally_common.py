"""What the tests of the distinct-read table share: the expected table as a Python dict over bytes(seq), and the reads at the word and
nibble edges (the lengths of test_gpu_derep.py)."""
import numpy as np

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 658)


def concat(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    flat = np.concatenate([np.asarray(s, np.uint8) for s in seqs] + [np.zeros(0, np.uint8)])
    return flat, off


def expected_table(seqs, sample=None, weight=None, columns=1):
    """{bytes(seq): counts per column} of the reads that count: weight above 0 (None: 1), length above 0.  Insertion order = first appearance."""
    table = {}
    for q, s in enumerate(seqs):
        w = 1 if weight is None else int(weight[q])
        if w == 0 or len(s) == 0:
            continue
        row = table.setdefault(bytes(np.asarray(s, np.uint8)), [0] * columns)
        row[0 if sample is None else int(sample[q])] += w
    return {k: tuple(v) for k, v in table.items()}


def random_seq(rng, n):
    return (1 << rng.integers(0, 4, n)).astype(np.uint8)


def edge_reads(seed=41):
    """(distinct, picks): 40 distinct sequences of the edge lengths -- prefix pairs, pairs that differ in the first or only in the last base,
    an ambiguity code against a plain base -- and about 330 picks of them in which every sequence occurs, several reads are empty and copies
    start on even and on odd nibbles."""
    rng = np.random.default_rng(seed)
    base = {n: random_seq(rng, n) for n in LENGTHS}
    base[65][5] = 2
    for short, long in ((8, 9), (16, 17), (512, 513)):   # one sequence a prefix of another
        base[short] = base[long][:short].copy()
    distinct = [base[n] for n in LENGTHS]
    for n in (1, 9, 17, 65, 513, 658):   # pairs that differ only in the first base, and only in the last
        first, last = base[n].copy(), base[n].copy()
        first[0] = 1 if first[0] != 1 else 2
        last[-1] = 4 if last[-1] != 4 else 8
        distinct += [first] + ([last] if n > 1 else [])
    plain, amb = base[65].copy(), base[65].copy()   # an ambiguity code against a plain base
    plain[5], amb[5] = 1, 15
    distinct += [plain, amb]
    distinct += [random_seq(rng, 658) for _ in range(40 - len(distinct))]
    assert len({bytes(s) for s in distinct}) == len(distinct) == 40
    picks = list(rng.integers(0, len(distinct), 286))
    picks += [0, 0, 0, 0] + list(range(len(distinct)))        # several empty reads; every sequence at least once
    picks = [int(x) for x in rng.permutation(picks)]
    seqs = [distinct[i] for i in picks]
    _, off = concat(seqs)
    dup = np.array([picks.index(p) != i for i, p in enumerate(picks)])
    starts = off[:-1].astype(np.int64)
    assert (starts[dup] % 2 == 0).any() and (starts[dup] % 2 == 1).any()   # copies start on even and on odd nibbles
    assert sum(len(s) == 0 for s in seqs) >= 4 and len(seqs) == 330
    return distinct, picks

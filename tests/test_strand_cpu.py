"""rtx_revcomp, the host form of the reverse complement of both-strand mode (RTX_OPT_STRAND), against numpy: reversed, the four bits of
every one-hot code reversed (A=1 <-> T=8, C=2 <-> G=4, ambiguity codes to their complements, N stays), a byte above 15 as it is."""
import numpy as np

import raxtax_amd as rx
from raxtax_amd.api import revcomp


def _numpy_revcomp(seq):
    comp = np.arange(256, dtype=np.uint8)
    for b in range(16):
        comp[b] = ((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3)
    return comp[np.asarray(seq, dtype=np.uint8)[::-1]]


def test_all_sixteen_codes():
    codes = np.arange(16, dtype=np.uint8)
    got = revcomp(codes)
    assert np.array_equal(got, _numpy_revcomp(codes))
    named = dict(A=1, C=2, G=4, T=8, N=15, R=5, Y=10, S=6, W=9, K=12, M=3)
    comp = {int(c): int(g) for c, g in zip(codes[::-1], got)}
    for a, b in (("A", "T"), ("C", "G"), ("R", "Y"), ("K", "M"), ("S", "S"), ("W", "W"), ("N", "N")):
        assert comp[named[a]] == named[b] and comp[named[b]] == named[a]
    assert comp[0] == 0


def test_bytes_above_fifteen_stay():
    seq = np.array([1, 16, 2, 0x20, 255, 8, 77], dtype=np.uint8)
    assert revcomp(seq).tolist() == [77, 1, 255, 0x20, 4, 16, 8]
    assert np.array_equal(revcomp(np.arange(256, dtype=np.uint8))[:240], np.arange(255, 15, -1, dtype=np.uint8))


def test_odd_and_even_lengths_and_involution():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 7, 8, 9, 16, 657, 658, 4097):
        seq = rng.integers(0, 16, n).astype(np.uint8)
        got = revcomp(seq)
        assert np.array_equal(got, _numpy_revcomp(seq)), n
        assert np.array_equal(revcomp(got), seq), n
    palin = np.tile(np.array([1, 2, 4, 8], np.uint8), 4)
    assert np.array_equal(revcomp(palin), palin)


def test_new_exports_are_bound():
    lib = rx._lib.load()
    for name in ("rtx_batch_strands", "rtx_revcomp", "rtx_raxtax_multi_ex"):
        assert name in rx._lib._SIGNATURES and hasattr(lib, name)

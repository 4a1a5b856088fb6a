"""The nearest reference of a query (RTX_OPT_NEAREST, rtx_nearest.hip) without a GPU: the additions to the C ABI, and the position
arithmetic of nearest_kernel's scan of one tile (rtx_math.hpp: packed_count_pos, nearest_lane_base, nearest_match16 / nearest_match8) run
through the x86 emulator on tiles packed by numpy.

The packing is the one hit_count's dense epilogues store (rtx_math.hpp, ref_slot): group g of lane l of a tile of L lanes holds the
references (g L + l) 8 + [0, 8) and goes to offset (g L + l) 8 of the tile's stretch -- low byte per reference, the two high bits of the
eight references of a chunk in one u16 at index g L + l, reference j of the chunk at bits 2 j.  The test packs group by group and lane by
lane from that rule (full tile: L = 64; the last tile of 848 references: L = 7) and expects the lowest reference that holds the peak."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx

ROOT = Path(__file__).resolve().parent.parent
NONE = 0xFFFFFFFF


def test_the_header_declares_and_the_library_exports_the_additions():
    header = (ROOT / "include" / "raxtax_hip.h").read_text()
    assert re.search(r"#define\s+RTX_OPT_NEAREST\s+26\b", header)
    assert re.search(r"#define\s+RTX_NO_REF\s+0xFFFFFFFFu\b", header)
    assert re.search(r"#define\s+RTX_ABI_VERSION\s+6\b", header)
    assert re.search(r"\bint\s+rtx_batch_nearest\s*\(\s*rtx_index\s*\*\s*\w*\s*,\s*const\s+uint32_t\s*\*\*\s*nearest\s*,\s*const\s+uint32_t\s*\*\*\s*ties\s*\)", header)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*rtx_query_hit_fn\s*\)", header)
    assert re.search(r"\bint\s+rtx_raxtax_multi_ex2\s*\(", header)
    lib = rx._lib.load()
    for name in ("rtx_batch_nearest", "rtx_raxtax_multi_ex2", "rtx_batch_nearest_time"):
        assert name in rx._lib._SIGNATURES and hasattr(lib, name), name
    assert hasattr(lib, "rtx_raxtax_multi_ex")   # stays
    assert rx.NO_REF == NONE


def _pack_tile(counts, L):
    """Low bytes and high-bit words of one tile of L lanes as the dense epilogue stores them: walked as the kernel does, group by group, lane by lane."""
    n = L * 128
    c = np.zeros(n, np.uint32)
    c[:len(counts)] = counts
    lo = np.zeros(n, np.uint8)
    hi = np.zeros(n // 8, np.uint16)
    for g in range(16):
        for lane in range(L):
            first = (g * L + lane) * 8                 # the group's references, and where its eight low bytes go
            word = 0
            for j in range(8):
                lo[first + j] = c[first + j] & 0xFF
                word |= int(c[first + j] >> 8) << (2 * j)
            hi[g * L + lane] = word                    # chunk order
    return lo, hi


def _scan(emul, lo, hi, in_tile, peak, packed):
    emul.emul_nearest_scan.restype = C.c_uint32
    # (the kernel's 16-byte loads stay inside the row: rows are padded to whole lanes of 128 references -- the arrays here are as long)
    return emul.emul_nearest_scan(lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p) if hi is not None else None, C.c_uint32(in_tile),
                                  C.c_uint32(peak), C.c_int(packed))


@pytest.mark.parametrize("in_tile, L", [(8192, 64), (848, 7)])
def test_first_occurrence_in_a_packed_tile(emul, in_tile, L):
    rng = np.random.default_rng(in_tile)
    base = rng.integers(0, 700, in_tile).astype(np.uint32)   # below every peak used here; high bits in use
    spots = [r for r in (0, 7, 8, 15, 16, 17, 127, 128, 511, 512, 1023, 1024, 4095, 4096, 8191, 847, 840, 839) if r < in_tile]
    for peak in (701, 1023, 768):
        for r in spots:
            c = base.copy()
            c[r] = peak
            lo, hi = _pack_tile(c, L)
            assert _scan(emul, lo, hi, in_tile, peak, 1) == r, (peak, r)
            # ... and as u16 counts
            u = np.zeros(L * 128, np.uint16)
            u[:in_tile] = c
            assert _scan(emul, u, None, in_tile, peak, 0) == r, (peak, r)
    # a count that differs from the peak in the high bits only, or in the low byte only, is no match
    c = base.copy()
    c[3], c[5], c[9] = 0x1AB, 0x2AB, 0x3AA
    lo, hi = _pack_tile(c, L)
    assert _scan(emul, lo, hi, in_tile, 0x3AB, 1) == NONE
    c[in_tile - 1] = 0x3AB
    lo, hi = _pack_tile(c, L)
    assert _scan(emul, lo, hi, in_tile, 0x3AB, 1) == in_tile - 1


@pytest.mark.parametrize("in_tile, L", [(8192, 64), (848, 7)])
def test_the_lowest_of_several_wins_whatever_the_lane(emul, in_tile, L):
    base = np.full(in_tile, 3, np.uint32)
    # the peak twice: in different lanes of one step, in different steps, in one lane; the later one in a LOWER lane of a later step
    for a, b in ((5, 40), (40, 1030), (33, 34), (700, 16 * 64 + 3), (8, in_tile - 1)):
        if b >= in_tile:
            b = in_tile - 2
        c = base.copy()
        c[[a, b]] = 900
        lo, hi = _pack_tile(c, L)
        assert _scan(emul, lo, hi, in_tile, 900, 1) == min(a, b), (a, b)
        u = np.zeros(L * 128, np.uint16)
        u[:in_tile] = c
        assert _scan(emul, u, None, in_tile, 900, 0) == min(a, b), (a, b)


def test_the_padding_behind_a_short_tile_is_never_a_match(emul):
    in_tile, L = 848, 7
    c = np.zeros(L * 128, np.uint32)
    c[848:] = 77          # what lies behind the last reference (the kernels leave 0 there: anything must do)
    c[100] = 76
    lo, hi = _pack_tile(c, L)
    assert _scan(emul, lo, hi, in_tile, 77, 1) == NONE
    assert _scan(emul, c.astype(np.uint16), None, in_tile, 77, 0) == NONE
    assert _scan(emul, lo, hi, in_tile, 76, 1) == 100


def test_position_of_a_reference_in_the_packed_form(emul):
    for L in (64, 7):
        counts = np.arange(L * 128, dtype=np.uint32) % 1024
        lo, hi = _pack_tile(counts, L)
        for rl in (0, 7, 8, 127, 128, 847, 895, 4096, 8191):
            if rl >= L * 128:
                continue
            byte, word, shift = C.c_uint32(), C.c_uint32(), C.c_uint32()
            emul.emul_packed_count_pos(C.c_uint32(rl), C.byref(byte), C.byref(word), C.byref(shift))
            got = int(lo[byte.value]) | (((int(hi[word.value]) >> shift.value) & 3) << 8)
            assert got == counts[rl], (L, rl)

"""Dereplication, the parts that run without a GPU: rtx_derep_plan (the host side of the map), the error paths and the constants."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import raxtax_amd as rx
from raxtax_amd import _lib

ROOT = Path(__file__).resolve().parent.parent


def restated(rep):
    """(uniq, slot, size) of a map, restated with numpy."""
    rep = np.asarray(rep, dtype=np.int64)
    uniq = np.flatnonzero(rep == np.arange(len(rep)))
    slot = np.searchsorted(uniq, rep)
    size = np.bincount(slot, minlength=len(uniq)) if len(rep) else np.zeros(0, np.int64)
    return uniq, slot, size


FAR = np.arange(400)
FAR[[350, 398, 399]] = [3, 17, 0]   # copies hundreds of queries behind their first occurrence

MAPS = {
    "all_distinct": np.arange(37),
    "all_identical": np.zeros(50, dtype=np.int64),
    "far_apart": FAR,
    "empty": np.zeros(0, dtype=np.int64),
    "one": np.zeros(1, dtype=np.int64),
    "mixed": np.array([0, 0, 2, 0, 2, 5, 6, 5, 8, 0]),
}


@pytest.mark.parametrize("name", sorted(MAPS))
def test_plan_equals_its_numpy_restatement(name):
    rep = MAPS[name]
    assert all(rep[rep[q]] == rep[q] and rep[q] <= q for q in range(len(rep)))   # (the hand-made map is one)
    uniq, slot, size = rx.derep_plan(rep)
    e_uniq, e_slot, e_size = restated(rep)
    assert np.array_equal(uniq, e_uniq)
    assert np.array_equal(slot, e_slot)
    assert np.array_equal(size, e_size)
    assert int(size.sum()) == len(rep)
    assert uniq.dtype == slot.dtype == size.dtype == np.uint32
    if len(rep):
        assert np.array_equal(uniq[slot], rep)   # slot[q] is the position of rep[q] in uniq


def test_plan_refuses_a_representative_behind_its_query():
    with pytest.raises(rx.RtxError) as e:
        rx.derep_plan(np.array([0, 2, 2]))
    assert e.value.code == _lib.RTX_ERR_INVALID


def test_plan_refuses_a_chain():
    with pytest.raises(rx.RtxError) as e:
        rx.derep_plan(np.array([0, 0, 1]))   # rep[2] = 1, but 1 is not its own representative
    assert e.value.code == _lib.RTX_ERR_INVALID


def test_plan_reports_the_count_through_the_c_abi():
    lib = _lib.load()
    rep = np.array([0, 0, 2, 2, 2], dtype=np.uint32)
    uniq, slot, size = (np.full(5, 99, dtype=np.uint32) for _ in range(3))
    nu = C.c_uint64(77)
    assert lib.rtx_derep_plan(5, _lib.ptr(rep, _lib.u32p), _lib.ptr(uniq, _lib.u32p), _lib.ptr(slot, _lib.u32p), _lib.ptr(size, _lib.u32p), C.byref(nu)) == 0
    assert nu.value == 2
    assert list(uniq[:2]) == [0, 2] and list(slot) == [0, 0, 1, 1, 1] and list(size[:2]) == [2, 3]
    nu = C.c_uint64(77)
    assert lib.rtx_derep_plan(0, None, None, None, None, C.byref(nu)) == 0 and nu.value == 0


def test_create_without_a_device_is_loud():
    lib = _lib.load()
    if lib.rtx_device_count() != 0:   # (with a GPU the object exists; what it computes: test_gpu_derep.py)
        rx.Derep(device=0)
        return
    h = C.c_void_p()
    assert lib.rtx_derep_create(0, C.byref(h)) == _lib.RTX_ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(rx.RtxError) as e:
        rx.Derep(device=0)
    assert e.value.code == _lib.RTX_ERR_NO_DEVICE


def test_constants_are_the_header_s():
    text = (ROOT / "include" / "raxtax_hip.h").read_text()
    defs = dict(re.findall(r"^#define (RTX_[A-Z_]+) (\d+)\b", text, flags=re.M))
    assert int(defs["RTX_OPT_DEREP"]) == _lib.RTX_OPT_DEREP == 27
    assert int(defs["RTX_DEFAULT_DEREP_HASH_MASK"]) == _lib.RTX_DEFAULT_DEREP_HASH_MASK == 3
    assert int(defs["RTX_ABI_VERSION"]) == 6
    # the default option is known to the library (0 restores the full hash)
    assert _lib.load().rtx_set_default_option(_lib.RTX_DEFAULT_DEREP_HASH_MASK, 0) == 0

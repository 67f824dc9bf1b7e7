"""CPU emulation of the segmented sketch kernel (auriclass_amd/csrc/mhx_segsketch.h, the very functions the kernel runs:
staging around seg_off, the per-window hash, the sort network, selection), run thread by thread by
tests/emul/segsketch_emul.cpp, against the oracle's definition-level sketch of every segment (tests/segment_cases.py)."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import segment_cases as sc

ABOVE_CUT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("segsketch_emul")
    L.emul_seg_cut.restype = ctypes.c_uint32
    L.emul_seg_sort_size.argtypes = [ctypes.c_uint32]
    L.emul_seg_sort_size.restype = ctypes.c_uint32
    L.emul_segsketch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_uint32]
    return L


def run(L, data: bytes, off: np.ndarray, k: int, s: int, shift: int = 0, stride=None):
    """shift: misalignment of the stream's first byte (the kernel stages whole aligned dwords around a segment)"""
    pad = np.full(len(data) + 64, ord("A"), dtype=np.uint8)       # valid bases around the stream: a cut that leaks would show
    base = (-pad.ctypes.data) % 16 + 16 + shift
    pad[base:base + len(data)] = np.frombuffer(data, dtype=np.uint8)
    n_seg = off.size - 1
    if stride is None:
        stride = max(1, min(s, int(np.diff(off.astype(np.int64)).max()) - k + 1)) if n_seg else 1
    rows = np.full((n_seg, stride), 0x5555555555555555, dtype=np.uint64)
    lens = np.full(n_seg, 0xDEAD, dtype=np.uint32)
    assert L.emul_segsketch(k, pad.ctypes.data + base, off.ctypes.data, n_seg, s, rows.ctypes.data, lens.ctypes.data, stride) == 0
    return rows, lens


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", sc.CASES)
def test_cases_against_the_oracle(emul, name, k):
    cut = emul.emul_seg_cut()
    data, off = sc.case(name, k, cut)
    windows = np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0)
    above = {int(i) for i in np.nonzero(windows > cut)[0]}
    assert bool(above) == (name == "edge_lengths")
    for s in sc.SS:
        rows, lens = run(emul, data, off, k, s, shift=(k + s) % 4)
        sc.check_rows(rows, lens, name, k, s, cut, skip=above)
        for i in above:                                                # the host's share: the kernel leaves the row alone
            assert lens[i] == ABOVE_CUT and (rows[i] == 0x5555555555555555).all()


def test_the_seam_sits_at_the_cut(emul):
    cut = emul.emul_seg_cut()
    assert cut >= 1024 and cut & (cut - 1) == 0
    k = 21
    data, off = sc.case("edge_lengths", k, cut)
    windows = np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0)
    assert {cut - 1, cut, cut + 1} <= set(int(w) for w in windows)
    _, lens = run(emul, data, off, k, 16)
    assert [int(w) for w, n in zip(windows, lens) if n == ABOVE_CUT] == [cut + 1]


def test_sort_size_is_the_power_of_two_at_or_above(emul):
    cut = emul.emul_seg_cut()
    for w in [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, cut - 1, cut]:
        n = emul.emul_seg_sort_size(w)
        assert n >= max(2, w) and n & (n - 1) == 0 and (n // 2 < w or n == 2)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_misalignment_of_the_stream(emul, shift):
    cut = emul.emul_seg_cut()
    data, off = sc.case("touching", 17, cut)
    rows, lens = run(emul, data, off, 17, 1000, shift=shift)
    sc.check_rows(rows, lens, "touching", 17, 1000, cut)


def test_rows_are_cut_at_the_stride(emul):
    """a stride below s (the engine refuses one that is too small; the kernel must still stay inside the row)"""
    cut = emul.emul_seg_cut()
    data, off = sc.case("repeats", 21, cut)
    rows, lens = run(emul, data, off, 21, 1000, stride=5)
    want = sc.expected_full("repeats", 21, cut)
    for i, full in enumerate(want):
        assert lens[i] == min(5, full.size) and np.array_equal(rows[i, :lens[i]], full[:lens[i]])

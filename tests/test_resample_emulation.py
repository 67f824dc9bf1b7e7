"""CPU emulation of the jackknife kernels (auriclass_amd/csrc/mhx_resample.h, the very functions the kernels run):
tests/emul/resample_emul.cpp runs whole calls chunk by chunk -- 64-lane ballots, the set bits below a lane, the waves' totals --
and the cut.  Rows, order, counts and s_r equal the rule's (tests/resample_rule.py), and the tail of every row is zero."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import resample_rule as rr
from tests import triangle_cases as tc

LADDER = (0, 1, 63, 64, 65, 255, 256, 257, 1000)   # around a wave, around a chunk, several chunks


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("resample_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_resample_mix.argtypes = [u64, u64, u32]
    L.emul_resample_mix.restype = u64
    L.emul_resample_keeps.argtypes = [u64, u64, u32, u64]
    L.emul_resample_threshold.argtypes = [ctypes.c_double, ctypes.POINTER(u64)]
    L.emul_resample_call.argtypes = [vp, vp, u32, u32, u32, u64, u32, u64, vp, vp, ctypes.POINTER(u32)]
    L.emul_resample_call.restype = u64
    return L


def ladder_lists(top=1000):
    """lists of the ladder's lengths off one base, so that they share hashes; the base holds 0 and 2^64 - 1"""
    rng = np.random.default_rng(81)
    base = np.unique(np.concatenate([tc.sketch_like(rng, top + 50)[:top - 2], np.array([0, 2 ** 64 - 1], np.uint64)]))
    assert len(base) == top and base[0] == 0 and base[-1] == 2 ** 64 - 1
    lists = [base[:n].copy() for n in LADDER]
    lists.append(base[-300:].copy())                      # a list that ends with 2^64 - 1
    lists.append(tc.mutate(rng, base, 0.3)[:top].copy())  # another full one
    return lists


def run(L, lists, stride, s, seed, r, keep):
    M, lens = tc.pad_rows(lists, stride)
    out = np.full_like(M, 0xDEADBEEFDEADBEEF)
    out_len = np.full_like(lens, 0xFFFFFFFF)
    s_r = ctypes.c_uint32(0)
    outside = L.emul_resample_call(M.ctypes.data, lens.ctypes.data, len(lists), stride, s, seed, r, rr.threshold(keep), out.ctypes.data, out_len.ctypes.data,
                                   ctypes.byref(s_r))
    assert outside == 0
    return out, out_len, s_r.value


def test_header_arithmetic_is_the_rules(emul):
    rng = np.random.default_rng(82)
    cases = [(0, 0, 0), (2 ** 64 - 1, 42, 3), (0xFFFFFFFFFFFFFF00, 0xFFFFFFFFFFFFFFF0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 9999)]
    cases += [(int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 10000))) for _ in range(300)]
    for h, seed, r in cases:
        assert emul.emul_resample_mix(h, seed, r) == rr.mix(h, seed, r), (h, seed, r)
        for T in (1, 1 << 31, 1 << 32):
            assert bool(emul.emul_resample_keeps(h, seed, r, T)) == rr.keeps(h, seed, r, T)
    T = ctypes.c_uint64(0)
    for keep in (1.0, 0.5, 0.03, 2.0 ** -32, 0.9999999999):
        assert emul.emul_resample_threshold(keep, ctypes.byref(T)) == 1 and T.value == rr.threshold(keep)
    for bad in (0.0, -1.0, 1.0000001, float("nan"), float("inf")):
        assert emul.emul_resample_threshold(bad, ctypes.byref(T)) == 0


@pytest.mark.parametrize("keep", [0.5, 1.0, 0.03])
@pytest.mark.parametrize("stride", [1000, 1008, 1024])   # len == stride; no multiple of 64; a multiple of 64
def test_whole_calls_equal_the_rule(emul, stride, keep):
    lists = ladder_lists()
    s = 1000
    for seed, r in ((42, 0), (2 ** 64 - 1, 7)):
        want, want_s = rr.replicate(lists, s, seed, r, keep)
        out, out_len, s_r = run(emul, lists, stride, s, seed, r, keep)
        assert s_r == want_s and (keep < 1.0 or s_r == s)
        assert out_len.tolist() == [len(v) for v in want]
        for i, v in enumerate(want):
            assert out[i, :len(v)].tolist() == v.tolist(), i
            assert not out[i, len(v):].any(), i


def test_short_rows_alone_leave_s(emul):
    """no row is full: s_r = s and nothing is cut; a stride of one chunk and of one more"""
    lists = ladder_lists()[:6]
    for stride in (256, 257):
        want, want_s = rr.replicate(lists, 1000, 1, 2, 0.5)
        out, out_len, s_r = run(emul, lists, stride, 1000, 1, 2, 0.5)
        assert s_r == want_s == 1000 and out_len.tolist() == [len(v) for v in want]
        for i, v in enumerate(want):
            assert out[i, :len(v)].tolist() == v.tolist() and not out[i, len(v):].any()
    # one row of one hash at stride 1
    out, out_len, s_r = run(emul, [np.array([2 ** 64 - 1], np.uint64)], 1, 1, 0, 0, 1.0)
    assert out.tolist() == [[2 ** 64 - 1]] and out_len.tolist() == [1] and s_r == 1

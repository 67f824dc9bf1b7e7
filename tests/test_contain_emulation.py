"""mhx_contain.h on the CPU (tests/emul/contain_emul.cpp runs the header's own functions) against the rule of
tests/contain_rule.py on every shared case: the bounds, the pair walk with 1, 3, 64 and 256 shares, and the finish pass of a
(query batch, reference slice) block at 16, 64 and 1024 value ranges, fed by the emulated split and range passes.  A block
whose flag goes up writes nothing -- the pair kernel's case -- and every number of ranges must be reached without a flag by
the case made for it.  CPU only."""
import ctypes
import functools

import numpy as np
import pytest

from tests import contain_cases as cc
from tests import emul_build

SHARES = (1, 3, 64, 256)
RANGES = (16, 64, 1024)
ALL = ("crafted",) + cc.NAMES


@functools.lru_cache(maxsize=None)
def emul():
    L = emul_build.load("contain_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_contain_pair_threads.restype = u32
    L.emul_contain_bounds.argtypes = [vp, vp, u32, u32, u32, vp, vp]
    L.emul_contain_bounds.restype = None
    L.emul_contain_pair.argtypes = [vp, u32, u64, vp, u32, u64, u32, vp, vp, vp]
    L.emul_contain_pair.restype = None
    L.emul_contain_block.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.emul_contain_block.restype = ctypes.c_int
    return L


def rows(name):
    return cc.crafted_rows() if name == "crafted" else cc.rows_of(name)


def bounds(M, lens, s):
    eff, bound = np.zeros(len(lens), np.uint32), np.zeros(len(lens), np.uint64)
    emul().emul_contain_bounds(M.ctypes.data, lens.ctypes.data, len(lens), M.shape[1], s, eff.ctypes.data, bound.ctypes.data)
    return eff, bound


def test_the_kernel_has_one_share_per_thread():
    assert emul().emul_contain_pair_threads() == 256


@pytest.mark.parametrize("name", ALL)
def test_bounds(name):
    Q, q_len, R, r_len, s_q, s_r = rows(name)
    for M, lens, s in ((Q, q_len, s_q), (R, r_len, s_r)):
        eff, bound = bounds(M, lens, s)
        for i in range(len(lens)):
            n = min(int(lens[i]), M.shape[1], s)
            assert eff[i] == n
            assert int(bound[i]) == (int(M[i, n - 1]) if n == s else 2 ** 64 - 1)


@pytest.mark.parametrize("name", ALL)
def test_pair_walk_equals_the_rule(name):
    Q, q_len, R, r_len, s_q, s_r = rows(name)
    want = cc.expected(name)
    (q_eff, q_bound), (r_eff, r_bound) = bounds(Q, q_len, s_q), bounds(R, r_len, s_r)
    nq, nr = len(q_len), len(r_len)
    step = 11 if nq * nr > 4000 else 1   # every eleventh pair of the large case: the finish test below covers all of them
    c, a, b = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    at = 0
    for i in range(nq):
        for j in range(nr):
            at += 1
            if at % step:
                continue
            for shares in SHARES if q_eff[i] + r_eff[j] < 10000 else (3, 256):
                emul().emul_contain_pair(R[j].ctypes.data, int(r_eff[j]), int(r_bound[j]), Q[i].ctypes.data, int(q_eff[i]), int(q_bound[i]), shares,
                                         ctypes.byref(c), ctypes.byref(a), ctypes.byref(b))
                assert (c.value, a.value, b.value) == (int(want[0][i, j]), int(want[1][i, j]), int(want[2][i, j])), (name, i, j, shares)


def finish(name, ranges):
    """the blocks of the case at `ranges`: (#blocks, #flagged); every unflagged block must equal the rule"""
    Q, q_len, R, r_len, s_q, s_r = rows(name)
    want = cc.expected(name)
    nq, nr = len(q_len), len(r_len)
    blocks = flagged = 0
    for r0 in range(0, nr, 32):
        bnr = min(32, nr - r0)
        Rb, rl = np.ascontiguousarray(R[r0:r0 + bnr]), np.ascontiguousarray(r_len[r0:r0 + bnr])
        got = [np.full((nq, bnr), 0xFFFFFFFF, np.uint32) for _ in range(3)]
        rc = emul().emul_contain_block(Q.ctypes.data, q_len.ctypes.data, nq, s_q, Rb.ctypes.data, rl.ctypes.data, bnr, s_r, Q.shape[1], ranges,
                                       got[0].ctypes.data, got[1].ctypes.data, got[2].ctypes.data)
        assert rc in (0, 1), (name, ranges, rc)
        blocks += 1
        if rc == 1:
            flagged += 1
            assert all((g == 0xFFFFFFFF).all() for g in got)   # a flagged block writes nothing
            continue
        for g, w, what in zip(got, want, ("shared", "n_qry", "n_ref")):
            assert np.array_equal(g, w[:, r0:r0 + bnr]), (name, ranges, r0, what, np.argwhere(g != w[:, r0:r0 + bnr])[:5])
    return blocks, flagged


@pytest.mark.parametrize("ranges", RANGES)
@pytest.mark.parametrize("name", [n for n in ALL if n != "long_pair"])
def test_range_finish_equals_the_rule(name, ranges):
    blocks, flagged = finish(name, ranges)
    print(name, ranges, "blocks", blocks, "flagged", flagged)
    clean = {16: ("crafted", "small"), 64: ("crafted", "small", "mixed", "set200", "extreme", "extreme_mirrored"),
             1024: ("crafted", "small", "mixed", "set200", "extreme", "extreme_mirrored")}
    if name in clean[ranges]:
        assert flagged == 0
    # what the pair kernel is there for: one value range holds nearly all of a crowded list at any geometry, and all 1000
    # entries of a large genome's sketch when a short list spans the hash space and the ranges are 64 or fewer
    if name == "crowded" or (name in ("plasmids", "plasmids_swapped") and ranges <= 64):
        assert flagged == blocks

"""mhx_contain_winner.h on the CPU (tests/emul/contain_winner_emul.cpp runs the header's own comparator, claim and tally)
against the rule of tests/contain_winner_rule.py on every shared case.  The pairs are claimed in forward, reverse and one
shuffled order, with workgroups of 256 and of 3 threads: a winner word must end at the best-ranked proposer whatever the
order of arrival.  CPU only."""
import ctypes
import functools

import numpy as np
import pytest

from tests import contain_winner_cases as wc
from tests import contain_winner_rule as wrule
from tests import emul_build


@functools.lru_cache(maxsize=None)
def emul():
    L = emul_build.load("contain_winner_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_contain_claim_threads.restype = u32
    L.emul_contain_ranks_before.argtypes = [vp, vp, vp, u32, u32]
    L.emul_contain_ranks_before.restype = ctypes.c_int
    L.emul_contain_winner.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp, vp]
    L.emul_contain_winner.restype = u64
    return L


def orders(n):
    forward = np.arange(n, dtype=np.uint32)
    return (("forward", forward), ("reverse", forward[::-1].copy()), ("shuffled", np.random.default_rng(2024).permutation(n).astype(np.uint32)))


def test_the_kernel_has_one_share_per_thread():
    assert emul().emul_contain_claim_threads() == 256


def test_comparator_equals_the_rank_key():
    """every ordered pair of references of the small cases that compete, without and with lengths; ratios that tie exactly
    (8 / 8 against 8 / 8, 1 / 2 against 4 / 8) and products above 2^32"""
    shared = np.array([8, 4, 8, 3, 1, 4, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD], np.uint32)
    n_ref = np.array([8, 5, 8, 8, 2, 8, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32)
    for lengths in (None, np.array([5, 5, 9, 5, 5, 6, 1, 1, 1], np.uint64)):
        lp = None if lengths is None else lengths.ctypes.data
        for a in range(len(shared)):
            for b in range(len(shared)):
                if a == b:
                    continue
                la, lb = (0, 0) if lengths is None else (lengths[a], lengths[b])
                want = wrule.rank_key(shared[a], n_ref[a], la, a) > wrule.rank_key(shared[b], n_ref[b], lb, b)
                assert bool(emul().emul_contain_ranks_before(shared.ctypes.data, n_ref.ctypes.data, lp, a, b)) == want, (a, b)


@pytest.mark.parametrize("name", wc.NAMES)
def test_claim_in_any_order_equals_the_rule(name):
    Q, q_len, R, r_len, s_q, s_r, lengths = wc.rows_of(name)
    want = wc.expected(name)
    nq, nr = len(q_len), len(r_len)
    walked_want = int((want[1] > 0).sum())
    for what, order in orders(nq * nr):
        for shares in (256, 3) if what == "forward" else (256,):
            got = [np.full((nq, nr), 0xFFFFFFFF, np.uint32) for _ in range(4)]
            walked = emul().emul_contain_winner(Q.ctypes.data, q_len.ctypes.data, nq, s_q, R.ctypes.data, r_len.ctypes.data, nr, s_r, Q.shape[1],
                                                None if lengths is None else lengths.ctypes.data, order.ctypes.data, shares, *(g.ctypes.data for g in got))
            assert walked == walked_want, (name, what, shares, walked)
            for g, w, col in zip(got, want[:4], ("won", "shared", "n_qry", "n_ref")):
                assert np.array_equal(g, w), (name, what, shares, col, np.argwhere(g != w)[:5])
            wrule.check_consequences(got[0], got[1], got[2], got[3], want[4], lengths)

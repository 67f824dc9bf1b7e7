"""CPU emulation of the winner-take-all form of the containment screen (auriclass_amd/csrc/mhx_screen.h, the very functions
the kernels and the engine run: priority order, claim, "won"), run sequentially by tests/emul/screen_winner_emul.cpp,
against the plain statement of the rule (tests/screen_winner_rule.py)."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import screen_winner_rule as wrule
from tests.test_screen_emulation import pack, random_case

MAXKEY = np.uint64(0xFFFFFFFFFFFFFFFF)
K = 21


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("screen_winner_emul")
    L.emul_screen_winner.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                     ctypes.c_uint64] + [ctypes.c_void_p] * 5
    L.emul_screen_winner.restype = ctypes.c_int64
    return L


def run(L, refs, probes, lengths=None):
    rows, lens = pack(refs)
    probes = np.ascontiguousarray(probes, dtype=np.uint64)
    length = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint64)
    counts = np.zeros(rows.shape, dtype=np.uint32)
    shared, median, shared0, prio = (np.zeros(len(refs), dtype=np.uint32) for _ in range(4))
    claimed = L.emul_screen_winner(rows.ctypes.data, lens.ctypes.data, None if length is None else length.ctypes.data, len(refs),
                                   rows.shape[1], probes.ctypes.data, probes.size, counts.ctypes.data, shared.ctypes.data,
                                   median.ctypes.data, shared0.ctypes.data, prio.ctypes.data)
    return claimed, counts, shared, median, shared0, prio


def check(L, refs, probes, lengths=None, k=K):
    claimed, counts, shared, median, shared0, prio = run(L, refs, probes, lengths)
    want = wrule.winner_tally(refs, probes, k, lengths)
    for i, (c, s, m) in enumerate(want):
        assert np.array_equal(counts[i, :len(refs[i])], c), i
        assert not counts[i, len(refs[i]):].any()
        assert (int(shared[i]), int(median[i])) == (s, m), i
    # priorities: unique, 1 .. nr, never "nobody"
    assert sorted(int(p) for p in prio) == list(range(1, len(refs) + 1))
    # the invariant: every found hash has exactly one winner
    found = wrule.distinct_found(refs, probes)
    assert int(shared.sum()) == found == claimed
    return shared, median, counts


@pytest.mark.parametrize("seed,bits,nr,n", [(1, 64, 4, 500), (2, 64, 24, 2000), (3, 32, 1, 50), (4, 32, 40, 300), (5, 12, 24, 900),
                                            (6, 64, 70, 64), (7, 12, 70, 200), (8, 32, 4, 800)])
def test_random_clades(emul, seed, bits, nr, n):
    refs, probes = random_case(seed, bits, nr, n)
    rng = np.random.default_rng(100 + seed)
    check(emul, refs, probes)                                             # lengths all equal
    check(emul, refs, probes, rng.integers(1, 4, size=nr) * 1000)         # few distinct lengths: ties on the length too


def test_three_identical_references_longest_then_lowest_index(emul):
    rng = np.random.default_rng(21)
    h = np.unique(rng.integers(0, 1 << 64, size=400, dtype=np.uint64))
    probes = np.repeat(h[::3], 2)
    shared, _, _ = check(emul, [h, h, h], probes, [5, 9, 9])
    assert list(shared) == [0, h[::3].size, 0]                            # index 1: the longer genome, and ahead of index 2
    shared, _, _ = check(emul, [h, h, h], probes, [7, 7, 7])
    assert list(shared) == [h[::3].size, 0, 0]
    shared, _, _ = check(emul, [h, h, h], probes)                         # no lengths given
    assert list(shared) == [h[::3].size, 0, 0]


def test_subset_with_the_same_score_loses_to_the_longer_genome(emul):
    rng = np.random.default_rng(22)
    h = np.unique(rng.integers(0, 1 << 64, size=600, dtype=np.uint64))
    half = h[::2]
    # all found: both score 1; the shared half goes to the longer genome, whichever index it has
    shared, _, _ = check(emul, [h, half], h, [100, 50])
    assert list(shared) == [h.size, 0]
    shared, _, _ = check(emul, [h, half], h, [50, 100])
    assert list(shared) == [h.size - half.size, half.size]
    shared, _, _ = check(emul, [half, h], h, [50, 50])                    # equal lengths: the lowest index
    assert list(shared) == [half.size, h.size - half.size]
    # a better ratio beats a longer genome: only the half is found, so the subset scores 1 and the full list 1/2
    shared, _, _ = check(emul, [h, half], half, [1000, 1])
    assert list(shared) == [0, half.size]


def test_the_key_that_cannot_live_in_the_table(emul):
    rng = np.random.default_rng(23)
    body = np.unique(rng.integers(0, 1 << 64, size=200, dtype=np.uint64))
    body = body[body != MAXKEY]
    a = np.concatenate([body, [MAXKEY]])
    b = np.concatenate([body[:20], [MAXKEY]])
    probes = np.concatenate([np.repeat(body[:100], 2), np.full(9, MAXKEY, np.uint64)])
    # b: 21 / 21 found, a: 101 / 201 -- b wins what it holds, the key 2^64-1 included
    _, _, counts = check(emul, [a, b], probes)
    assert counts[0, body.size] == 0 and counts[1, 20] == 9
    _, _, counts = check(emul, [a, np.array([MAXKEY], np.uint64), a], probes, [1, 1, 2])
    assert counts[1, 0] == 9 and counts[0, body.size] == 0 and counts[2, body.size] == 0
    # the value never seen: nobody wins it
    shared, _, _ = check(emul, [a, b], np.repeat(body[:100], 2))
    assert int(shared.sum()) == 100


def test_empty_and_one_entry_references_and_nothing_probed(emul):
    rng = np.random.default_rng(24)
    full = np.unique(rng.integers(0, 1 << 64, size=300, dtype=np.uint64))
    refs = [full, np.zeros(0, np.uint64), full[7:8], np.zeros(0, np.uint64)]
    probes = np.concatenate([np.repeat(full[:100], 3), np.repeat(full[7:8], 40)])
    shared, median, _ = check(emul, refs, probes, [10, 99, 1, 99])
    assert list(shared) == [99, 0, 1, 0] and list(median[1:]) == [0, 43, 0]  # the one-entry reference scores 1 and takes its hash
    shared, median, counts = check(emul, refs, np.zeros(0, np.uint64))
    assert not shared.any() and not median.any() and not counts.any()
    assert run(emul, [], probes)[0] == 0


def test_score_order_is_the_exact_ratio(emul):
    """two references whose ratios differ by 1 / (n (n + 1)): 499/1000 against 500/1001 (0.499 < 0.4995...)"""
    rng = np.random.default_rng(25)
    pool = np.unique(rng.integers(0, 1 << 64, size=1700, dtype=np.uint64))
    common = pool[:400]
    a = np.sort(np.concatenate([common, pool[400:1000]]))                 # n = 1000
    b = np.sort(np.concatenate([common, pool[1000:1601]]))[:1001]         # n = 1001
    assert a.size == 1000 and b.size == 1001
    only_a = np.setdiff1d(a, common)[:99]
    only_b = np.setdiff1d(b, common)[:100]
    probes = np.concatenate([common, only_a, only_b])                     # shared0: 499 / 1000 and 500 / 1001
    shared, _, _ = check(emul, [a, b], probes, [5, 1])
    assert list(shared) == [99, 500]

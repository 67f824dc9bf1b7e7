"""CPU emulation of the all-pairs path within one sketch set (auriclass_amd/csrc/mhx_triangle.h and mhx_dist.h, the very
functions the kernels run): tests/emul/triangle_emul.cpp runs them sequentially -- shift, ONE split pass over the set,
then block by block the range pass, the finish walk of the block's geometry and the scatter into the packed triangle.
`common` and `denom` of every pair against the oracle's compareSketches; the packed index, the geometry rule, the
schedule and the prefilter of the edge mode on their own."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests import extreme_cases as xc
from tests import triangle_cases as tc

SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("triangle_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_tri_index.argtypes = [u32, u32]
    L.emul_tri_index.restype = u64
    L.emul_tri_ranges.argtypes = [u64]
    L.emul_tri_ranges.restype = u32
    L.emul_tri_ranges_dist.argtypes = [u64]
    L.emul_tri_ranges_dist.restype = u32
    L.emul_tri_max_queries.argtypes = [u32]
    L.emul_tri_max_queries.restype = u32
    L.emul_tri_jmin.argtypes = [ctypes.c_double, ctypes.c_int]
    L.emul_tri_jmin.restype = ctypes.c_double
    L.emul_tri_distance.argtypes = [u32, u32, ctypes.c_int]
    L.emul_tri_distance.restype = ctypes.c_double
    L.emul_tri_keep_many.argtypes = [vp, vp, u64, ctypes.c_double, vp]
    L.emul_tri_keep_many.restype = None
    L.emul_tri_blocks.argtypes = [u32, u32, vp, u32]
    L.emul_tri_blocks.restype = u32
    L.emul_tri_pair_counts.argtypes = [u32] * 6
    L.emul_tri_pair_counts.restype = ctypes.c_int
    L.emul_triangle.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, vp, vp]
    L.emul_triangle.restype = ctypes.c_int
    return L


def run_emul(L, lists, s, ranges=0, qbatch=0):
    M, lens = tc.pad_rows(lists)
    n = len(lists)
    common = np.full(n * (n - 1) // 2, SENTINEL, np.uint32)
    denom = np.full(n * (n - 1) // 2, SENTINEL, np.uint32)
    stats = np.zeros(6, np.uint32)
    rc = L.emul_triangle(M.ctypes.data, lens.ctypes.data, n, M.shape[1], s, ranges, qbatch, common.ctypes.data, denom.ctypes.data,
                         stats.ctypes.data)
    return rc, common, denom, stats


@pytest.mark.parametrize("n", [2, 3, 33, 70])
def test_packed_index_is_a_bijection(emul, n):
    got = [emul.emul_tri_index(i, j) for i in range(n) for j in range(i)]
    assert got == list(range(n * (n - 1) // 2))   # rows in Mash's print order, nothing skipped, nothing twice


def test_packed_index_at_the_largest_set(emul):
    n = 65536
    assert emul.emul_tri_index(1, 0) == 0 and emul.emul_tri_index(2, 0) == 1 and emul.emul_tri_index(2, 1) == 2
    assert emul.emul_tri_index(n - 1, 0) == (n - 1) * (n - 2) // 2
    assert emul.emul_tri_index(n - 1, n - 2) == n * (n - 1) // 2 - 1 == 2 ** 31 - 32769   # 64-bit arithmetic: i (i - 1) passes 2^32
    assert emul.emul_tri_index(n - 2, n - 3) + 1 == emul.emul_tri_index(n - 1, 0)


def test_geometry_rule(emul):
    """R from the longest list alone: the smallest power of two with longest <= 16 R, between 16 and 16 384; nothing beyond 2^20"""
    r = emul.emul_tri_ranges
    assert r(1000) == 64 and r(8193) == 1024 and r(16_384) == 1024 and r(20_000) == 2048
    assert r(262_144) == 16_384 and r(262_145) == 16_384 and r(1_000_000) == 16_384 and r(1 << 20) == 16_384
    assert r(0) == 16 and r(1) == 16 and r(17) == 16 and r(256) == 16 and r(257) == 32
    assert r((1 << 20) + 1) == 0 and r(1 << 31) == 0 and r(1 << 40) == 0
    last = 16
    for n in list(range(1, 1 << 20, 4099)) + [16 * (1 << e) + d for e in range(4, 15) for d in (-1, 0, 1)]:
        got = r(n)
        assert 16 <= got <= 16_384 and got & (got - 1) == 0, n
        assert n <= 16 * got or got == 16_384, n
        assert got == 16 or n > 16 * got // 2, (n, got)   # the smallest that fits
    for n in range(1, (1 << 20) + 1, 65_521):
        assert r(n) >= last
        last = r(n)
    # the A/B switch: the geometry of mhx_dist_batch, never fewer than 1024 ranges
    d = emul.emul_tri_ranges_dist
    assert d(1000) == 1024 and d(65_536) == 1024 and d(65_537) == 2048 and d(1 << 20) == 16_384 and d((1 << 20) + 1) == 0


def test_block_workspace_keeps_32_bit_indices(emul):
    for ranges in (16, 64, 512, 1024, 2048, 16_384):
        n = emul.emul_tri_max_queries(ranges)
        work = n * (ranges * 32 + 256 + (ranges // 64 * 128 if ranges > 1024 else 0)) + 1024
        assert n >= 1 and work <= 256 << 20
        assert n * (ranges + 1) < 2 ** 32
    assert emul.emul_tri_max_queries(64) == 65_536   # a whole set of the largest size in one batch at s = 1000


@pytest.mark.parametrize("qbatch", [0, 48])
@pytest.mark.parametrize("n", [1, 2, 32, 33, 64, 70, 200])
def test_schedule_counts_every_pair_once(emul, n, qbatch):
    qb = qbatch or emul.emul_tri_max_queries(64)
    out = np.zeros(4 * 64, np.uint32)
    count = emul.emul_tri_blocks(n, qb, out.ctypes.data, 64)
    assert count <= 64
    seen = np.zeros((n, n), np.int32)
    for r0, nr, q0, nq in out[:4 * count].reshape(-1, 4).tolist():
        assert r0 % 32 == 0 and 1 <= nr <= 32 and r0 + nr <= n and nr == min(32, n - r0)
        assert 1 <= nq <= qb and q0 >= r0 + 1 and q0 + nq <= n
        for ql in range(nq):
            for rl in range(32):
                counts = emul.emul_tri_pair_counts(r0, nr, q0, nq, ql, rl)
                assert counts == int(rl < nr and r0 + rl < q0 + ql)
                if counts:
                    seen[q0 + ql, r0 + rl] += 1
        assert not emul.emul_tri_pair_counts(r0, nr, q0, nq, nq, 0)
    want = np.tril(np.ones((n, n), np.int32), -1)
    assert np.array_equal(seen, want)   # every j < i exactly once, nothing else
    if n == 1:
        assert count == 0


@pytest.mark.parametrize("ranges,qbatch", [(0, 0), (64, 48), (512, 0), (1024, 0), (2048, 0)])
def test_emulated_triangle_equals_the_oracle(emul, ranges, qbatch):
    """The 70-list set through the rule's own geometry (64 ranges), the short-range finish with R forced to 64 (in query
    batches of 48) and 512, the base finish at 1024 and the windowed finish at 2048.  (R = 16: the next test.)"""
    lists, s = tc.set70()
    rc, common, denom, stats = run_emul(emul, lists, s, ranges, qbatch)
    print("ranges", stats[0], "longest slice", stats[1], "most distinct keys in a range", stats[2], "blocks", stats[3], "thrown away", stats[5])
    assert rc == 0 and stats[0] == (ranges or 64) and stats[4] == 0
    assert stats[3] == (3 if not qbatch else 2 + 1 + 1)
    assert stats[1] <= 255 and stats[2] <= 1536
    want_c, want_d, _ = tc.expected("set70")
    assert not (common == SENTINEL).any() and not (denom == SENTINEL).any()
    assert np.array_equal(common, want_c) and np.array_equal(denom, want_d)


def test_sixteen_ranges_one_range_per_segment(emul):
    """R forced to 16, where each of the 16 threads of a pair sums ONE range.  At s = 1000 a slice of 32 independent lists
    puts 32 x 1000 / 16 = 2000 keys into a range's table, more than its 1536: on the 70-list set as it is the emulated
    range pass raises the flag in the slice of 32 independent lists (the generic kernel's case, nothing of it is scattered),
    and what the first slice (the base list, its copies, 21 others: ~1400 keys) and the last (6 lists) scatter is the oracle's.  The
    same 70 lists thinned to every second hash (s = 500, 1000 keys per range) go through whole and are the oracle's."""
    lists, s = tc.set70()
    want_c, want_d, _ = tc.expected("set70")
    rc, common, denom, stats = run_emul(emul, lists, s, 16)
    assert rc == 1 and stats[0] == 16 and stats[3] == 3 and stats[4] == 1 and stats[2] > 1536
    done = common != SENTINEL
    assert np.array_equal(done, denom != SENTINEL)
    unflagged = np.array([j < 32 or j >= 64 for i in range(70) for j in range(i)])
    assert np.array_equal(done, unflagged)
    assert np.array_equal(common[done], want_c[done]) and np.array_equal(denom[done], want_d[done])
    thin = tuple(v[::2] for v in lists)
    rc, common, denom, stats = run_emul(emul, thin, 500, 16)
    print("ranges", stats[0], "longest slice", stats[1], "most distinct keys in a range", stats[2])
    assert rc == 0 and stats[0] == 16 and stats[4] == 0 and stats[1] <= 255 and stats[2] <= 1536
    thin_c, thin_d, _ = tc.oracle_pairs(thin, 500, 21)
    assert np.array_equal(common, thin_c) and np.array_equal(denom, thin_d)


def test_crowded_values_raise_the_flag(emul):
    """The construction of test_crowded_values_raise_the_flag (tests/test_dist_emulation.py): one value range holds nearly
    everything, every block gives up (the generic kernel's case) and nothing is scattered."""
    lists, s = tc.crowded(12)
    for ranges in (0, 1024):
        rc, common, denom, stats = run_emul(emul, lists, s, ranges)
        assert rc == 1 and stats[4] == stats[3] == 1 and stats[1] > 255
        assert (common == SENTINEL).all()


def oracle_distance(common, denom, k):
    """the oracle's distance of a pair with these counts: compareSketches on two lists that produce them"""
    c, d, dist = mo.compare(np.arange(denom, dtype=np.uint64), np.arange(common, dtype=np.uint64), denom, k)
    assert (c, d) == (common, denom)
    return dist


def test_prefilter_keeps_what_the_exact_rule_keeps(emul):
    """For every k, denom and common of the sweep and every bound D: a pair whose oracle distance is <= D passes tri_keep with
    the host's jmin; the pairs that pass although their distance is above D (the slack of 2^-30 in the Jaccard index) stay
    below 1 % of the sweep."""
    total = extra = 0
    for k in (11, 21, 27, 32):
        for denom in (1, 7, 1000, 50_000):
            commons = np.array(sorted(set(range(0, denom + 1, 97 if denom == 50_000 else 1)) | {denom}), np.uint32)
            denoms = np.full(commons.size, denom, np.uint32)
            dist = np.array([oracle_distance(int(c), denom, k) for c in commons])
            assert all(emul.emul_tri_distance(int(c), denom, k) == x for c, x in zip(commons[::37], dist[::37]))   # the library's own arithmetic
            for D in (0.0, 0.001, 0.05, 0.3, 0.999, 1.0):
                keep = np.zeros(commons.size, np.uint8)
                emul.emul_tri_keep_many(commons.ctypes.data, denoms.ctypes.data, commons.size, emul.emul_tri_jmin(D, k), keep.ctypes.data)
                must = dist <= D
                assert keep[must].all(), (k, denom, D, commons[must & (keep == 0)][:5])
                total += commons.size
                extra += int((keep.astype(bool) & ~must).sum())
    print("pairs kept beyond the exact rule:", extra, "of", total)
    assert extra < 0.01 * total


@pytest.mark.parametrize("ranges", [0, 16, 1024, 2048])
@pytest.mark.parametrize("mirrored", [False, True])
def test_the_vacant_slot_marker_as_a_hash(emul, mirrored, ranges):
    """2^64 - 1 (kEmptyKey) and values of its home slot in one set (the planted batch of tests/extreme_cases.py, references
    then queries: 73 lists, three slices), through every finish form.  Before the range table kept 2^64 - 1 out of its slots
    the pairs of its holders with the holders of the colliding value were one off (the figures: tests/test_dist_emulation.py)."""
    lists, s, (want_c, want_d, _) = xc.batch_as_one_set(40, mirrored)
    rc, common, denom, stats = run_emul(emul, lists, s, ranges)
    assert rc == 0 and stats[0] == (ranges or 64) and stats[4] == 0
    bad = np.flatnonzero((common != want_c) | (denom != want_d))
    assert bad.size == 0, (bad[:6], common[bad[:6]], want_c[bad[:6]], denom[bad[:6]], want_d[bad[:6]])


def test_prefilter_takes_a_negative_bound_for_zero(emul):
    """no distance is negative: below 0 the prefilter keeps what it keeps at 0, the identical pairs, however far below -- as it
    stood, 2 exp(k D) - 1 reached 0 at D = -ln 2 / k and the index of the bound went to infinity and then negative, which
    keeps every pair"""
    for k in (11, 21, 32):
        at_zero = emul.emul_tri_jmin(0.0, k)
        assert at_zero == 1.0 - 2.0 ** -30
        for D in (-1e-300, -0.001, -0.03, -0.0331, -0.1, -1.0, -1e9, float("-inf")):
            assert emul.emul_tri_jmin(D, k) == at_zero, (k, D)
    commons, denoms = np.array([0, 5, 999, 1000, 0], np.uint32), np.array([1000, 1000, 1000, 1000, 0], np.uint32)
    keep = np.zeros(5, np.uint8)
    emul.emul_tri_keep_many(commons.ctypes.data, denoms.ctypes.data, 5, emul.emul_tri_jmin(-1.0, 21), keep.ctypes.data)
    assert keep.tolist() == [0, 0, 0, 1, 1]

"""CPU emulation of the medoid kernels (auriclass_amd/csrc/mhx_medoid.h, the very functions the kernels run):
tests/emul/medoid_emul.cpp runs the block predicate next to a brute force over every cell, the sum pass cell by cell in the
kernel's order with the wave's combine on arrays of 64 lanes, the pick, and the pair walk share by share.  Everything against
the rule of tests/medoid_rule.py and the oracle's compare.  A stand-alone program over the same functions runs under the host's
sanitizers (tests/asan/medoid_fuzz.cpp)."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import cluster_cases as cc
from tests import emul_build
from tests import medoid_rule as mr

K = cc.K


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("medoid_emul")
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_medoid_key.argtypes = [u64, u32]
    L.emul_medoid_key.restype = u64
    L.emul_medoid_key_sum.argtypes = [u64]
    L.emul_medoid_key_sum.restype = u64
    L.emul_medoid_key_index.argtypes = [u64]
    L.emul_medoid_key_index.restype = u32
    L.emul_medoid_max_sum.restype = u64
    L.emul_medoid_pair_threads.restype = u32
    L.emul_medoid_first_bad_label.argtypes = [vp, u32]
    L.emul_medoid_first_bad_label.restype = u32
    L.emul_medoid_blocks.argtypes = [vp, u32, u32, vp, vp, u32]
    L.emul_medoid_blocks.restype = u32
    L.emul_medoid_wave.argtypes = [vp, u64, vp, vp]
    L.emul_medoid_wave.restype = u32
    L.emul_medoid_sums.argtypes = [vp, vp, u32, ctypes.c_int, u32, vp, vp, vp, vp]
    L.emul_medoid_sums.restype = u32
    L.emul_medoid_pick.argtypes = [vp, vp, u32, vp]
    L.emul_medoid_pick.restype = None
    L.emul_medoid_pair.argtypes = [vp, u32, vp, u32, u32, u32, vp, vp]
    L.emul_medoid_pair.restype = None
    return L


def random_partition(n, clusters, seed):
    """a seeded partition into `clusters` clusters as a valid label array"""
    of = np.random.default_rng(seed).integers(0, clusters, size=n)
    first = {}
    return np.array([first.setdefault(int(c), i) for i, c in enumerate(of)], np.uint32)


def partitions():
    """(name of the case set, partition name, label)"""
    n200, n150 = len(cc.set200()[0]), len(cc.chains()[0])
    return [("set200", "rule", cc.expected("set200", 0.05)[0].astype(np.uint32)),
            ("chains", "rule", cc.expected("chains", cc.CHAINS_BOUND)[0].astype(np.uint32)),
            ("set200", "singletons", np.arange(n200, dtype=np.uint32)),
            ("set200", "one", np.zeros(n200, np.uint32)),
            ("set200", "seven", random_partition(n200, 7, 77)),
            ("chains", "seven", random_partition(n150, 7, 78))]


def test_key_and_labels(emul):
    top = 65535 << 32
    assert emul.emul_medoid_max_sum() == top == mr.MAX_SUM
    for total, index in ((top, 65535), (0, 0), (12345678901234, 4711)):
        word = emul.emul_medoid_key(total, index)
        assert word == mr.key(total, index) and (emul.emul_medoid_key_sum(word), emul.emul_medoid_key_index(word)) == (total, index)
    assert emul.emul_medoid_key(top, 65535) < (1 << 64) - 1   # below the empty word of the pick
    for label, bad in (([0, 0, 2, 3, 0], 5), ([0, 2, 2, 3, 0], 1), ([0, 0, 1, 3, 0], 2), ([1, 1, 2, 3, 4], 0), ([0, 1, 2, 3, 9], 4), ([], 0)):
        a = np.array(label, np.uint32)
        assert emul.emul_medoid_first_bad_label(a.ctypes.data, a.size) == bad
        assert mr.valid(label) == (bad == len(label))


@pytest.mark.parametrize("qbatch", [48, 65536])
def test_block_predicate_equals_brute_force(emul, qbatch):
    for name, what, label in partitions():
        n = label.size
        runs, brute = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
        nb = emul.emul_medoid_blocks(label.ctypes.data, n, qbatch, runs.ctypes.data, brute.ctypes.data, runs.size)
        assert 0 < nb <= runs.size
        assert np.array_equal(runs[:nb], brute[:nb]), (name, what, qbatch)
        if what == "singletons":
            assert not runs[:nb].any()          # exact, not conservative: no diagonal block of singletons is run
        if what == "one":
            assert runs[:nb].all()
        if (name, what, qbatch) == ("set200", "rule", 48):
            assert 0 < runs[:nb].sum() < nb      # the predicate does select (the chains run through every slice: all of theirs run)
        print(name, what, qbatch, "blocks run", int(runs[:nb].sum()), "of", nb)


def test_wave_combine_on_64_lanes(emul):
    rng = np.random.default_rng(64)

    def run(v, votes):
        row, ref = np.full(2, 1 << 63, np.uint64), np.full(32, 1 << 63, np.uint64)   # a marker where nothing is added
        adds = emul.emul_medoid_wave(v.ctypes.data, votes, row.ctypes.data, ref.ctypes.data)
        return adds, row, ref

    def expect(v, votes):
        row = [int(v[h * 32:(h + 1) * 32].sum()) for h in (0, 1)]
        ref = [int(v[l]) + int(v[l + 32]) for l in range(32)]
        return row, ref

    # the two rows in different clusters: row 0 pairs with references 0 .. 9, row 1 with references 20 .. 31
    v = np.zeros(64, np.uint64)
    v[0:10] = rng.integers(1, 1 << 32, 10, dtype=np.uint64)
    v[32 + 20:64] = rng.integers(1, 1 << 32, 12, dtype=np.uint64)
    votes = sum(1 << l for l in range(64) if v[l])
    adds, row, ref = run(v, votes)
    w_row, w_ref = expect(v, votes)
    assert row.tolist() == w_row and adds == 2 + 22
    assert [int(x) for x in ref] == [w if w else 1 << 63 for w in w_ref]
    # the two rows in the same cluster: both pair with references 3 .. 17, every reference is added once with both values
    v = np.zeros(64, np.uint64)
    v[3:18] = rng.integers(1, 1 << 32, 15, dtype=np.uint64)
    v[32 + 3:32 + 18] = rng.integers(1, 1 << 32, 15, dtype=np.uint64)
    votes = sum(1 << l for l in range(64) if v[l])
    adds, row, ref = run(v, votes)
    w_row, w_ref = expect(v, votes)
    assert row.tolist() == w_row and adds == 2 + 15
    assert [int(x) for x in ref] == [w if w else 1 << 63 for w in w_ref]
    # one big cluster, the largest values: 34 adds, and the sums do not wrap
    v = np.full(64, 1 << 32, np.uint64)
    adds, row, ref = run(v, (1 << 64) - 1)
    assert adds == 34 and row.tolist() == [32 << 32] * 2 and ref.tolist() == [2 << 32] * 32
    # a contributing cell of distance 0 (identical lists) adds nothing and breaks nothing
    v = np.zeros(64, np.uint64)
    adds, row, ref = run(v, 0b1011)
    assert adds == 0


@pytest.mark.parametrize("qbatch", [48, 65536])
def test_sum_pass_and_pick_equal_the_rule(emul, qbatch):
    for name, what, label in partitions():
        lists, s = getattr(cc, name)()
        n = len(lists)
        common, denom, _ = cc.pairs(name)
        total = np.zeros(n, np.uint64)
        adds, most = ctypes.c_uint64(0), ctypes.c_uint32(0)
        run = emul.emul_medoid_sums(common.ctypes.data, denom.ctypes.data, n, K, qbatch, label.ctypes.data, total.ctypes.data, ctypes.byref(adds), ctypes.byref(most))
        want = mr.sums(mr.pair_table(common, denom, n, K), label)
        assert [int(x) for x in total] == want, (name, what)
        assert most.value <= 34
        if what == "singletons":
            assert run == 0 and adds.value == 0
        if what == "one":
            assert sum(int(x) for x in total) == 2 * sum(mr.lr.fixed_distance(int(c), int(d), K) for c, d in zip(common, denom))   # every pair, at both ends
        medoid = np.zeros(n, np.uint32)
        emul.emul_medoid_pick(label.ctypes.data, total.ctypes.data, n, medoid.ctypes.data)
        assert medoid.tolist() == mr.medoids(want, label), (name, what)
        print(name, what, qbatch, "blocks run", run, "adds", adds.value, "most per wave", most.value)


def pair(emul, a, b, shares, s):
    a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
    c, d = ctypes.c_uint32(0), ctypes.c_uint32(0)
    emul.emul_medoid_pair(a.ctypes.data, a.size, b.ctypes.data, b.size, shares, s, ctypes.byref(c), ctypes.byref(d))
    return c.value, d.value


@pytest.mark.parametrize("shares", [1, 16, 1024])
def test_pair_walk_equals_the_oracle(emul, shares):
    assert emul.emul_medoid_pair_threads() == 256
    lists, s = cc.set200()
    empty = np.zeros(0, np.uint64)
    cases = [(lists[5], lists[5], s), (lists[5], lists[190], s),      # identical lists
             (empty, lists[3], s), (lists[3], empty, s), (empty, empty, s),
             (lists[150], lists[3], s), (lists[3], lists[150], s),   # len < s on one side
             (lists[150], lists[150][:9], s),                        # a union smaller than s
             (lists[3], lists[10], s), (lists[3], lists[24], s), (lists[77], lists[141], s), (lists[0], lists[1], s),
             (lists[3], lists[10], 100), (lists[3], lists[10], 1), (lists[3], lists[3], 7)]
    # a shared value whose two copies fall into different shares: two lists of 8 with every value shared, 16 shares of one element
    both = np.arange(1, 9, dtype=np.uint64) * 1000
    cases += [(both, both, 8), (both, both, 5)]
    # a shared value that is exactly the s-th distinct one, and the same one place later (then it does not count)
    a = np.array([1, 3, 5, 7, 9, 20], np.uint64)
    b = np.array([2, 4, 6, 8, 9, 30], np.uint64)
    cases += [(a, b, 9), (a, b, 8), (a, b, 10), (b, a, 9)]
    assert mo.compare(a, b, 9, K)[:2] == (1, 9) and mo.compare(a, b, 8, K)[:2] == (0, 8)
    for x, y, size in cases:
        assert pair(emul, x, y, shares, size) == mo.compare(x, y, size, K)[:2], (len(x), len(y), size, shares)
    # every pair of a slice of the case set, both ways round
    for i in range(0, 40, 3):
        for j in range(1, 40, 7):
            assert pair(emul, lists[i], lists[j], shares, s) == mo.compare(lists[i], lists[j], s, K)[:2], (i, j)


def test_header_functions_under_address_sanitizer(tmp_path):
    """CPU ASan/UBSan build of tests/asan/medoid_fuzz.cpp, a stand-alone program over the same header functions: exact-size
    heap arrays, seeded random partitions and lists; any out-of-bounds access or overflow aborts."""
    import os
    import shutil
    import subprocess
    from pathlib import Path

    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "medoid_fuzz"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(root / "tests" / "asan" / "medoid_fuzz.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime on this host")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"), timeout=120)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout[-500:], r.stderr[-3000:])

"""Medoids of a partition of one sketch set on the GPU (mhx_dist_medoids) and the pair of every list with a target
(mhx_dist_to) against the rule of tests/medoid_rule.py, every comparison an exact integer equality: the labels of the
clustering on the case sets, arbitrary partitions (one cluster of everything, all singletons, a random one), every switch of
the schedule, tiny sets, the device-pointer form (bit for bit the host form, twice) and the argument checks."""
import ctypes
import functools

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from tests import cluster_cases as cc
from tests import medoid_rule as mr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = cc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


@functools.lru_cache(maxsize=None)
def table(name, *args):
    """the fixed-point distances of a case set, once per process"""
    lists, _ = getattr(cc, name)(*args)
    common, denom, _ = cc.pairs(name, K, *args)
    return mr.pair_table(common, denom, len(lists), K)


def rule(name, args, label):
    lists, s = getattr(cc, name)(*args)
    total = mr.sums(table(name, *args), label)
    medoid = mr.medoids(total, label)
    common, denom = mr.dist_to(lists, s, K, medoid)
    return medoid, total, common, denom


def check(got, want):
    for what, g, w in zip(("medoid", "sum", "common", "denom"), got, want):
        g = [int(x) for x in g]
        bad = [i for i in range(len(w)) if g[i] != w[i]]
        assert not bad, (what, bad[:8], [g[i] for i in bad[:8]], [w[i] for i in bad[:8]])


def blocks(lib):
    word = lib.mhx_last_medoid_blocks()
    return word >> 32, word & 0xFFFFFFFF


def run(name, args, label):
    lists, s = getattr(cc, name)(*args)
    M, lens = tc.pad_rows(lists)
    return engine.dist_medoids(M, lens, K, s, np.asarray(label, np.uint32))


def seven(n, seed=77):
    of = np.random.default_rng(seed).integers(0, 7, size=n)
    first = {}
    return np.array([first.setdefault(int(c), i) for i, c in enumerate(of)], np.uint32)


@pytest.mark.parametrize("name,args,bound", [("chains", (), cc.CHAINS_BOUND), ("set70", (), 0.02), ("set200", (), 0.05), ("crowded", (40,), None),
                                             ("long_set", (40, 12_000), None)])
def test_medoids_of_the_clusters_equal_the_rule(lib, name, args, bound):
    if bound is None:
        bound = cc.middle_bound(name, *args)
    label = cc.expected(name, bound, K, *args)[0]
    assert (label != np.arange(label.size)).any()   # the bound does join something
    got = run(name, args, label)
    ran, scheduled = blocks(lib)
    print(name, "blocks run", ran, "of", scheduled, "ranges", lib.mhx_last_dist_ranges(), "fallbacks", lib.mhx_last_dist_fallback_blocks())
    assert 0 < ran <= scheduled
    want = rule(name, args, label)
    check(got, want)
    if name == "chains":
        assert all(want[0][r] != r for r in (0, 1, 4))   # no medoid is its cluster's first member
    if name == "long_set":
        assert lib.mhx_last_dist_ranges() == 1024


def test_arbitrary_partitions(lib):
    lists, s = cc.set200()
    n = len(lists)
    # one cluster of everything: every block runs, all 19 900 pairs count, the disjoint ones with the full 2^32
    got = run("set200", (), np.zeros(n, np.uint32))
    ran, scheduled = blocks(lib)
    assert ran == scheduled > 0
    want = rule("set200", (), [0] * n)
    check(got, want)
    common, denom, _ = cc.pairs("set200")
    assert int((common == 0).sum()) > 1000 and sum(want[1]) == 2 * sum(table("set200")[i][j] for i in range(n) for j in range(i))
    assert len(set(want[0])) == 1
    # all singletons: nothing of the triangle is launched
    got = run("set200", (), np.arange(n, dtype=np.uint32))
    assert blocks(lib)[0] == 0 and blocks(lib)[1] == scheduled
    assert got[0].tolist() == list(range(n)) and not got[1].any()
    check(got, rule("set200", (), list(range(n))))
    assert got[2].tolist() == got[3].tolist() == [min(len(v), s) for v in lists]   # every list against itself
    # a seeded partition into seven clusters that has nothing to do with the distances
    label = seven(n)
    assert mr.valid(label) and len(set(label.tolist())) == 7
    check(run("set200", (), label), rule("set200", (), label.tolist()))


@pytest.mark.parametrize("env,ranges", [({"MHX_TRI_QBATCH": "48"}, 64), ({"MHX_TRI_GEOMETRY": "dist"}, 1024), ({"MHX_DIST_GENERIC": "1"}, 0)])
@pytest.mark.parametrize("name,bound", [("chains", cc.CHAINS_BOUND), ("set200", 0.05)])
def test_the_switches_of_the_schedule(lib, monkeypatch, name, bound, env, ranges):
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    label = cc.expected(name, bound)[0]
    got = run(name, (), label)
    ran, scheduled = blocks(lib)
    print(name, env, "blocks run", ran, "of", scheduled)
    assert lib.mhx_last_dist_ranges() == ranges and 0 < ran <= scheduled
    if "MHX_TRI_QBATCH" in env:
        assert scheduled > 5   # clusters straddle blocks
    check(got, rule(name, (), label))


def test_tiny_sets(lib):
    lists, s = cc.set70()
    M, lens = tc.pad_rows(lists[:3])
    got = engine.dist_medoids(M[:0], lens[:0], K, s, np.zeros(0, np.uint32))
    assert all(a.size == 0 for a in got)
    got = engine.dist_medoids(M[:1].copy(), lens[:1].copy(), K, s, [0])
    assert [a.tolist() for a in got] == [[0], [0], [len(lists[0])], [len(lists[0])]] and blocks(lib) == (0, 0)
    empty = np.zeros(0, np.uint64)
    M1, lens1 = tc.pad_rows([empty])
    assert [a.tolist() for a in engine.dist_medoids(M1, lens1, K, s, [0])] == [[0], [0], [0], [0]]
    # two lists in one cluster: the two sums are equal, the lower index wins
    for pair in ((lists[0], lists[1]), (lists[1], lists[0]), (lists[0], lists[11]), (empty, lists[0]), (empty, empty)):
        pairs = tc.oracle_pairs(pair, s, K)
        M2, lens2 = tc.pad_rows(pair)
        for label in ([0, 0], [0, 1]):
            want = mr.medoids_of(pair, s, K, label, pairs)
            assert want[1][0] == want[1][1] and want[0] == ([0, 0] if label == [0, 0] else [0, 1])
            check(engine.dist_medoids(M2, lens2, K, s, label), want)
    three = (lists[0], lists[1], lists[2])
    pairs = tc.oracle_pairs(three, s, K)
    for label in ([0, 0, 0], [0, 0, 2], [0, 1, 0], [0, 1, 1], [0, 1, 2]):
        check(engine.dist_medoids(M, lens, K, s, label), mr.medoids_of(three, s, K, label, pairs))


def test_dist_to_any_target(lib):
    lists, s = cc.set70()
    n = len(lists)
    M, lens = tc.pad_rows(lists)
    rng = np.random.default_rng(70)
    target = rng.integers(0, n, size=n).astype(np.uint32)
    target[0:8] = np.arange(8)            # itself
    target[8:16] = [0, 3, 20, 21, 5, 1, 2, 7]   # a lower index (the empty and the short list among them)
    target[16:24] = [69, 40, 20, 21, 66, 23, 33, 50]   # a higher one
    target[20], target[21], target[40] = 20, 0, 15   # the empty list against itself; the exact duplicate against its original
    common, denom = engine.dist_to(M, lens, K, s, target)
    want = mr.dist_to(lists, s, K, target)
    assert common.tolist() == want[0] and denom.tolist() == want[1]
    assert (common[20], denom[20]) == (0, 0) and common[40] == denom[40] == len(lists[15])
    # a smaller sketch size than the lists hold: the cut lies inside both lists
    common, denom = engine.dist_to(M, lens, K, 100, target)
    want = mr.dist_to(lists, 100, K, target)
    assert common.tolist() == want[0] and denom.tolist() == want[1]


def test_device_pointers_equal_the_host_form_bit_for_bit(lib):
    dev = f"cuda:{torch.cuda.current_device()}"
    lists, s = cc.set200()
    n = len(lists)
    M, lens = tc.pad_rows(lists)
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    for label in (cc.expected("set200", 0.05)[0].astype(np.uint32), seven(n)):
        host = engine.dist_medoids(M, lens, K, s, label)
        d_label = torch.from_numpy(label.view(np.int32)).to(dev)
        outs = []
        for _ in range(2):
            medoid, common, denom = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(3))
            total = torch.full((n,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ran = engine.dist_medoids_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, d_label.data_ptr(), medoid.data_ptr(), total.data_ptr(),
                                             common.data_ptr(), denom.data_ptr())
            assert ran > 0
            outs.append((medoid.cpu().numpy().view(np.uint32), total.cpu().numpy().view(np.uint64), common.cpu().numpy().view(np.uint32),
                         denom.cpu().numpy().view(np.uint32)))
        for out in outs:
            assert all(np.array_equal(a, b) for a, b in zip(out, host))
        check(outs[0], rule("set200", (), label.tolist()))
        # the medoids alone: sum, common and denom NULL
        medoid = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        engine.dist_medoids_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, d_label.data_ptr(), medoid.data_ptr())
        assert np.array_equal(medoid.cpu().numpy().view(np.uint32), host[0])
        # the pair kernel with device pointers: every list against its medoid
        common, denom = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        d_target = torch.from_numpy(host[0].view(np.int32)).to(dev)
        torch.cuda.synchronize()
        engine.dist_to_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, d_target.data_ptr(), common.data_ptr(), denom.data_ptr())
        assert np.array_equal(common.cpu().numpy().view(np.uint32), host[2]) and np.array_equal(denom.cpu().numpy().view(np.uint32), host[3])
    # a bad label on the device is refused by the host's check: nothing is launched
    bad = np.arange(n, dtype=np.uint32)
    bad[7] = 9
    d_bad = torch.from_numpy(bad.view(np.int32)).to(dev)
    medoid = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_medoids_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, d_bad.data_ptr(), medoid.data_ptr())
    assert exc.value.code == engine.MHX_E_ARG and (medoid.cpu().numpy() == -1).all()


def test_bad_arguments_are_refused_before_anything_is_launched(lib):
    lists, s = cc.set70()
    M, lens = tc.pad_rows(lists[:5])
    medoid, common, denom = (np.full(8, 0xFFFFFFFF, np.uint32) for _ in range(3))
    total = np.zeros(8, np.uint64)
    good = np.array([0, 0, 2, 2, 0], np.uint32)

    def medoids(label=good, n=5, s_=s, k=K, rows=M, ln=lens, med=medoid, c=common, d=denom):
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.mhx_dist_medoids(p(rows), p(ln), n, M.shape[1], k, s_, p(label), p(med), total.ctypes.data, p(c), p(d), 0)

    def to(target, n=5, s_=s, rows=M, c=common, d=denom):
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.mhx_dist_to(p(rows), p(lens), n, M.shape[1], K, s_, p(target), p(c), p(d), 0)

    for label in ([0, 2, 2, 3, 0], [0, 0, 1, 3, 0], [0, 0, 2, 2, 5], [0, 0, 2, 2, 0xFFFFFFFF], [1, 1, 2, 3, 4]):
        assert medoids(np.array(label, np.uint32)) == engine.MHX_E_ARG and b"label[" in lib.mhx_last_error(), label
    assert (medoid == 0xFFFFFFFF).all()
    assert medoids(s_=1 << 20) == engine.MHX_E_ARG and b"sketch size" in lib.mhx_last_error()
    assert medoids(n=65537, rows=None, ln=None) == engine.MHX_E_ARG
    assert medoids(rows=None) == engine.MHX_E_ARG and medoids(ln=None) == engine.MHX_E_ARG
    assert medoids(label=None) == engine.MHX_E_ARG and medoids(med=None) == engine.MHX_E_ARG
    assert medoids(c=None) == engine.MHX_E_ARG and b"go together" in lib.mhx_last_error()
    assert medoids(d=None) == engine.MHX_E_ARG and b"go together" in lib.mhx_last_error()
    for k_bad, s_bad in ((0, s), (33, s), (K, 0)):
        assert medoids(k=k_bad, s_=s_bad) == engine.MHX_E_ARG
    assert medoids(n=1, rows=None) == engine.MHX_E_ARG   # a single list is still looked at
    for target in ([0, 1, 2, 3, 5], [0xFFFFFFFF, 0, 0, 0, 0]):
        assert to(np.array(target, np.uint32)) == engine.MHX_E_ARG and b"target[" in lib.mhx_last_error()
    assert to(good, s_=1 << 20) == engine.MHX_E_ARG
    assert to(good, n=65537, rows=None) == engine.MHX_E_ARG
    assert to(None) == engine.MHX_E_ARG and to(good, rows=None) == engine.MHX_E_ARG and to(good, c=None) == engine.MHX_E_ARG and to(good, d=None) == engine.MHX_E_ARG
    assert (common == 0xFFFFFFFF).all() and (denom == 0xFFFFFFFF).all()
    # and the good call goes through: sum NULL, the pairs asked for
    assert lib.mhx_dist_medoids(M.ctypes.data, lens.ctypes.data, 5, M.shape[1], K, s, good.ctypes.data, medoid.ctypes.data, None, common.ctypes.data,
                                denom.ctypes.data, 0) == engine.MHX_OK
    want = mr.medoids_of(lists[:5], s, K, good.tolist(), tc.oracle_pairs(lists[:5], s, K))
    assert medoid[:5].tolist() == want[0] and common[:5].tolist() == want[2] and denom[:5].tolist() == want[3]

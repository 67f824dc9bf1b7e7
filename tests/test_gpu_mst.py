"""The single-linkage tree of one sketch set on the GPU (mhx_dist_mst) against the rule of tests/mst_rule.py -- Kruskal over
the oracle's pairs in the exact edge order: edges, their order and their distances in both pair sources (stored and
recomputed), under each switch of the triangle's schedule, through the larger geometries and the fallback to the generic
kernel, the device-pointer form (the same set twice), the cut against mhx_dist_cluster, tiny sets and the argument checks."""
import math

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from tests import cluster_rule as cr
from tests import mst_cases as mc
from tests import mst_rule as mr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = mc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(lists, s, k=K):
    M, lens = tc.pad_rows(lists)
    return engine.dist_mst(M, lens, k, s)


def check(lib, got, tree, n, k=K):
    """edges and their order equal the rule's, dist equals the oracle's double, the rounds stay within the cap"""
    ei, ej, ec, ed, dist = got
    rounds = lib.mhx_last_mst_rounds()
    print("edges", ei.size, "rounds", rounds)
    assert ei.size == len(tree) == n - 1
    rows = list(zip(ei.tolist(), ej.tolist(), ec.tolist(), ed.tolist()))
    bad = [t for t in range(len(tree)) if rows[t] != tree[t]]
    assert not bad, (bad[:5], [rows[t] for t in bad[:5]], [tree[t] for t in bad[:5]])
    assert np.array_equal(dist, mr.distances(tree, k))
    assert 1 <= rounds <= max(1, math.ceil(math.log2(n)))


def check_source(lib, monkeypatch_store):
    assert lib.mhx_last_mst_stored() == int(monkeypatch_store)   # the pair source that was asked for is the one that ran


@pytest.mark.parametrize("store", ["1", "0"])
@pytest.mark.parametrize("name,args", mc.CASES)
def test_edges_order_and_distances_equal_the_rule(lib, monkeypatch, name, args, store):
    monkeypatch.setenv("MHX_MST_STORE", store)
    lists, s = mc.lists_of(name, args)
    got = run(lists, s)
    check(lib, got, mc.expected(name, args), len(lists))
    check_source(lib, store)
    if name == "crowded" and store == "0":
        assert lib.mhx_last_dist_fallback_blocks() > 0   # the generic kernel redoes the blocks, every round
    if name == "identical":
        assert (got[0] == np.arange(1, 70)).all() and (got[1] == 0).all()   # the star at list 0


@pytest.mark.parametrize("store", ["1", "0"])
@pytest.mark.parametrize("name,env,ranges", [("chains", {"MHX_TRI_QBATCH": "48"}, 64), ("chains", {"MHX_TRI_GEOMETRY": "dist"}, 1024),
                                             ("set200", {"MHX_TRI_QBATCH": "48"}, 64), ("set200", {"MHX_TRI_GEOMETRY": "dist"}, 1024)])
def test_the_switches_of_the_schedule(lib, monkeypatch, name, env, ranges, store):
    monkeypatch.setenv("MHX_MST_STORE", store)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    lists, s = mc.lists_of(name)
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    check(lib, got, mc.expected(name), len(lists))
    check_source(lib, store)


@pytest.mark.parametrize("store", ["1", "0"])
def test_longer_lists_take_the_windowed_finish(lib, monkeypatch, store):
    monkeypatch.setenv("MHX_MST_STORE", store)
    lists, s = mc.long_set(40, 20_000)
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == 2048 and lib.mhx_last_dist_fallback_blocks() == 0
    check(lib, got, mc.expected("long_set", (40, 20_000)), 40)
    check_source(lib, store)


def test_the_generic_kernel_alone_feeds_the_recomputed_rounds(lib, monkeypatch):
    """MHX_DIST_GENERIC=1 on set200, recomputed: no value ranges, the blocks go through the generic pair kernel alone (the
    counters say 0 ranges and -1 fallbacks) and run again every round, from the second on over flag words that a round
    before has used.  The tree is the rule's and, edge for edge, the one the stored source gives on the fast path."""
    lists, s = mc.set200()
    monkeypatch.setenv("MHX_MST_STORE", "1")
    stored = run(lists, s)
    check_source(lib, "1")
    monkeypatch.setenv("MHX_MST_STORE", "0")
    monkeypatch.setenv("MHX_DIST_GENERIC", "1")
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1
    check(lib, got, mc.expected("set200"), len(lists))
    check_source(lib, "0")
    assert all(np.array_equal(a, b) for a, b in zip(got, stored))


def test_the_budget_chooses_the_pair_source(lib, monkeypatch):
    """set200 holds 19 900 pairs, 159 200 bytes: a budget of 0 MB recomputes, 1 MB and the default store, and MHX_MST_STORE
    overrides the budget either way; mhx_last_mst_stored() tells which ran, and all give the rule's tree"""
    lists, s = mc.set200()
    for force, mb, stored in ((None, "0", 0), (None, "1", 1), (None, None, 1), ("1", "0", 1), ("0", None, 0)):
        for var, value in (("MHX_MST_STORE", force), ("MHX_MST_STORE_MB", mb)):
            if value is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, value)
        check(lib, run(lists, s), mc.expected("set200"), len(lists))
        assert lib.mhx_last_mst_stored() == stored, (force, mb)
    # 70 lists hold 2415 pairs, 19 320 bytes: they fit 1 MB; nothing fits 0 MB, and a call that launches nothing says -1
    monkeypatch.delenv("MHX_MST_STORE", raising=False)
    monkeypatch.setenv("MHX_MST_STORE_MB", "1")
    run(*mc.set70())
    assert lib.mhx_last_mst_stored() == 1
    M, lens = tc.pad_rows(lists[:1])
    engine.dist_mst(M, lens, K, s)
    assert lib.mhx_last_mst_stored() == -1 and lib.mhx_last_mst_rounds() == 0


@pytest.mark.parametrize("store", ["1", "0"])
def test_device_pointers_give_the_same_set_twice(lib, monkeypatch, store):
    monkeypatch.setenv("MHX_MST_STORE", store)
    dev = f"cuda:{torch.cuda.current_device()}"
    lists, s = mc.set200()
    M, lens = tc.pad_rows(lists)
    n = len(lists)
    host = engine.dist_mst(M, lens, K, s)
    want = sorted(zip(host[0].tolist(), host[1].tolist(), host[2].tolist(), host[3].tolist()))
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    for with_dist in (True, False, True):
        outs = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev) for _ in range(4)]
        dist = torch.full((n - 1,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        m = engine.dist_mst_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, *(o.data_ptr() for o in outs),
                                   dist.data_ptr() if with_dist else 0)
        assert m == n - 1 and lib.mhx_last_dist_kernel_ms() > 0
        check_source(lib, store)
        ei, ej, ec, ed = (o.cpu().numpy().view(np.uint32) for o in outs)
        assert sorted(zip(ei.tolist(), ej.tolist(), ec.tolist(), ed.tolist())) == want
        if with_dist:   # the device's log: within a few ulp of the oracle's double
            w = np.array([cr.distance(c, d, K) for c, d in zip(ec.tolist(), ed.tolist())])
            assert np.allclose(dist.cpu().numpy(), w, rtol=1e-12, atol=1e-15)
        else:
            assert (dist.cpu().numpy() == -1.0).all()


def test_cut_equals_dist_cluster(lib):
    """mst_labels of the tree against engine.dist_cluster: six bounds on set200, every distinct distance of set70 and the
    double just below it"""
    for name, bounds in (("set200", [-0.1, 0.0, 0.005, 0.02, 0.05, 1.0]), ("set70", None)):
        lists, s = mc.lists_of(name)
        n = len(lists)
        M, lens = tc.pad_rows(lists)
        ei, ej, ec, ed, _ = engine.dist_mst(M, lens, K, s)
        if bounds is None:
            distinct = np.unique(mc.pairs(name)[2])
            bounds = [b for T in distinct.tolist() for b in (T, float(np.nextafter(T, -np.inf)))]
        for bound in bounds:
            want_label, _, want_clusters, _ = engine.dist_cluster(M, lens, K, s, bound)
            label, clusters = engine.mst_labels(ei, ej, ec, ed, n, K, bound)
            assert clusters == want_clusters and np.array_equal(label, want_label), (name, bound)


def test_tiny_sets_and_bad_arguments(lib):
    lists, s = mc.set70()
    M, lens = tc.pad_rows(lists[:5])
    for n in (0, 1):
        got = engine.dist_mst(M[:n], lens[:n], K, s)
        assert all(a.size == 0 for a in got)
    ei, ej, ec, ed, dist = engine.dist_mst(M[:2], lens[:2], K, s)
    c, d, dd = mc.pairs("set70")
    assert (ei.tolist(), ej.tolist(), ec.tolist(), ed.tolist(), dist.tolist()) == ([1], [0], [int(c[0])], [int(d[0])], [float(dd[0])])
    assert lib.mhx_last_mst_rounds() == 1
    # refused before anything is launched
    out = np.full(8, 77, np.uint32)

    def call(n, k=K, s_=s, rows=M, ln=lens, o=out, oi=out):
        p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
        return lib.mhx_dist_mst(p(rows), p(ln), n, M.shape[1], k, s_, p(oi), p(o), p(o), p(o), None, 0)
    assert call(5, s_=1 << 20) == engine.MHX_E_ARG and b"sketch size too large" in lib.mhx_last_error()
    assert call(1, s_=1 << 20) == engine.MHX_E_ARG
    was = int(lens[3])
    lens[3] = M.shape[1] + 1
    assert call(5) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    lens[3] = was
    assert call(65537, rows=None, ln=None) == engine.MHX_E_ARG
    for k, s_bad in ((0, s), (33, s), (K, 0)):
        assert call(5, k=k, s_=s_bad) == engine.MHX_E_ARG
    assert call(5, rows=None) == engine.MHX_E_ARG and call(5, ln=None) == engine.MHX_E_ARG
    assert call(5, o=None) == engine.MHX_E_ARG and call(5, oi=None) == engine.MHX_E_ARG
    assert (out == 77).all()
    assert call(5) == engine.MHX_OK

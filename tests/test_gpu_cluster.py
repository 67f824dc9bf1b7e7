"""Single-linkage clustering of one sketch set on the GPU (mhx_dist_cluster) against the rule of tests/cluster_rule.py --
edges by the oracle's distance, components by breadth-first search: labels, degrees and both counts at bounds from "no edge"
to "every pair", the bound exactly at and just below every distance that occurs, chains whose every union is indispensable
under each switch of the schedule, the larger geometries, the fallback to the generic kernel, the device-pointer form
(exact and repeatable as well), tiny sets and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import cluster_cases as cc
from tests import cluster_rule as cr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = cc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(lists, s, max_dist, k=K):
    M, lens = tc.pad_rows(lists)
    return engine.dist_cluster(M, lens, k, s, max_dist)


def check(got, want):
    (label, degree, clusters, n_edges), (w_label, w_degree, w_clusters, w_edges) = got, want
    print("clusters", clusters, "of the rule", w_clusters, "edges", n_edges, "of the rule", w_edges)
    assert (clusters, n_edges) == (w_clusters, w_edges)
    bad = np.flatnonzero(label != w_label)
    assert bad.size == 0, (bad[:8], label[bad[:8]], w_label[bad[:8]])
    bad = np.flatnonzero(degree != w_degree)
    assert bad.size == 0, (bad[:8], degree[bad[:8]], w_degree[bad[:8]])


@pytest.mark.parametrize("max_dist", [-0.1, 0.0, 0.005, 0.02, 0.05, 1.0])
@pytest.mark.parametrize("name", ["set70", "set200"])
def test_labels_degrees_and_counts_equal_the_rule(lib, name, max_dist):
    lists, s = getattr(cc, name)()
    got = run(lists, s, max_dist)
    assert lib.mhx_last_dist_ranges() == 64 and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, cc.expected(name, max_dist))
    n = len(lists)
    if max_dist < 0:
        assert got[2] == n and got[3] == 0
    if max_dist >= 1:
        assert got[2] == 1 and got[3] == n * (n - 1) // 2 and (got[1] == n - 1).all()


def test_the_bound_is_exact_at_every_distance_that_occurs(lib):
    """max_dist at each distinct distance of the 70-list set and at the double just below it: the edges are the oracle
    distances <= the bound to the pair -- no prefilter's slack, no other log than the host's"""
    lists, s = cc.set70()
    pairs = cc.pairs("set70")
    distinct = np.unique(pairs[2])
    assert distinct.size == 48
    M, lens = tc.pad_rows(lists)
    for T in distinct.tolist():
        for bound in (T, float(np.nextafter(T, -np.inf))):
            label, degree, clusters, n_edges = engine.dist_cluster(M, lens, K, s, bound)
            assert n_edges == int((pairs[2] <= bound).sum()), (T, bound)
            w_label, w_degree, w_clusters, _ = cr.cluster(lists, s, K, bound, pairs)
            assert clusters == w_clusters and np.array_equal(label, w_label) and np.array_equal(degree, w_degree), (T, bound)


@pytest.mark.parametrize("name,env,ranges", [("chains", {}, 64), ("chains", {"MHX_TRI_QBATCH": "48"}, 64), ("chains", {"MHX_TRI_GEOMETRY": "dist"}, 1024),
                                             ("set200", {"MHX_TRI_QBATCH": "48"}, 64)])
def test_chains_and_the_switches_of_the_schedule(lib, monkeypatch, name, env, ranges):
    """chains(): 144 edges, each the only link between the two halves of its chain, every chain through all five slices"""
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    bound = cc.CHAINS_BOUND if name == "chains" else 0.02
    lists, s = getattr(cc, name)()
    got = run(lists, s, bound)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, cc.expected(name, bound))
    if name == "chains":
        assert (got[2], got[3]) == (6, 144)


@pytest.mark.parametrize("length,ranges", [(12_000, 1024), (20_000, 2048)])
def test_longer_lists_take_the_base_and_the_windowed_finish(lib, length, ranges):
    lists, s = cc.long_set(40, length)
    bound = cc.middle_bound("long_set", 40, length)
    got = run(lists, s, bound)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    want = cc.expected("long_set", bound, K, 40, length)
    assert 0 < want[3] < 10   # the bound splits the ten close copies
    check(got, want)


def test_crowded_values_fall_back_and_count_once(lib):
    """the range pass gives its blocks up, the generic kernel redoes them, and each is taken out once: no degree doubled"""
    lists, s = cc.crowded(40)
    bound = cc.middle_bound("crowded", 40)
    got = run(lists, s, bound)
    assert lib.mhx_last_dist_fallback_blocks() > 0
    want = cc.expected("crowded", bound, K, 40)
    assert want[3] > 0 and got[1].sum() == 2 * want[3]
    check(got, want)


def test_device_pointers_are_exact_and_repeatable(lib):
    dev = f"cuda:{torch.cuda.current_device()}"
    lists, s = cc.set200()
    M, lens = tc.pad_rows(lists)
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    n = len(lists)
    for bound in (0.02, 0.05):
        host = engine.dist_cluster(M, lens, K, s, bound)
        outs = []
        for _ in range(2):
            label = torch.full((n,), -1, dtype=torch.int32, device=dev)
            degree = torch.full((n,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            clusters, n_edges = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, bound, label.data_ptr(), degree.data_ptr())
            assert lib.mhx_last_dist_kernel_ms() > 0
            outs.append((label.cpu().numpy().view(np.uint32), degree.cpu().numpy().view(np.uint32), clusters, n_edges))
        check(outs[0], host)   # element for element the host form, which is the rule's
        check(outs[0], cc.expected("set200", bound))
        check(outs[1], outs[0])
        label = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, bound, label.data_ptr(), 0) == outs[0][2:]   # degree == NULL
        assert np.array_equal(label.cpu().numpy().view(np.uint32), outs[0][0])


def test_device_pointers_from_the_segmented_sketch(lib):
    """40 records of one stream, sketched record by record on the device (sketch_segments_device) and clustered without a
    host round trip; the oracle sketches every record on its own"""
    rng = np.random.default_rng(4040)
    k, s, stride = 21, 200, 208
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = [rng.choice(acgt, size=int(n)) for n in rng.integers(300, 3000, size=40)]
    for i in range(5, 40, 5):   # some records are near copies of the one before
        src = recs[i - 1].copy()
        at = rng.integers(0, src.size, size=max(1, src.size // (20 * i)))
        src[at] = rng.choice(acgt, size=at.size)
        recs[i] = src
    recs[12] = recs[11].copy()
    recs[20] = recs[20][:k + 3]
    data = b"".join(r.tobytes() for r in recs)
    off = np.zeros(41, np.uint64)
    off[1:] = np.cumsum([r.size for r in recs], dtype=np.uint64)
    dev = f"cuda:{torch.cuda.current_device()}"
    d_bytes = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    n = 40
    d_rows = torch.zeros((n, stride), dtype=torch.int64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    label = torch.full((n,), -1, dtype=torch.int32, device=dev)
    degree = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), n, k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
    clusters, n_edges = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s, 0.1, label.data_ptr(), degree.data_ptr())
    sketches = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in recs]
    want = cr.cluster(sketches, s, k, 0.1)
    assert 0 < want[3] < n * (n - 1) // 2
    check((label.cpu().numpy().view(np.uint32), degree.cpu().numpy().view(np.uint32), clusters, n_edges), want)


def test_tiny_sets_and_bad_arguments(lib):
    lists, s = cc.set70()
    M, lens = tc.pad_rows(lists[:1])
    label, degree, clusters, n_edges = engine.dist_cluster(M[:0], lens[:0], K, s, 0.05)
    assert label.size == 0 and (clusters, n_edges) == (0, 0)
    M1, lens1 = M.copy(), lens.copy()
    label, degree, clusters, n_edges = engine.dist_cluster(M1, lens1, K, s, 0.05)
    assert label.tolist() == [0] and degree.tolist() == [0] and (clusters, n_edges) == (1, 0)
    empty = np.zeros(0, np.uint64)
    for pair, bound, joined in (((lists[0], lists[1]), 0.05, True), ((lists[0], lists[1]), 0.0, False), ((lists[0], lists[11]), 0.05, False),
                                ((empty, empty), 0.0, True), ((empty, empty), -1e-300, False), ((empty, lists[0]), 0.999, False),
                                ((empty, lists[0]), 1.0, True)):
        want = cr.cluster(pair, s, K, bound)
        assert (want[2] == 1) == joined
        check(run(pair, s, bound), want)
    # refused before anything is launched
    clusters, n_edges = ctypes.c_uint32(9), ctypes.c_uint64(9)
    out = np.zeros(8, np.uint32)
    M, lens = tc.pad_rows(lists[:5])

    def call(n, max_dist, k=K, s_=s, rows=M, ln=lens):
        return lib.mhx_dist_cluster(rows.ctypes.data if rows is not None else None, ln.ctypes.data if ln is not None else None, n, M.shape[1], k, s_, max_dist,
                                    out.ctypes.data, None, ctypes.byref(clusters), ctypes.byref(n_edges), 0)
    assert call(5, float("nan")) == engine.MHX_E_ARG and b"not a number" in lib.mhx_last_error()
    was = int(lens[3])
    lens[3] = M.shape[1] + 1
    assert call(5, 0.05) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    lens[3] = was
    assert call(65537, 0.05, rows=None, ln=None) == engine.MHX_E_ARG
    for k, s_bad in ((0, s), (33, s), (K, 0)):
        assert call(5, 0.05, k=k, s_=s_bad) == engine.MHX_E_ARG
    assert call(5, 0.05, rows=None) == engine.MHX_E_ARG
    assert lib.mhx_dist_cluster(M.ctypes.data, lens.ctypes.data, 5, M.shape[1], K, s, 0.05, None, None, ctypes.byref(clusters), ctypes.byref(n_edges), 0) == engine.MHX_E_ARG
    assert call(5, 0.05) == engine.MHX_OK and (clusters.value, n_edges.value) == cr.cluster(lists[:5], s, K, 0.05)[2:]
    assert np.array_equal(out[:5], cr.cluster(lists[:5], s, K, 0.05)[0])

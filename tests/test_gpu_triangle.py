"""All pairs within one sketch set on the GPU (mhx_dist_triangle, mhx_dist_triangle_edges) against the oracle's
compareSketches of every pair j < i: every geometry the rule gives (64, 1024 and 2048 value ranges), both forms of the
range pass, query batches, the fallback of crowded values to the generic kernel, the argument checks, the edge list with
its capacity protocol, and the device-pointer form fed by the segmented sketch."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import cluster_rule as cr
from tests import mst_rule as mr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = 21


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(lists, s, k=K):
    M, lens = tc.pad_rows(lists)
    return engine.dist_triangle(M, lens, k, s)


def check(got, want):
    (c, d, x), (wc, wd, wx) = got, want
    bad = np.flatnonzero((c != wc) | (d != wd))
    assert bad.size == 0, (bad[:5], c[bad[:5]], wc[bad[:5]], d[bad[:5]], wd[bad[:5]])
    assert np.array_equal(x.view(np.uint64), wx.view(np.uint64))   # host libm on the same counts: bit for bit


def test_seventy_lists_sixty_four_ranges(lib):
    """three slices, the last partial; every block has fewer than 128 queries: the slice-per-wave range kernel"""
    lists, s = tc.set70()
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == 64 and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, tc.expected("set70"))


@pytest.mark.parametrize("env,ranges", [({}, 64), ({"MHX_TRI_QBATCH": "48"}, 64), ({"MHX_TRI_GEOMETRY": "dist"}, 1024)])
def test_two_hundred_lists(lib, monkeypatch, env, ranges):
    """the first slices have 128 queries and more (one query per lane), the last ones fewer; in batches of 48 queries; and
    with the geometry of mhx_dist_batch (1024 ranges, the base finish)"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    lists, s = tc.set200()
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, tc.expected("set200"))


@pytest.mark.parametrize("length,ranges", [(12_000, 1024), (20_000, 2048)])
def test_longer_lists_take_the_base_and_the_windowed_finish(lib, length, ranges):
    lists, s = tc.long_set(40, length)
    got = run(lists, s)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, tc.expected("long_set", K, 40, length))


def test_crowded_values_fall_back_and_stay_exact(lib):
    """the non-uniform construction of the distance tests: the range pass gives its blocks up, the generic kernel redoes them"""
    lists, s = tc.crowded(40)
    got = run(lists, s)
    assert lib.mhx_last_dist_fallback_blocks() > 0
    check(got, tc.expected("crowded", K, 40))


def test_flagged_blocks_in_both_groups_of_flag_words(lib, monkeypatch):
    """The group boundary of the all-pairs schedule (tests/triangle_cases.py: flagged_groups): 512 lists at s = 64, one query
    per block, 4336 blocks, the last 240 in a second group of flag words, and two slices crowded into one value range, one of
    them with blocks in both groups.  The flagged blocks are exactly those of the two slices, 447 + 63; a flag word left
    standing across the boundary would count as one more.  The dense triangle, the clustering (whose flatten pass follows the
    last block of a slice and of a group) and the tree from the recomputed pairs (the blocks once per round, the words
    cleared in front of the first group from the second round on) ride the same blocks."""
    monkeypatch.setenv("MHX_TRI_QBATCH", "1")
    lists, s = tc.flagged_groups()
    n = len(lists)
    want = tc.expected("flagged_groups")
    block, r0 = tc.flagged_groups_blocks(n)
    for lo in (64, 448):
        assert len(np.unique(np.concatenate(lists[lo:lo + 32]))) > 1536   # more keys than a range table holds
    assert block.max() + 1 == 4336 > 4096
    shares = want[0] > 0
    assert (shares & (r0 == 64)).any() and (shares & (r0 == 448)).any() and (shares & (block >= 4096)).any()
    M, lens = tc.pad_rows(lists)
    got = engine.dist_triangle(M, lens, K, s)
    print("ranges", lib.mhx_last_dist_ranges(), "fallback blocks", lib.mhx_last_dist_fallback_blocks())
    assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == 447 + 63
    check(got, want)
    label, degree, clusters, n_edges = engine.dist_cluster(M, lens, K, s, 0.05)
    assert lib.mhx_last_dist_fallback_blocks() == 447 + 63
    w_label, w_degree, w_clusters, w_edges = cr.cluster(lists, s, K, 0.05, want)
    assert (clusters, n_edges) == (w_clusters, w_edges) and np.array_equal(label, w_label) and np.array_equal(degree, w_degree)
    monkeypatch.setenv("MHX_MST_STORE", "0")
    ei, ej, ec, ed, dist = engine.dist_mst(M, lens, K, s)
    assert lib.mhx_last_mst_stored() == 0 and lib.mhx_last_dist_fallback_blocks() == 447 + 63   # counted in the first round only
    tree = mr.kruskal(want[0], want[1], n)
    assert list(zip(ei.tolist(), ej.tolist(), ec.tolist(), ed.tolist())) == tree
    assert np.array_equal(dist, mr.distances(tree, K))


def test_tiny_sets_and_bad_arguments(lib):
    lists, s = tc.set70()
    for n in (0, 1):
        M, lens = tc.pad_rows(lists[:1])
        c, d, x = engine.dist_triangle(M[:n], lens[:n], K, s)
        assert c.size == d.size == x.size == 0
    c, d, x = run(lists[:2], s)
    wc, wd, wx = mo.compare(lists[1], lists[0], s, K)
    assert (int(c[0]), int(d[0]), float(x[0])) == (wc, wd, wx) and c.size == 1
    found = ctypes.c_uint64(99)
    assert lib.mhx_dist_triangle_edges(None, None, 1, 16, K, s, 0.5, None, None, None, None, None, 0, ctypes.byref(found), 0) == engine.MHX_OK
    assert found.value == 0
    M, lens = tc.pad_rows(lists[:5])
    lens[3] = M.shape[1] + 1
    out = np.zeros(10, np.uint32)
    assert lib.mhx_dist_triangle(M.ctypes.data, lens.ctypes.data, 5, M.shape[1], K, s, out.ctypes.data, out.ctypes.data, None, 0) == engine.MHX_E_ARG
    assert b"exceeds stride" in lib.mhx_last_error()
    assert lib.mhx_dist_triangle(None, None, 65537, 16, K, s, None, None, None, 0) == engine.MHX_E_ARG   # before anything is launched
    assert lib.mhx_dist_triangle_edges(None, None, 65537, 16, K, s, 0.5, None, None, None, None, None, 0, ctypes.byref(found), 0) == engine.MHX_E_ARG
    lens[3] = 5
    for k, s_bad in ((0, s), (33, s), (K, 0)):
        assert lib.mhx_dist_triangle(M.ctypes.data, lens.ctypes.data, 5, M.shape[1], k, s_bad, out.ctypes.data, out.ctypes.data, None, 0) == engine.MHX_E_ARG


@pytest.mark.parametrize("D", [0.0, 0.02, 0.2, 1.0])
def test_edges_equal_the_oracles_filter(lib, D):
    lists, s = tc.set200()
    wc, wd, wx = tc.expected("set200")
    n = len(lists)
    ii = np.array([i for i in range(n) for j in range(i)], np.uint32)
    jj = np.array([j for i in range(n) for j in range(i)], np.uint32)
    keep = wx <= D   # packed order is ascending (i, j)
    M, lens = tc.pad_rows(lists)
    ei, ej, c, d, x = engine.dist_triangle_edges(M, lens, K, s, D)
    assert keep.sum() > 0 and (D == 1.0 or keep.sum() < keep.size)
    assert np.array_equal(ei, ii[keep]) and np.array_equal(ej, jj[keep])
    assert np.array_equal(c, wc[keep]) and np.array_equal(d, wd[keep])
    assert np.array_equal(x.view(np.uint64), wx[keep].view(np.uint64))
    # a buffer that is too small: the exact count comes back, and the retry with it succeeds
    small = [np.zeros(3, np.uint32) for _ in range(4)]
    found = ctypes.c_uint64(0)
    rc = lib.mhx_dist_triangle_edges(M.ctypes.data, lens.ctypes.data, n, M.shape[1], K, s, D, *[a.ctypes.data for a in small], None, 3,
                                     ctypes.byref(found), 0)
    assert keep.sum() > 3 and rc == engine.MHX_E_CAPACITY and found.value == keep.sum()
    ei2, ej2, c2, d2, _ = engine.dist_triangle_edges(M, lens, K, s, D, cap=3)
    assert np.array_equal(ei2, ei) and np.array_equal(ej2, ej) and np.array_equal(c2, c) and np.array_equal(d2, d)


def test_device_pointers_from_the_segmented_sketch(lib):
    """40 records of one stream, sketched record by record on the device (sketch_segments_device), compared with each other
    without a host round trip; the oracle sketches every record on its own and compares."""
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
    pairs = n * (n - 1) // 2
    common = torch.zeros(pairs, dtype=torch.int32, device=dev)
    denom = torch.zeros(pairs, dtype=torch.int32, device=dev)
    dist = torch.zeros(pairs, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), n, k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
    ms = engine.dist_triangle_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s, common.data_ptr(), denom.data_ptr(), dist.data_ptr())
    # stride 208 <= 16 x 16: 16 ranges.  Records of 300 .. 3000 bases keep the 200 smallest of 280 .. 2980 hashes, so the lists'
    # maxima differ tenfold and the long records crowd the lowest range: the slice of 32 may go to the generic kernel
    assert ms > 0 and lib.mhx_last_dist_ranges() in (0, 16) and lib.mhx_last_dist_fallback_blocks() in (0, 1, 2)
    sketches = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in recs]
    wc, wd, wx = tc.oracle_pairs(sketches, s, k)
    common, denom, dist = common.cpu().numpy(), denom.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(common.view(np.uint32), wc) and np.array_equal(denom.view(np.uint32), wd)
    assert np.all(np.abs(dist - wx) <= 2e-16 * np.maximum(1.0, np.abs(wx)) + 1e-300)   # device log(): <= 1 ulp (as tests/test_gpu_segments.py)
    # the edge list on the device: prefiltered only, in the order of arrival
    cap = 256
    ei = torch.zeros(cap, dtype=torch.int32, device=dev)
    ej = torch.zeros(cap, dtype=torch.int32, device=dev)
    ec = torch.zeros(cap, dtype=torch.int32, device=dev)
    ed = torch.zeros(cap, dtype=torch.int32, device=dev)
    ex = torch.zeros(cap, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    m = engine.dist_triangle_edges_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s, 0.1, ei.data_ptr(), ej.data_ptr(), ec.data_ptr(),
                                          ed.data_ptr(), ex.data_ptr(), cap)
    ii = np.array([i for i in range(n) for j in range(i)])
    jj = np.array([j for i in range(n) for j in range(i)])
    keep = wx <= 0.1
    assert m == keep.sum() and 0 < m < cap
    got = sorted(zip(ei.cpu().numpy()[:m].tolist(), ej.cpu().numpy()[:m].tolist(), ec.cpu().numpy()[:m].tolist(), ed.cpu().numpy()[:m].tolist()))
    assert got == list(zip(ii[keep].tolist(), jj[keep].tolist(), wc[keep].tolist(), wd[keep].tolist()))

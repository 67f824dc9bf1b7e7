"""The distance kernels at the hash values that uniform draws never produce (tests/extreme_cases.py), through every consumer
of the range table -- mhx_dist_batch in its four range-pass forms and in the windowed form, mhx_dist_triangle with its edge
mode, mhx_dist_search in both geometries and with device pointers -- against the oracle's compareSketches of every pair,
in exact integers:

    2^64 - 1   kEmptyKey, the vacant-slot marker of the range table, as a hash: in references 0 / 8 (wave 0 inserts both, in
               program order, in every form) next to values of the same home slot, in queries, and in two lists that differ
               in that value alone
    0          in zero-padded rows, where only the length tells it from padding
    tiny       every value below the number of value ranges: shift 0
    2^b - 1, 2^b   as the largest value of a call, b = 40

No case may pass because the generic pair kernel did the work: the range pass must have run (mhx_last_dist_ranges() != 0)
and no block may have fallen back.  (A block that holds 2^64 - 1 would be allowed to; the table keeps that value in a mask
word of its own instead, so none does.)"""
import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from tests import extreme_cases as xc
from tests import search_cases as sc
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = xc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def on_the_fast_path(lib, ranges=None):
    got = lib.mhx_last_dist_ranges()
    assert got != 0 and (ranges is None or got == ranges), got
    assert lib.mhx_last_dist_fallback_blocks() == 0


def rows_of(qrys, refs, extra=0):
    stride = (max(max(map(len, qrys)), max(map(len, refs)), 1) + 15) // 16 * 16 + extra
    return tc.pad_rows(qrys, stride) + tc.pad_rows(refs, stride)


def same_matrix(got, want, what):
    common, denom, dist = got
    bad = np.argwhere((common != want[0]) | (denom != want[1]))
    assert bad.size == 0, (what, [(int(q), int(r), int(common[q, r]), int(want[0][q, r]), int(denom[q, r]), int(want[1][q, r])) for q, r in bad[:6]])
    assert np.array_equal(dist.view(np.uint64), want[2].view(np.uint64))   # host libm on the same counts: bit for bit


def same_triangle(got, want):
    (c, d, x), (wc, wd, wx) = got, want
    bad = np.flatnonzero((c != wc) | (d != wd))
    assert bad.size == 0, (bad[:6], c[bad[:6]], wc[bad[:6]], d[bad[:6]], wd[bad[:6]])
    assert np.array_equal(x.view(np.uint64), wx.view(np.uint64))


def same_lists(got, want):
    assert np.array_equal(got[4], want[4]), ("n_hits", np.flatnonzero(got[4] != want[4])[:5])
    for name, a, b in zip(("ref", "common", "denom"), got[:3], want[:3]):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (name, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))


# ---- 2^64 - 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("form", ["lane", "lane64", "walk", "wave"])
def test_dist_batch_forms_with_the_vacant_slot_marker(lib, monkeypatch, form, mirrored):
    """150 queries against 33 references (two slices, the second of one list) in the forms that
    test_dist_one_query_per_lane_forms_equal_oracle (tests/test_gpu_parity.py) selects, selected the same way"""
    if form == "walk":
        monkeypatch.setenv("MHX_DIST_WALK_MIN", "128")
    if form == "wave":
        monkeypatch.setenv("MHX_DIST_NO_LANE", "1")
    qrys, refs, s = xc.batch(150, mirrored)
    assert xc.holders(refs) == [8 if mirrored else 0] and xc.holders(qrys) == [1, 6]
    Q, ql, R, rl = rows_of(qrys, refs, 8 if form == "lane64" else 0)
    got = engine.dist_batch(Q, ql, R, rl, K, s)
    on_the_fast_path(lib, 1024)
    same_matrix(got, xc.batch_expected(150, mirrored), (form, mirrored))


def long_planted(n, nrefs, length, mirrored=False):
    """tc.long_set cut into references and queries and planted; s = 3 x length, so that the union of a pair stays below s
    and the top range counts"""
    lists, _ = tc.long_set(n, length)
    refs, qrys = xc.plant(list(lists[:nrefs]), list(lists[nrefs:]), mirrored)
    return qrys, refs, 3 * length


def test_dist_batch_windowed_form_with_the_vacant_slot_marker(lib):
    """lists of 70 000 hashes: 2048 value ranges, window totals and the wide finish"""
    qrys, refs, s = long_planted(28, 18, 70_000)
    Q, ql, R, rl = rows_of(qrys, refs)
    got = engine.dist_batch(Q, ql, R, rl, K, s)
    on_the_fast_path(lib, 2048)
    same_matrix(got, xc.oracle_matrix(qrys, refs, s), "windowed")


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("env,ranges", [({}, 64), ({"MHX_TRI_GEOMETRY": "dist"}, 1024)])
def test_triangle_with_the_vacant_slot_marker(lib, monkeypatch, env, ranges, mirrored):
    """the 33 references and 40 queries as one set of 73 lists (three slices); lists 0, 8 and 16 are references of the first"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    lists, s, want = xc.batch_as_one_set(40, mirrored)
    M, lens = tc.pad_rows(lists)
    got = engine.dist_triangle(M, lens, K, s)
    on_the_fast_path(lib, ranges)
    same_triangle(got, want)


def test_triangle_and_search_windowed_finish_with_the_vacant_slot_marker(lib):
    """one tc.long_set(40, 20 000)-sized case: 2048 ranges from the triangle's rule, window totals and the wide finish"""
    qrys, refs, s = long_planted(40, 20, 20_000)
    lists = refs + qrys
    M, lens = tc.pad_rows(lists)
    got = engine.dist_triangle(M, lens, K, s)
    on_the_fast_path(lib, 2048)
    same_triangle(got, tc.oracle_pairs(lists, s, K))
    Q, ql, R, rl = rows_of(qrys, refs)
    got = engine.dist_search(Q, ql, R, rl, K, s, 5, 1.0)
    on_the_fast_path(lib, 2048)
    same_lists(got, sc.lists_from(*xc.oracle_matrix(qrys, refs, s), 5, 1.0))


@pytest.mark.parametrize("mirrored", [False, True])
def test_triangle_edges_with_the_vacant_slot_marker(lib, mirrored):
    D = 0.05
    lists, s, (wc, wd, wx) = xc.batch_as_one_set(40, mirrored)
    n = len(lists)
    ii = np.array([i for i in range(n) for j in range(i)], np.uint32)
    jj = np.array([j for i in range(n) for j in range(i)], np.uint32)
    keep = wx <= D
    assert 0 < keep.sum() < keep.size
    M, lens = tc.pad_rows(lists)
    ei, ej, c, d, x = engine.dist_triangle_edges(M, lens, K, s, D)
    on_the_fast_path(lib, 64)
    assert np.array_equal(ei, ii[keep]) and np.array_equal(ej, jj[keep])
    assert np.array_equal(c, wc[keep]) and np.array_equal(d, wd[keep])
    assert np.array_equal(x.view(np.uint64), wx[keep].view(np.uint64))


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("env,ranges", [({}, 64), ({"MHX_SEARCH_GEOMETRY": "dist"}, 1024)])
def test_search_with_the_vacant_slot_marker(lib, monkeypatch, env, ranges, mirrored):
    """top = 5: the pairs the construction is about are among a query's best (query 0 derives from reference 0, query 6 is the
    holder of 2^64 - 1 itself, and query 1's single shared hash with it outranks every pair without one); top = 33 lists
    every pair"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    qrys, refs, s = xc.batch(40, mirrored)
    want = xc.batch_expected(40, mirrored)
    Q, ql, R, rl = rows_of(qrys, refs)
    for top in (5, 33):
        got = engine.dist_search(Q, ql, R, rl, K, s, top, 1.0)
        on_the_fast_path(lib, ranges)
        same_lists(got, sc.lists_from(*want, top, 1.0))


def test_search_device_pointers_rows_that_end_in_the_vacant_slot_marker(lib):
    """rows built on the host and handed over as device pointers, as a segmented sketch on the device hands over a row it
    ended in 2^64 - 1; max_dist = 1: the prefilter keeps every pair, the lists are the rule's"""
    top = 5
    qrys, refs, s = xc.batch(40)
    want = sc.lists_from(*xc.batch_expected(40), top, 1.0)
    Q, ql, R, rl = rows_of(qrys, refs)
    assert Q[1, ql[1] - 1] == np.uint64(xc.EMPTY) and R[0, rl[0] - 1] == np.uint64(xc.EMPTY)
    dev = f"cuda:{torch.cuda.current_device()}"
    d_q, d_r = torch.from_numpy(Q.view(np.int64)).to(dev), torch.from_numpy(R.view(np.int64)).to(dev)
    d_ql, d_rl = torch.from_numpy(ql.view(np.int32)).to(dev), torch.from_numpy(rl.view(np.int32)).to(dev)
    nq, nr = len(qrys), len(refs)
    out = [torch.full((nq, top), 7, dtype=torch.int32, device=dev) for _ in range(3)]
    dist = torch.full((nq, top), -1.0, dtype=torch.float64, device=dev)
    n_hits = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ms = engine.dist_search_device(d_q.data_ptr(), d_ql.data_ptr(), nq, d_r.data_ptr(), d_rl.data_ptr(), nr, Q.shape[1], K, s, top, 1.0,
                                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dist.data_ptr(), n_hits.data_ptr())
    assert ms > 0
    on_the_fast_path(lib, 64)   # the row stride (1008) bounds the lengths: the geometry of lists of 1000
    n = n_hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(n, want[4]) and (n == top).all()
    for a, b in zip(out, want[:3]):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b)
    x, wx = dist.cpu().numpy(), want[3]
    assert np.all(np.abs(x - wx) <= 2e-16 * np.maximum(1.0, np.abs(wx)) + 1e-300)   # device log(): <= 1 ulp (as tests/test_gpu_search.py)


# ---- the neighbouring values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,args,batch_ranges,set_ranges", [("with_zero", (), 1024, 64), ("below_the_ranges", (1024, 300, 1000), 1024, 64),
                                                               ("below_the_ranges", (16, 10, 16), 1024, 16),
                                                               ("power_of_two_top", (40, False), 1024, 64), ("power_of_two_top", (40, True), 1024, 64)])
def test_values_uniform_draws_never_produce(lib, case, args, batch_ranges, set_ranges):
    """hash 0 in zero-padded rows; every value below 1024 (shift 0 in mhx_dist_batch) and below 16 (shift 0 in every geometry);
    the largest value of the call exactly 2^40 - 1 and exactly 2^40 -- through the batch, the triangle and the search, with
    no block handed to the generic kernel"""
    qrys, refs, s = getattr(xc, case)(*args)
    want = xc.oracle_matrix(qrys, refs, s)
    Q, ql, R, rl = rows_of(qrys, refs)
    got = engine.dist_batch(Q, ql, R, rl, K, s)
    on_the_fast_path(lib, batch_ranges)
    same_matrix(got, want, case)
    got = engine.dist_search(Q, ql, R, rl, K, s, 5, 1.0)
    on_the_fast_path(lib, set_ranges)
    same_lists(got, sc.lists_from(*want, 5, 1.0))
    lists = refs + qrys
    M, lens = tc.pad_rows(lists)
    got = engine.dist_triangle(M, lens, K, s)
    on_the_fast_path(lib, set_ranges)
    same_triangle(got, tc.oracle_pairs(lists, s, K))

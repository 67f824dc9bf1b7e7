"""The containment search on the GPU (mhx_dist_contain_search) against the rule of tests/contain_search_rule.py over the rule of
the containment, every integer exact: the pair kernel alone, the range route at 16, 64 and 1024 value ranges (no block may
fall back there), flagged blocks whose take-out is deferred, a pair without a geometry, the tie case across three slices, a
call that crosses the group of 4096 blocks, the device-pointer form twice, the tie to mhx_dist_contain, the argument checks."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_contain.py: the two then share one device runtime

from auriclass_amd import engine
from tests import contain_cases as cc
from tests import contain_search_cases as csc
from tests import contain_search_rule as rule
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = cc.K
FORMS = ((5, 0.0, 1), (64, 0.0, 1), (1, 0.0, 1), (5, 0.95, 3), (7, 1.0, 1))   # (top, min_identity, min_shared)


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def rows_of(name):
    if name == "ties":
        return csc.rows()
    return cc.crafted_rows() if name == "crafted" else cc.rows_of(name)


def counts_of(name):
    return csc.expected() if name == "ties" else cc.expected(name)


def same(got, want, what=""):
    for name, a, b in zip(("ref", "shared", "n_ref", "n_qry", "n_hits"), got, want):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def check(lib, name, forms=FORMS, ranges=None, fallbacks=None):
    Q, q_len, R, r_len, s_q, s_r = rows_of(name)
    for top, min_identity, min_shared in forms:
        got = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, top, min_identity, min_shared)
        if ranges is not None:
            assert lib.mhx_last_dist_ranges() == ranges
        if fallbacks is not None:
            assert fallbacks(lib.mhx_last_dist_fallback_blocks())
        same(got, rule.arrays(rule.search(*counts_of(name), K, top, min_identity, min_shared), top), (name, top, min_identity, min_shared))


def test_pair_kernel_on_the_crafted_edge_cases(lib):
    """6 x 5 (tests/contain_cases.py: crafted_rows): 30 pairs go through the pair kernel per block, with the same take-out"""
    check(lib, "crafted", ranges=0, fallbacks=lambda f: f == -1)
    hits = rule.search(*cc.expected("crafted"), K, 5)
    assert [h[0] for h in hits[1]][:1] == [1] and hits[0] == [] and hits[3] == []   # the identical short list; the empty and the disjoint query


@pytest.mark.parametrize("name,env,ranges", [("small", {}, 16), ("mixed", {}, 64), ("mixed", {"MHX_SEARCH_QBATCH": "13"}, 64),
                                             ("mixed", {"MHX_SEARCH_GEOMETRY": "dist"}, 1024), ("set200", {}, 64), ("extreme", {}, 64)])
def test_range_route(lib, monkeypatch, name, env, ranges):
    """small: 16 ranges; mixed: 64 ranges, two slices, the second of one reference, also in query batches of 13 (a best list is
    carried across batches and slices) and at the distance path's 1024 ranges; set200: seven slices; extreme: 2^64 - 1 as a hash.
    No block falls back, so the pair kernel cannot have made the lists."""
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    check(lib, name, ranges=ranges, fallbacks=lambda f: f == 0)


@pytest.mark.parametrize("name", ["crowded", "plasmids"])
def test_flagged_blocks_are_taken_out_later(lib, name):
    """blocks whose flag went up are redone by the pair kernel behind their group and taken out then: the lists are the rule's"""
    check(lib, name, fallbacks=lambda f: f > 0)
    if name == "plasmids":   # what min_shared is for: reference 0 lies inside query 0's genome, and one hash of it inside the window
        Q, q_len, R, r_len, s_q, s_r = rows_of(name)
        ref, shared, n_ref, n_qry, n_hits = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, 2)
        assert n_hits[0] == 1 and (ref[0, 0], shared[0, 0], n_ref[0, 0], n_qry[0, 0]) == (0, 1, 1, 1000)
        assert (n_hits[2], ref[2, 0], shared[2, 0]) == (1, 8, 1000) and n_hits[1] == 0   # the full list of query 2's own genome
        assert engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, 2, min_shared=2)[4].tolist() == [0, 0, 1, 1, 0, 0, 0, 0]


def test_a_pair_without_a_geometry(lib):
    """70 000 entries: above the base form of the range route"""
    check(lib, "long_pair", forms=((5, 0.0, 1), (1, 0.999, 1)), ranges=0, fallbacks=lambda f: f == -1)


@pytest.mark.parametrize("top", [1, 2, 5, 64])
def test_ties_across_three_slices(lib, top):
    """references 3, 35 and 67 are one list, one in every slice: only the index orders them, whichever slice arrives when"""
    check(lib, "ties", forms=((top, 0.0, 1), (top, 0.9, 1)), ranges=64, fallbacks=lambda f: f == 0)
    Q, q_len, R, r_len, s_q, s_r = rows_of("ties")
    ref = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, top)[0]
    assert ref[0].tolist()[:5] == [3, 11, 35, 67, 10][:top] and ref[1, 0] == 3


def test_more_blocks_than_one_group(lib, monkeypatch):
    """8 x 16 640 lists of 16 hashes with one query per block: 4160 blocks, 64 more than the group whose flag words come back
    together -- the words are reset between the groups and the last query's list goes on growing in the second.  The
    expectation is the rule, vectorised (tests/contain_search_cases.py, tests/contain_search_rule.py: search_np)."""
    monkeypatch.setenv("MHX_SEARCH_QBATCH", "1")
    Q, q_len, R, r_len, s_q, s_r = csc.many_blocks()
    counts = csc.many_blocks_expected()
    for top, min_identity, min_shared in ((5, 0.0, 1), (64, 0.9, 2)):
        got = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, top, min_identity, min_shared)
        assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == 0   # (32 lists of 16 hashes cannot crowd a range)
        same(got, rule.search_np(*counts, rule.need_table(16, K, min_identity, min_shared), top), (top, min_identity))
        assert (got[0][:, 0] == 16000 + np.arange(8)).all() and (got[1][:, 0] == 16).all()   # every query's own list, planted behind block 4096 of the last


def test_flagged_blocks_in_both_groups_of_flag_words(lib, monkeypatch):
    """The case above cannot raise a flag, so it cannot see a flag word left standing between the groups.  This one can
    (tests/contain_search_cases.py: flagged_groups): 150 x 900 at s = 64, one query per block, 4350 blocks, and slice 27 crowded
    into one value range -- exactly one fallback per query, in the first group and in the second.  A word that was not reset
    would flag another block of the second group and count one more."""
    monkeypatch.setenv("MHX_SEARCH_QBATCH", "1")
    qs, rs, s, _ = csc.flagged_groups()
    Q, q_len = tc.pad_rows(list(qs), 64)
    R, r_len = tc.pad_rows(list(rs), 64)
    counts = csc.flagged_groups_expected()
    for top, min_identity, min_shared in ((5, 0.0, 1), (3, 0.9, 2)):
        got = engine.dist_contain_search(Q, q_len, R, r_len, s, s, K, top, min_identity, min_shared)
        assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == len(qs)   # slice 27 once per query
        want = rule.arrays(rule.search(*counts, K, top, min_identity, min_shared), top)
        assert want[0][145, 0] == 870 and want[0][147, 0] == 880
        same(got, want, (top, min_identity))


def test_device_pointers_twice_against_the_host_form(lib):
    """everything on the device, lengths above the sketch size and above the stride included (the kernels clip what the host
    form refuses); the first n_hits entries are the host form's, exactly, and the second run's are the first's"""
    dev = torch.device("cuda")
    for name, top, min_identity in (("mixed", 5, 0.9), ("crafted", 64, 0.0), ("ties", 3, 0.0)):
        Q, q_len, R, r_len, s_q, s_r = rows_of(name)
        host = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, top, min_identity)
        same(host, rule.arrays(rule.search(*counts_of(name), K, top, min_identity), top), name)
        lying_q, lying_r = q_len.copy(), r_len.copy()
        lying_q[q_len >= s_q] = 0xFFFFFFF0   # a full list whose length lies: the stride and s bound it
        lying_r[r_len >= s_r] = Q.shape[1] + 5
        d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, lying_q, R, lying_r)]
        nq, nr = len(q_len), len(r_len)
        runs = []
        for _ in range(2):
            out = [torch.full((nq, top), 7, dtype=torch.int32, device=dev) for _ in range(4)] + [torch.full((nq,), 7, dtype=torch.int32, device=dev)]
            torch.cuda.synchronize()
            ms = engine.dist_contain_search_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, Q.shape[1], K, top,
                                                   min_identity, 1, *[o.data_ptr() for o in out])
            assert ms > 0
            got = [o.cpu().numpy().view(np.uint32) for o in out]
            assert np.array_equal(got[4], host[4])
            live = np.arange(top)[None, :] < got[4][:, None]
            for a, b in zip(got[:4], host[:4]):
                assert np.array_equal(a[live], b[live]), name
            runs.append([np.where(live, a, 0) for a in got[:4]] + [got[4]])
        same(runs[1], runs[0], name)


@pytest.mark.parametrize("name", ["mixed", "small", "crafted", "plasmids_swapped"])
def test_the_hits_are_the_pairs_of_dist_contain(lib, name):
    """nr <= 64, top = 64, min_shared = 1, min_identity = 0: the hits of every query are exactly the pairs of
    engine.dist_contain with shared > 0, in rule order"""
    Q, q_len, R, r_len, s_q, s_r = rows_of(name)
    assert len(r_len) <= 64
    shared, n_qry, n_ref = engine.dist_contain(Q, q_len, R, r_len, s_q, s_r)
    ref, hs, hr, hq, n_hits = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, 64)
    for q in range(len(q_len)):
        want = rule.ranked([(r, int(shared[q, r]), int(n_ref[q, r]), int(n_qry[q, r])) for r in range(len(r_len)) if shared[q, r] > 0])
        got = list(zip(ref[q, :n_hits[q]].tolist(), hs[q, :n_hits[q]].tolist(), hr[q, :n_hits[q]].tolist(), hq[q, :n_hits[q]].tolist()))
        assert got == want, (name, q)


def test_argument_checks(lib):
    Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows()

    def refused(**kw):
        a = dict(s_q=s_q, s_r=s_r, k=K, top=5, min_identity=0.0, min_shared=1, q_len=q_len, r_len=r_len)
        a.update(kw)
        with pytest.raises(engine.EngineError) as e:
            engine.dist_contain_search(Q, a["q_len"], R, a["r_len"], a["s_q"], a["s_r"], a["k"], a["top"], a["min_identity"], a["min_shared"])
        assert e.value.code == engine.MHX_E_ARG, kw
        return e.value.message

    for bad in (dict(top=0), dict(top=65), dict(min_shared=0), dict(min_identity=float("nan")), dict(k=0), dict(k=33), dict(s_q=0), dict(s_r=0)):
        refused(**bad)
    too_long = q_len.copy()
    too_long[3] = Q.shape[1] + 1
    assert "q_len[3]" in refused(q_len=too_long)
    too_long = r_len.copy()
    too_long[1] = R.shape[1] + 1
    assert "r_len[1]" in refused(r_len=too_long)
    v = ctypes.c_void_p
    out = np.full((6, 5), 9, np.uint32)
    n_hits = np.full(6, 9, np.uint32)
    p = lambda a: v(a.ctypes.data)
    call = lambda q, ql, nq, r, rl, nr, stride, o, nh: lib.mhx_dist_contain_search(q, ql, nq, s_q, r, rl, nr, s_r, stride, K, 0.0, 1, 5, o, p(out), p(out), p(out), nh, 0)
    assert call(p(Q), p(q_len), 6, p(R), p(r_len), 5, 0, p(out), p(n_hits)) == engine.MHX_E_ARG    # stride 0
    assert call(p(Q), p(q_len), 6, p(R), p(r_len), 5, 24, None, p(n_hits)) == engine.MHX_E_ARG   # a null output
    assert call(p(Q), p(q_len), 6, p(R), p(r_len), 5, 24, p(out), None) == engine.MHX_E_ARG
    assert (out == 9).all() and (n_hits == 9).all()
    # no queries: a successful no-op that touches nothing; no references: n_hits zeroed, the lists untouched
    assert call(None, None, 0, p(R), p(r_len), 5, 24, p(out), p(n_hits)) == 0
    assert (out == 9).all() and (n_hits == 9).all()
    assert call(p(Q), p(q_len), 6, None, None, 0, 24, p(out), p(n_hits)) == 0
    assert (out == 9).all() and (n_hits == 0).all()
    # an identity bound above 1: no hits, and zeros behind n_hits in the host form
    got = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, 5, 1.0000001)
    assert not got[4].any() and not any(a.any() for a in got[:4])

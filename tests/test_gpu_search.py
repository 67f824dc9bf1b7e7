"""The reference-set search on the GPU (mhx_dist_search) against the rule of tests/search_rule.py over the oracle's
compareSketches of every pair: the shared case set at every `top` and bound, both forms of the range pass, query batches
that carry a list across blocks, both geometries, reference counts around a slice, the base and the windowed finish, the
fallback of crowded values to the generic kernel, the argument checks, and the device-pointer form fed by the segmented
sketch."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import search_cases as sc
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = sc.K
BOUNDS = [0.0, 0.05, 1.0]


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(qs, rs, s, top, max_dist, k=K):
    stride = (max(max(map(len, qs)), max(map(len, rs)), 1) + 15) // 16 * 16
    Q, ql = tc.pad_rows(qs, stride)
    R, rl = tc.pad_rows(rs, stride)
    return engine.dist_search(Q, ql, R, rl, k, s, top, max_dist)


def check(got, want):
    names = ("ref", "common", "denom")
    assert np.array_equal(got[4], want[4]), ("n_hits", np.flatnonzero(got[4] != want[4])[:5])
    for name, a, b in zip(names, got[:3], want[:3]):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (name, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))   # host libm on the same counts: bit for bit


@pytest.mark.parametrize("top", [1, 5, 64])
@pytest.mark.parametrize("max_dist", BOUNDS)
def test_case_set(lib, top, max_dist):
    """150 queries: the one-query-per-lane range pass; seven slices, the last of 8 references"""
    refs, s = sc.references()
    want = sc.expected(top, max_dist)
    hits = [sc.hits_per_query(d) for d in BOUNDS]   # over the three bounds every `top` meets truncated, short and empty lists
    assert any((h > top).any() for h in hits) and any(((h > 0) & (h <= top)).any() for h in hits) and any((h == 0).any() for h in hits)
    if (top, max_dist) == (5, 0.05):
        assert (hits[1] > top).any() and ((hits[1] > 0) & (hits[1] <= top)).any() and (hits[1] == 0).any()   # all three in ONE call
    got = run(sc.queries(), refs, s, top, max_dist)
    assert lib.mhx_last_dist_ranges() == 64 and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, want)


@pytest.mark.parametrize("nq,env,ranges", [(40, {}, 64), (40, {"MHX_SEARCH_QBATCH": "13"}, 64), (150, {"MHX_SEARCH_QBATCH": "48"}, 64),
                                           (150, {"MHX_SEARCH_GEOMETRY": "dist"}, 1024), (40, {"MHX_SEARCH_GEOMETRY": "dist", "MHX_SEARCH_QBATCH": "7"}, 1024)])
def test_query_batches_and_geometries(lib, monkeypatch, nq, env, ranges):
    """40 queries: the slice-per-wave range pass; small batches carry a query's list across batches and slices; the
    geometry of mhx_dist_batch (1024 ranges, the base finish)"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    refs, s = sc.references()
    hits = sc.hits_per_query(0.05, nq)
    assert (hits > 5).any() and ((hits > 0) & (hits <= 5)).any() and (hits == 0).any()
    for top, max_dist in ((5, 0.05), (64, 1.0), (1, 0.0)):
        got = run(sc.queries()[:nq], refs, s, top, max_dist)
        assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
        check(got, sc.expected(top, max_dist, nq))


@pytest.mark.parametrize("nr", [1, 3, 31, 32, 33])
def test_reference_counts_around_a_slice(lib, nr):
    refs, s = sc.references()
    for top, max_dist in ((5, 1.0), (5, 0.05), (64, 1.0)):
        got = run(sc.queries(), refs[:nr], s, top, max_dist)
        check(got, sc.expected(top, max_dist, sc.NQ, nr))
        if max_dist == 1.0:
            assert (got[4] == min(top, nr)).all()   # fewer references than `top`: all of them, no more


@pytest.mark.parametrize("length,ranges", [(12_000, 1024), (20_000, 2048)])
def test_longer_lists_take_the_base_and_the_windowed_finish(lib, length, ranges):
    lists, s = tc.long_set(40, length)
    qs, rs = lists[:20], lists[20:]
    common, denom, dist = sc.oracle_matrix(qs, rs, s, K)
    for top, max_dist in ((3, 1.0), (20, 0.2)):
        got = run(qs, rs, s, top, max_dist)
        assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
        check(got, sc.lists_from(common, denom, dist, top, max_dist))


def test_crowded_values_fall_back_and_stay_exact(lib):
    """the non-uniform construction of the distance tests: the range pass gives the block up, the generic kernel redoes it and
    its take-out runs then"""
    lists, s = tc.crowded(40)
    qs, rs = lists[:20], lists[20:]
    common, denom, dist = sc.oracle_matrix(qs, rs, s, K)
    for top, max_dist in ((5, 1.0), (20, 0.02)):
        got = run(qs, rs, s, top, max_dist)
        assert lib.mhx_last_dist_fallback_blocks() > 0
        check(got, sc.lists_from(common, denom, dist, top, max_dist))


def test_empty_sets_and_bad_arguments(lib):
    refs, s = sc.references()
    Q, ql = tc.pad_rows(sc.queries()[:5], 1008)
    R, rl = tc.pad_rows(refs[:5], 1008)
    out = [np.full((5, 5), 9, np.uint32) for _ in range(3)]
    n_hits = np.full(5, 9, np.uint32)

    def call(q=Q, qlen=ql, nq=5, r=R, rlen=rl, nr=5, stride=1008, k=K, s_=s, max_dist=1.0, top=5, outs=None, n=n_hits):
        o = [a.ctypes.data for a in out] if outs is None else outs
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.mhx_dist_search(p(q), p(qlen), nq, p(r), p(rlen), nr, stride, k, s_, max_dist, top, o[0], o[1], o[2], None, p(n), 0)

    assert call(nq=0) == engine.MHX_OK and (n_hits == 9).all()
    assert call(nq=0, q=None, qlen=None, n=None, outs=[None] * 3) == engine.MHX_OK
    assert call(nr=0) == engine.MHX_OK and (n_hits == 0).all()   # no references: every query has no hits
    for bad in (dict(top=0), dict(top=65), dict(max_dist=float("nan")), dict(k=0), dict(k=33), dict(s_=0), dict(stride=0), dict(q=None),
                dict(qlen=None), dict(r=None), dict(rlen=None), dict(n=None), dict(outs=[None, out[1].ctypes.data, out[2].ctypes.data])):
        assert call(**bad) == engine.MHX_E_ARG, bad
    long = ql.copy()
    long[3] = 1009
    assert call(qlen=long) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    long = rl.copy()
    long[4] = 2000
    assert call(rlen=long) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    assert call() == engine.MHX_OK and (n_hits == 5).all()   # five references, top = 5 (25 pairs: the generic kernel alone)
    assert lib.mhx_last_dist_fallback_blocks() == -1
    want = sc.expected(5, 1.0, 5, 5)
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and np.array_equal(out[2], want[2])


def records(rng, n, k):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [rng.choice(acgt, size=int(m)) for m in rng.integers(300, 3000, size=n)], acgt


def test_device_pointers_from_the_segmented_sketch(lib):
    """two streams of about 40 records, sketched record by record on the device (sketch_segments_device); one is the queries,
    the other the references, some records of one near copies of records of the other; nothing returns to the host in
    between.  The oracle sketches every record on its own; the rule over its pairs is what the device lists must hold."""
    rng = np.random.default_rng(4141)
    k, s, stride, top, D = 21, 200, 208, 5, 0.1
    ref_recs, acgt = records(rng, 41, k)
    qry_recs, _ = records(rng, 38, k)
    for i in range(0, 38, 3):   # near copies of references, some of the same one
        src = ref_recs[(i * 5) % 12].copy()
        at = rng.integers(0, src.size, size=max(1, src.size // (15 * (i + 1))))
        src[at] = rng.choice(acgt, size=at.size)
        qry_recs[i] = src
    for j in range(13, 20):     # and more than `top` references close to query 0
        src = ref_recs[0].copy()
        at = rng.integers(0, src.size, size=j)
        src[at] = rng.choice(acgt, size=at.size)
        ref_recs[j] = src
    ref_recs[30] = ref_recs[3].copy()
    qry_recs[20] = qry_recs[20][:k + 3]
    dev = f"cuda:{torch.cuda.current_device()}"

    def sketch(recs):
        data = b"".join(r.tobytes() for r in recs)
        off = np.zeros(len(recs) + 1, np.uint64)
        off[1:] = np.cumsum([r.size for r in recs], dtype=np.uint64)
        d_bytes = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_rows = torch.zeros((len(recs), stride), dtype=torch.int64, device=dev)
        d_len = torch.zeros(len(recs), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), len(recs), k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
        return d_rows, d_len

    q_rows, q_len = sketch(qry_recs)
    r_rows, r_len = sketch(ref_recs)
    nq, nr = len(qry_recs), len(ref_recs)
    out = [torch.full((nq, top), 7, dtype=torch.int32, device=dev) for _ in range(3)]
    dist = torch.full((nq, top), -1.0, dtype=torch.float64, device=dev)
    n_hits = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ms = engine.dist_search_device(q_rows.data_ptr(), q_len.data_ptr(), nq, r_rows.data_ptr(), r_len.data_ptr(), nr, stride, k, s, top, D,
                                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dist.data_ptr(), n_hits.data_ptr())
    assert ms > 0 and lib.mhx_last_dist_ranges() in (0, 16)   # (see tests/test_gpu_triangle.py: the slices may go to the generic kernel)
    qs = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in qry_recs]
    rs = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in ref_recs]
    want = sc.lists_from(*sc.oracle_matrix(qs, rs, s, k), top, D)
    n = n_hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(n, want[4]) and (n > 0).any() and (n == 0).any() and (n == top).any() and ((n > 0) & (n < top)).any()
    live = np.arange(top)[None, :] < n[:, None]   # entries behind n_hits are unspecified
    for a, b in zip(out, want[:3]):
        assert np.array_equal(a.cpu().numpy().view(np.uint32)[live], b[live])
    x, wx = dist.cpu().numpy()[live], want[3][live]
    assert np.all(np.abs(x - wx) <= 2e-16 * np.maximum(1.0, np.abs(wx)) + 1e-300)   # device log(): <= 1 ulp (as tests/test_gpu_triangle.py)


def all_pairs(qs, rs, s):
    """(common, denom) [nq, nr] of every pair by sorting the two lists together, in numpy: the second copy of a shared hash
    directly follows the first, its place in the union is its position less the copies before it, and it counts when
    that place is below s; denom = min(s, size of the union).  No list may hold 2^64 - 1 or 2^64 - 2 (the paddings)."""
    L = max(max(map(len, qs)), max(map(len, rs)))
    pad_r, pad_q = np.uint64(2 ** 64 - 1), np.uint64(2 ** 64 - 2)
    assert all(len(v) == 0 or v[-1] < pad_q for v in list(qs) + list(rs))
    R = np.full((len(rs), L), pad_r, np.uint64)
    for j, v in enumerate(rs):
        R[j, :len(v)] = v
    rl = np.array([len(v) for v in rs], np.int64)
    common = np.zeros((len(qs), len(rs)), np.uint32)
    denom = np.zeros_like(common)
    at = np.arange(2 * L, dtype=np.int64)[None, :]
    for i, q in enumerate(qs):
        row = np.full(L, pad_q, np.uint64)
        row[:len(q)] = q
        both = np.sort(np.concatenate([R, np.broadcast_to(row, R.shape)], axis=1), axis=1)   # the paddings behind every hash
        second = np.zeros(both.shape, bool)
        second[:, 1:] = both[:, 1:] == both[:, :-1]
        second &= at < (rl + len(q))[:, None]
        place = at - np.cumsum(second, axis=1)
        common[i] = (second & (place < s)).sum(axis=1)
        denom[i] = np.minimum(s, rl + len(q) - second.sum(axis=1))
    return common, denom


def oracle_distances(common, denom, k):
    """the oracle's distance for every (common, denom) of the matrices: compareSketches on two lists that produce them"""
    dist = np.zeros(common.shape, np.float64)
    for c, d in {(int(c), int(d)) for c, d in zip(common.ravel(), denom.ravel())}:
        wc, wd, x = mo.compare(np.arange(d, dtype=np.uint64), np.arange(c, dtype=np.uint64), d, k)
        assert (wc, wd) == (c, d) and d > 0
        dist[(common == c) & (denom == d)] = x
    return dist


def test_more_blocks_than_one_group_of_flag_words(lib, monkeypatch):
    """The flag words of the blocks come back per group of 4096 blocks.  One query per block, 150 queries against 900
    references (29 slices) at s = 64 (16 ranges): 4350 blocks, the last 254 in a second group -- its flag words are cleared
    and used again, and one of its blocks per query falls back: slice 27 holds 32 lists crowded into one value range (2048 keys
    for a table of 1536).  Queries 145 and 147 of the second group derive from references of that slice, so their lists hold
    what the generic kernel computed there.  The expected lists are the rule over all pairs computed in numpy, that matrix
    cross-checked against the oracle's compareSketches on 400 pairs."""
    monkeypatch.setenv("MHX_SEARCH_QBATCH", "1")
    rng = np.random.default_rng(4350)
    s, nq, nr = 64, 150, 900
    bases = [tc.sketch_like(rng, s) for _ in range(30)]
    refs = [tc.mutate(rng, bases[j % 30], 0.02 * (j % 11)) if j % 3 else tc.sketch_like(rng, s) for j in range(nr)]
    lo = 1 << 62
    for j in range(27 * 32, 28 * 32):
        refs[j] = np.uint64(lo) + tc.sketch_like(rng, s, hi=2 ** 20)
    qrys = [tc.mutate(rng, refs[(7 * i) % nr], 0.03 * (i % 9)) for i in range(nq)]
    qrys[145], qrys[147], qrys[3] = refs[870].copy(), refs[880][5:].copy(), refs[866][::2].copy()
    nblocks = nq * ((nr + 31) // 32)
    assert nblocks > 4096 and 145 * 29 + 27 >= 4096   # query 145's block with slice 27 lies in the second group
    assert len(np.unique(np.concatenate(refs[27 * 32:28 * 32]))) > 1536
    common, denom = all_pairs(qrys, refs, s)
    sample = set(zip(rng.integers(0, nq, 380).tolist(), rng.integers(0, nr, 380).tolist())) | {(q, r) for q in (3, 145, 147) for r in (866, 870, 880, 895)}
    for q, r in sample:
        assert (int(common[q, r]), int(denom[q, r])) == mo.compare(refs[r], qrys[q], s, K)[:2], (q, r)
    dist = oracle_distances(common, denom, K)
    for top, max_dist in ((5, 1.0), (3, 0.1)):
        got = run(qrys, refs, s, top, max_dist)
        assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == nq   # slice 27 once per query
        want = sc.lists_from(common, denom, dist, top, max_dist)
        assert want[0][145, 0] == 870 and want[0][147, 0] == 880
        check(got, want)


def test_a_negative_bound(lib):
    """No distance is negative.  The host form returns no hit.  The device form only prefilters, and the prefilter takes a
    negative bound for 0: its lists are the rule's at max_dist = 0 -- the pairs of distance 0 -- however negative the bound."""
    refs, s = sc.references()
    qs, top = sc.queries()[:40], 5
    for max_dist in (-0.001, -1.0):
        got = run(qs, refs, s, top, max_dist)
        assert not got[4].any() and not got[0].any() and not got[1].any()
    want = sc.expected(top, 0.0, 40)
    assert want[4].any()
    stride = 1008
    Q, ql = tc.pad_rows(qs, stride)
    R, rl = tc.pad_rows(refs, stride)
    dev = f"cuda:{torch.cuda.current_device()}"
    d = [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev) for a in (Q, ql, R, rl)]
    for max_dist in (-0.001, -1.0):
        out = [torch.full((40, top), 7, dtype=torch.int32, device=dev) for _ in range(3)]
        n_hits = torch.full((40,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        engine.dist_search_device(d[0].data_ptr(), d[1].data_ptr(), 40, d[2].data_ptr(), d[3].data_ptr(), len(refs), stride, K, s, top, max_dist,
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0, n_hits.data_ptr())
        n = n_hits.cpu().numpy().view(np.uint32)
        assert np.array_equal(n, want[4])
        live = np.arange(top)[None, :] < n[:, None]
        for a, b in zip(out, want[:3]):
            assert np.array_equal(a.cpu().numpy().view(np.uint32)[live], b[live])

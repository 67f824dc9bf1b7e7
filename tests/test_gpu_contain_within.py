"""The unbounded containment call on the GPU (mhx_dist_contain_within) against the rule of tests/contain_within_rule.py over the
rule of the containment, every integer exact: the crowd case at every bound, the crafted edge cases and every case of the
containment (the pair kernel alone, a pair without a geometry, flagged blocks that are taken out late), the device form
against the host form bit for bit and run against run, shapes around a half-wave, a wave, a workgroup and a slice, query
batches and super-batches (where a block's query counts from the super-batch for the cells and from the call for the lists),
more blocks than one group of flag words, the capacity protocol and the counting form, the ties to mhx_dist_contain_search
and mhx_dist_contain, the extreme hash values, empty sets, the argument checks, and device pointers from the segmented sketch."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_contain.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import contain_cases as cc
from tests import contain_rule
from tests import contain_search_rule as search_rule
from tests import contain_within_cases as cwc
from tests import contain_within_rule as rule

pytestmark = pytest.mark.gpu
K = cc.K
THREE = ((0.0, 1), (0.9, 1), (0.95, 3))


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def rows_of(name):
    if name == "crowd":
        return cwc.rows_of()
    return cc.crafted_rows() if name == "crafted" else cc.rows_of(name)


def check(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "row_off", np.flatnonzero(got[0] != want[0])[:5])
    for name, a, b in zip(("ref", "shared", "n_ref", "n_qry"), got[1:], want[1:]):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name, np.flatnonzero(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))


def run(name, bound, cap=None, nq=None, nr=None):
    Q, q_len, R, r_len, s_q, s_r = rows_of(name)
    return engine.dist_contain_within(Q[:nq], q_len[:nq], R[:nr], r_len[:nr], s_q, s_r, K, bound[0], bound[1], cap)


def on_device(*arrays):
    dev = f"cuda:{torch.cuda.current_device()}"
    return [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev) for a in arrays]


def run_device(d, nq, s_q, nr, s_r, stride, bound, cap, k=K):
    """d = on_device(Q, q_len, R, r_len) -> (n, row_off, ref, shared, n_ref, n_qry) as numpy, the hit arrays whole ([cap], filled with 7)"""
    dev = d[0].device
    row_off = torch.full((nq + 1,), 7, dtype=torch.int64, device=dev)
    out = [torch.full((max(cap, 1),), 7, dtype=torch.int32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    n = engine.dist_contain_within_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, stride, k, bound[0], bound[1],
                                          row_off.data_ptr(), *[o.data_ptr() for o in out], cap)
    return (n, row_off.cpu().numpy().view(np.uint64)) + tuple(a.cpu().numpy().view(np.uint32) for a in out)


@pytest.mark.parametrize("bound", cwc.bounds())
def test_crowd_host_form(lib, bound):
    """70 queries x 330 references: eleven slices, the last of 10 references; thirty queries beyond the search's 64 hits.  The
    range route runs (the copies of one genome crowd some of its blocks, which fall back; most do not)"""
    got = run("crowd", bound)
    assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() >= 0 and lib.mhx_last_dist_kernel_ms() > 0
    check(got, cwc.expected(*bound), bound)


@pytest.mark.parametrize("name", ("crafted",) + cc.NAMES)
def test_every_case_of_the_containment(lib, name):
    """crafted: 30 pairs, the pair kernel alone; long_pair: 70 000 entries, no geometry, the pair kernel per block; plasmids and
    crowded: blocks whose flag went up are redone by the pair kernel behind their group and taken out then"""
    for bound in THREE:
        got = run(name, bound)
        if name in ("crafted", "long_pair"):
            assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1
        if name in ("plasmids", "crowded"):
            assert lib.mhx_last_dist_fallback_blocks() > 0
        check(got, rule.csr(*cc.expected(name), K, *bound), (name, bound))


def test_device_form_equals_host_form_and_itself(lib):
    """everything on the device, lengths above the sketch size and above the stride included (the kernels clip what the host form
    refuses); two runs return the same bytes, the untouched tail included"""
    Q, q_len, R, r_len, s_q, s_r = rows_of("crowd")
    lying_q, lying_r = q_len.copy(), r_len.copy()
    lying_q[q_len >= s_q] = 0xFFFFFFF0
    lying_r[r_len >= s_r] = Q.shape[1] + 5
    d = on_device(Q, lying_q, R, lying_r)
    for bound in cwc.bounds():
        host = run("crowd", bound)
        n = int(host[0][-1])
        a = run_device(d, cwc.NQ, s_q, cwc.NR, s_r, Q.shape[1], bound, n + 5)
        b = run_device(d, cwc.NQ, s_q, cwc.NR, s_r, Q.shape[1], bound, n + 5)
        assert a[0] == n == b[0]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
        assert np.array_equal(a[1], host[0])
        for x, h in zip(a[2:], host[1:]):
            assert np.array_equal(x[:n], h) and (x[n:] == 7).all()


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 70])
def test_shapes_around_a_half_wave_a_wave_a_workgroup_and_a_slice(lib, nq):
    for nr in (1, 31, 32, 33, 330):
        for bound in ((0.0, 1), cwc.MAIN[0], cwc.MAIN[1]):
            check(run("crowd", bound, nq=nq, nr=nr), cwc.expected(bound[0], bound[1], nq, nr), (nq, nr, bound))


@pytest.mark.parametrize("env,generic", [({"MHX_SEARCH_QBATCH": "1"}, False), ({"MHX_SEARCH_QBATCH": "13"}, False), ({"MHX_WITHIN_CELLS": "100"}, False),
                                         ({"MHX_WITHIN_CELLS": "45", "MHX_SEARCH_QBATCH": "3"}, False), ({"MHX_DIST_GENERIC": "1"}, True),
                                         ({"MHX_DIST_GENERIC": "1", "MHX_WITHIN_CELLS": "45", "MHX_SEARCH_QBATCH": "3"}, True)])
def test_query_batches_super_batches_and_the_pair_kernel(lib, monkeypatch, env, generic):
    """small batches spread a query's cells over many blocks; MHX_WITHIN_CELLS cuts the 770 cells of the call into super-batches
    of 9 and of 4 queries (18 of them): from the second on a block's lists lie at the query counted from the CALL's first while
    its cells count from the super-batch's, in the finish pass and in the pair kernel alike"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    Q, q_len, R, r_len, s_q, s_r = rows_of("crowd")
    d = on_device(Q, q_len, R, r_len)
    for bound in cwc.bounds():
        want = cwc.expected(*bound)
        got = run("crowd", bound)
        if generic:
            assert (lib.mhx_last_dist_ranges(), lib.mhx_last_dist_fallback_blocks()) == (0, -1)
        else:
            assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() >= 0
        check(got, want, (env, bound))
        n = int(want[0][-1])
        a = run_device(d, cwc.NQ, s_q, cwc.NR, s_r, Q.shape[1], bound, n)
        assert a[0] == n and np.array_equal(a[1], want[0])
        for x, w in zip(a[2:], want[1:]):
            assert np.array_equal(x[:n], w)


def test_more_blocks_than_one_group_of_flag_words(lib, monkeypatch):
    """140 x 960 lists of 64 hashes with one query per block (tests/contain_cases.py: two_groups): 4200 blocks, the last 104 in a
    second group whose flag words are cleared and used again"""
    monkeypatch.setenv("MHX_SEARCH_QBATCH", "1")
    Q, q_len, R, r_len, s_q, s_r = cc.rows_of("two_groups")
    assert len(q_len) * ((len(r_len) + 31) // 32) > 4096
    counts = cc.expected("two_groups")
    for bound in ((0.0, 1), (0.99, 1)):
        want = rule.csr(*counts, K, *bound)
        assert (np.diff(want[0][137:].astype(np.int64)) > 0).all()   # queries of the second group have hits
        got = engine.dist_contain_within(Q, q_len, R, r_len, s_q, s_r, K, bound[0], bound[1])
        assert lib.mhx_last_dist_ranges() == 16
        check(got, want, bound)


def test_capacity_and_the_counting_form(lib):
    Q, q_len, R, r_len, s_q, s_r = rows_of("crowd")
    bound = cwc.MAIN[1]
    want = cwc.expected(*bound)
    n = int(want[0][-1])
    found = ctypes.c_uint64(0)

    def host(cap, store=True):
        row_off = np.full(cwc.NQ + 1, 9, np.uint64)
        out = [np.full(max(cap, 1), 9, np.uint32) for _ in range(4)]
        p = [a.ctypes.data if store else None for a in out]
        rc = lib.mhx_dist_contain_within(Q.ctypes.data, q_len.ctypes.data, cwc.NQ, s_q, R.ctypes.data, r_len.ctypes.data, cwc.NR, s_r, Q.shape[1], K, bound[0],
                                         bound[1], row_off.ctypes.data, p[0], p[1], p[2], p[3], cap, ctypes.byref(found), 0)
        return rc, row_off, out

    rc, row_off, out = host(n - 1)
    assert rc == engine.MHX_E_CAPACITY and found.value == n and np.array_equal(row_off, want[0]) and str(n).encode() in lib.mhx_last_error()
    rc, row_off, out = host(n)
    assert rc == engine.MHX_OK and found.value == n and np.array_equal(row_off, want[0])
    assert all(np.array_equal(a, w) for a, w in zip(out, want[1:]))
    rc, row_off, out = host(5)   # smaller than one cell's run
    assert rc == engine.MHX_E_CAPACITY and found.value == n and np.array_equal(row_off, want[0])
    rc, row_off, out = host(0, store=False)
    assert rc == engine.MHX_OK and found.value == n and np.array_equal(row_off, want[0]) and all((a == 9).all() for a in out)
    assert np.array_equal(engine.dist_contain_within_counts(Q, q_len, R, r_len, s_q, s_r, K, *bound), want[0])
    check(engine.dist_contain_within(Q, q_len, R, r_len, s_q, s_r, K, bound[0], bound[1], cap=10), want)   # the wrapper's one retry
    # the device form: the same protocol, row_off complete beside a list that did not fit
    d = on_device(Q, q_len, R, r_len)
    for cap in (n - 1, 5):
        with pytest.raises(engine.EngineError) as e:
            run_device(d, cwc.NQ, s_q, cwc.NR, s_r, Q.shape[1], bound, cap)
        assert e.value.code == engine.MHX_E_CAPACITY and str(n) in e.value.message
    a = run_device(d, cwc.NQ, s_q, cwc.NR, s_r, Q.shape[1], bound, n)
    assert a[0] == n and np.array_equal(a[1], want[0]) and all(np.array_equal(x, w) for x, w in zip(a[2:], want[1:]))
    row_off = torch.full((cwc.NQ + 1,), 7, dtype=torch.int64, device=d[0].device)
    torch.cuda.synchronize()
    assert engine.dist_contain_within_device(d[0].data_ptr(), d[1].data_ptr(), cwc.NQ, s_q, d[2].data_ptr(), d[3].data_ptr(), cwc.NR, s_r, Q.shape[1], K,
                                             bound[0], bound[1], row_off.data_ptr(), 0, 0, 0, 0, 0) == n
    assert np.array_equal(row_off.cpu().numpy().view(np.uint64), want[0])


@pytest.mark.parametrize("name", ["crowd", "mixed", "small"])
def test_ties_to_the_search_and_to_the_table(lib, name):
    """on the same inputs: every row sorted by contain_better and cut to 64 is mhx_dist_contain_search(top = 64), and the CSR
    is mhx_dist_contain's table filtered through the need table"""
    Q, q_len, R, r_len, s_q, s_r = rows_of(name)
    shared, n_qry, n_ref = engine.dist_contain(Q, q_len, R, r_len, s_q, s_r)
    for bound in THREE:
        got = run(name, bound)
        ref, hs, hr, hq, n_hits = engine.dist_contain_search(Q, q_len, R, r_len, s_q, s_r, K, 64, bound[0], bound[1])
        per_query = rule.rows_of_arrays(got)
        for q, hits in enumerate(per_query):
            top = list(zip(ref[q, :n_hits[q]].tolist(), hs[q, :n_hits[q]].tolist(), hr[q, :n_hits[q]].tolist(), hq[q, :n_hits[q]].tolist()))
            assert search_rule.ranked(hits)[:64] == top, (name, bound, q)
        need = np.array(search_rule.need_table(min(Q.shape[1], s_r), K, bound[0], bound[1]), np.int64)
        keep = shared.astype(np.int64) >= need[n_ref]
        qi, ri = np.nonzero(keep)
        assert np.array_equal(got[0][1:], np.cumsum(keep.sum(axis=1)).astype(np.uint64)) and np.array_equal(got[1], ri.astype(np.uint32))
        assert np.array_equal(got[2], shared[qi, ri]) and np.array_equal(got[3], n_ref[qi, ri]) and np.array_equal(got[4], n_qry[qi, ri])
    if name == "crowd":
        assert max(len(h) for h in per_query) > 64


def test_empty_sets_and_bad_arguments(lib):
    Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows()
    out = [np.full(30, 9, np.uint32) for _ in range(4)]
    row_off = np.full(7, 9, np.uint64)
    found = ctypes.c_uint64(9)

    def call(q=Q, qlen=q_len, nq=6, r=R, rlen=r_len, nr=5, stride=24, k=K, sq=s_q, sr=s_r, min_identity=0.0, min_shared=1, outs=None, off=row_off, cap=30,
             n_out=found):
        o = [a.ctypes.data for a in out] if outs is None else outs
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.mhx_dist_contain_within(p(q), p(qlen), nq, sq, p(r), p(rlen), nr, sr, stride, k, min_identity, min_shared, p(off), o[0], o[1], o[2], o[3],
                                           cap, ctypes.byref(n_out) if n_out is not None else None, 0)

    assert call(nq=0) == engine.MHX_OK and (row_off == 9).all() and found.value == 0 and all((a == 9).all() for a in out)   # nothing but *n_out
    found.value = 9
    assert call(nr=0) == engine.MHX_OK and (row_off == 0).all() and found.value == 0 and all((a == 9).all() for a in out)   # every row is empty
    row_off[:] = 9
    o = [a.ctypes.data for a in out]
    for bad in (dict(min_shared=0), dict(min_identity=float("nan")), dict(k=0), dict(k=33), dict(sq=0), dict(sr=0), dict(stride=0), dict(q=None),
                dict(qlen=None), dict(r=None), dict(rlen=None), dict(off=None), dict(n_out=None), dict(outs=[None] + o[1:]), dict(outs=o[:1] + [None] + o[2:]),
                dict(outs=o[:2] + [None] + o[3:]), dict(outs=o[:3] + [None]), dict(outs=[None] * 4, cap=3)):
        assert call(**bad) == engine.MHX_E_ARG, bad
    assert (row_off == 9).all() and all((a == 9).all() for a in out)
    long = q_len.copy()
    long[3] = 25
    assert call(qlen=long) == engine.MHX_E_ARG and b"q_len[3] exceeds stride" in lib.mhx_last_error()
    long = r_len.copy()
    long[1] = 2000
    assert call(rlen=long) == engine.MHX_E_ARG and b"r_len[1] exceeds stride" in lib.mhx_last_error()
    assert call() == engine.MHX_OK
    want = rule.csr(*cc.expected("crafted"), K)
    n = int(want[0][-1])
    assert found.value == n > 0 and np.array_equal(row_off, want[0]) and all(np.array_equal(a[:n], w) and (a[n:] == 9).all() for a, w in zip(out, want[1:]))
    assert call(min_identity=1.0000001) == engine.MHX_OK and found.value == 0 and (row_off == 0).all()   # above 1: none


def records(rng, n):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [rng.choice(acgt, size=int(m)) for m in rng.integers(300, 3000, size=n)], acgt


def test_device_pointers_from_the_segmented_sketch(lib):
    """two streams of records sketched record by record on the device (sketch_segments_device), the queries at s = 200 and the
    references at s = 60; a query is a reference next to as much of something else, or a near copy of one; nothing returns to the
    host in between.  The oracle sketches every record on its own; the rule over its lists is what the device CSR must hold."""
    rng = np.random.default_rng(2121)
    k, s_q, s_r, stride = 21, 200, 60, 208
    ref_recs, acgt = records(rng, 41)
    qry_recs, _ = records(rng, 38)
    for i in range(0, 38, 3):
        src = ref_recs[(i * 5) % 12].copy()
        at = rng.integers(0, src.size, size=max(1, src.size // (40 * (i + 1))))
        src[at] = rng.choice(acgt, size=at.size)
        qry_recs[i] = np.concatenate([src, rng.choice(acgt, size=src.size)]) if i % 2 == 0 else src
    for j in range(13, 20):     # and several references inside query 0
        ref_recs[j] = qry_recs[0][40 * j: 40 * j + 400 + 30 * j].copy()
    qry_recs[20] = qry_recs[20][:k + 3]
    dev = f"cuda:{torch.cuda.current_device()}"

    def sketch(recs, s):
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

    q_rows, q_len = sketch(qry_recs, s_q)
    r_rows, r_len = sketch(ref_recs, s_r)
    qs = [mo.bruteforce_sketch([r.tobytes()], k, s_q)[0] for r in qry_recs]
    rs = [mo.bruteforce_sketch([r.tobytes()], k, s_r)[0] for r in ref_recs]
    counts = contain_rule.matrix(qs, rs, s_q, s_r)
    for bound in ((0.0, 1), (0.99, 2)):
        want = rule.csr(*counts, k, *bound)
        n = int(want[0][-1])
        per = np.diff(want[0].astype(np.int64))
        assert (per > 5).any() and (per == 0).any()
        a = run_device([q_rows, q_len, r_rows, r_len], len(qry_recs), s_q, len(ref_recs), s_r, stride, bound, n, k=k)
        assert a[0] == n and np.array_equal(a[1], want[0])
        for x, w in zip(a[2:], want[1:]):
            assert np.array_equal(x[:n], w)

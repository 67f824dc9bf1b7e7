"""The bounded neighbourhood call on the GPU (mhx_dist_within) against the rule of tests/within_rule.py over the oracle's
compareSketches of every pair: the shared case set at every bound, the device form against the host form bit for bit and run
against run, shapes around a slice and a wave, query batches, super-batches and both geometries, more blocks than one group
of flag words, the fallback of crowded values, the extreme hash values, the capacity protocol and the counting form, the
argument checks, and the device-pointer form fed by the segmented sketch."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import extreme_cases as ec
from tests import search_cases as sc
from tests import triangle_cases as tc
from tests import within_cases as wc
from tests import within_rule as rule

pytestmark = pytest.mark.gpu
K = wc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def padded(qs, rs):
    stride = (max(max(map(len, qs)), max(map(len, rs)), 1) + 15) // 16 * 16
    return tc.pad_rows(qs, stride) + tc.pad_rows(rs, stride) + (stride,)


def run(qs, rs, s, max_dist, k=K, cap=None):
    Q, ql, R, rl, _ = padded(qs, rs)
    return engine.dist_within(Q, ql, R, rl, k, s, max_dist, cap)


def check(got, want):
    assert np.array_equal(got[0], want[0]), ("row_off", np.flatnonzero(got[0] != want[0])[:5])
    for name, a, b in zip(("ref", "common", "denom"), got[1:4], want[1:4]):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, np.flatnonzero(a != b)[:5])
    assert np.array_equal(got[4].view(np.uint64), want[4].view(np.uint64))   # host libm on the same counts: bit for bit


def on_device(*arrays):
    dev = f"cuda:{torch.cuda.current_device()}"
    return [torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev) for a in arrays]


def run_device(d, nq, nr, stride, s, max_dist, cap, k=K, with_dist=False):
    """d = on_device(Q, ql, R, rl) -> (n, row_off, ref, common, denom[, dist]) as numpy, the hit arrays whole ([cap], filled with 7)"""
    dev = d[0].device
    row_off = torch.full((nq + 1,), 7, dtype=torch.int64, device=dev)
    out = [torch.full((max(cap, 1),), 7, dtype=torch.int32, device=dev) for _ in range(3)]
    dist = torch.full((max(cap, 1),), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    n = engine.dist_within_device(d[0].data_ptr(), d[1].data_ptr(), nq, d[2].data_ptr(), d[3].data_ptr(), nr, stride, k, s, max_dist,
                                  row_off.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), dist.data_ptr() if with_dist else 0, cap)
    res = (n, row_off.cpu().numpy().view(np.uint64)) + tuple(a.cpu().numpy().view(np.uint32) for a in out)
    return res + (dist.cpu().numpy(),) if with_dist else res


@pytest.mark.parametrize("max_dist", wc.bounds())
def test_case_set_host_form(lib, max_dist):
    """70 queries x 330 references: eleven slices, the last of 10 references; two queries beyond the search's 64 hits"""
    refs, qrys = wc.case_set()
    h = wc.hits_per_query(0.02)
    assert h[0] > 64 and h[1] > 64 and not wc.hits_per_query(np.nextafter(1.0, 0.0))[4:].any()   # conditions on the case set
    assert wc.hits_per_query(0.0)[:4].tolist() == [3, 0, 1, 1]
    got = run(qrys, refs, wc.S, max_dist)
    assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == 0 and lib.mhx_last_dist_kernel_ms() > 0
    check(got, wc.expected(max_dist))


def test_the_bound_that_is_a_pairs_distance(lib):
    """a pair whose distance IS the bound is a hit; at the next double towards 0 it is not"""
    x = wc.exact_bound()
    dist = wc.matrix()[2]
    assert (dist[1] == x).any()
    at, below = wc.expected(x), wc.expected(float(np.nextafter(x, 0.0)))
    lost = int(at[0][-1] - below[0][-1])
    assert lost == int((dist == x).sum()) and lost > 0
    refs, qrys = wc.case_set()
    assert int(run(qrys, refs, wc.S, x)[0][-1]) - int(run(qrys, refs, wc.S, float(np.nextafter(x, 0.0)))[0][-1]) == lost


def test_device_form_equals_host_form_and_itself(lib):
    refs, qrys = wc.case_set()
    Q, ql, R, rl, stride = padded(qrys, refs)
    d = on_device(Q, ql, R, rl)
    for max_dist in wc.bounds():
        want = wc.expected(max_dist)
        n = int(want[0][-1])
        cap = n + 5
        a = run_device(d, wc.NQ, wc.NR, stride, wc.S, max_dist, cap, with_dist=True)
        b = run_device(d, wc.NQ, wc.NR, stride, wc.S, max_dist, cap, with_dist=True)
        assert a[0] == n == b[0]
        for x, y in zip(a[1:5], b[1:5]):
            assert x.tobytes() == y.tobytes()          # two runs: identical bytes, the untouched tail included
        assert a[5].tobytes() == b[5].tobytes()
        assert np.array_equal(a[1], want[0])
        for x, w in zip(a[2:5], want[1:4]):
            assert np.array_equal(x[:n], w) and (x[n:] == 7).all()   # the host form's integers, nothing behind them
        dx, wx = a[5][:n], want[4]
        assert np.all(np.abs(dx - wx) <= 2e-16 * np.maximum(1.0, np.abs(wx)) + 1e-300)   # device log(): <= 1 ulp (as tests/test_gpu_triangle.py)


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 70])
def test_shapes_around_a_slice_and_a_wave(lib, nq):
    refs, qrys = wc.case_set()
    for nr in (1, 31, 32, 33, 330):
        for max_dist in (0.0, 0.02, wc.exact_bound(), 1.0):
            got = run(qrys[:nq], refs[:nr], wc.S, max_dist)
            check(got, wc.expected(max_dist, nq, nr))
            if max_dist == 1.0:
                assert int(got[0][-1]) == nq * nr and np.array_equal(got[1], np.tile(np.arange(nr, dtype=np.uint32), nq))


@pytest.mark.parametrize("env,ranges", [({"MHX_WITHIN_QBATCH": "1"}, 16), ({"MHX_WITHIN_QBATCH": "13"}, 16), ({"MHX_WITHIN_GEOMETRY": "dist"}, 1024),
                                        ({"MHX_WITHIN_CELLS": "100"}, 16), ({"MHX_WITHIN_CELLS": "45", "MHX_WITHIN_QBATCH": "3"}, 16)])
def test_query_batches_super_batches_and_geometries(lib, monkeypatch, env, ranges):
    """small batches spread a query's cells over many blocks; MHX_WITHIN_CELLS cuts the 770 cells of the call into super-batches
    of 9 and of 4 queries, each with its own scan and gather on top of the rows before it"""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    refs, qrys = wc.case_set()
    Q, ql, R, rl, stride = padded(qrys, refs)
    d = on_device(Q, ql, R, rl)
    for max_dist in wc.bounds():
        want = wc.expected(max_dist)
        got = run(qrys, refs, wc.S, max_dist)
        assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
        check(got, want)
        n = int(want[0][-1])
        a = run_device(d, wc.NQ, wc.NR, stride, wc.S, max_dist, n)
        assert a[0] == n and np.array_equal(a[1], want[0])
        for x, w in zip(a[2:5], want[1:4]):
            assert np.array_equal(x[:n], w)


def test_longer_lists_take_1024_ranges(lib):
    lists, s = tc.long_set(12, 12_000)
    qs, rs = lists[0::2], lists[1::2]   # the three close pairs of the set lie across the two halves
    common, denom, dist = sc.oracle_matrix(qs, rs, s, K)
    assert [int((dist <= d).sum()) for d in (0.002, 0.004, 1.0)] == [1, 2, 36]
    for max_dist in (0.002, 0.004, 1.0):
        got = run(qs, rs, s, max_dist)
        assert lib.mhx_last_dist_ranges() == 1024 and lib.mhx_last_dist_fallback_blocks() == 0
        check(got, rule.csr_from_matrix(common, denom, dist, max_dist))


def test_more_blocks_than_one_group_of_flag_words(lib, monkeypatch):
    """one query per block, 70 queries against 1920 references (60 slices): 4200 blocks, the last 104 in a second group whose
    flag words are cleared and used again"""
    monkeypatch.setenv("MHX_WITHIN_QBATCH", "1")
    refs, qrys, (common, denom, dist) = wc.big()
    assert len(qrys) * ((len(refs) + 31) // 32) > 4096
    for max_dist in (0.02, 0.05):
        want = rule.csr_from_matrix(common, denom, dist, max_dist)
        assert int(want[0][1]) > 64 and int(want[0][2] - want[0][1]) > 64
        got = run(qrys, refs, wc.S, max_dist)
        assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == 0
        check(got, want)


def test_crowded_values_fall_back_and_stay_exact(lib):
    """the non-uniform construction of the distance tests on both sides: the range pass gives blocks up, the generic kernel
    redoes them later and their take-out fills the same cells"""
    lists, s = tc.crowded(40)
    qs, rs = lists[:20], lists[20:]
    common, denom, dist = sc.oracle_matrix(qs, rs, s, K)
    Q, ql, R, rl, stride = padded(qs, rs)
    d = on_device(Q, ql, R, rl)
    for max_dist in (0.02, 0.05, 1.0):
        want = rule.csr_from_matrix(common, denom, dist, max_dist)
        got = run(qs, rs, s, max_dist)
        assert lib.mhx_last_dist_fallback_blocks() > 0
        check(got, want)
        n = int(want[0][-1])
        a = run_device(d, 20, 20, stride, s, max_dist, n)
        b = run_device(d, 20, 20, stride, s, max_dist, n)
        assert lib.mhx_last_dist_fallback_blocks() > 0 and a[0] == n
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])) and np.array_equal(a[1], want[0])
        for x, w in zip(a[2:5], want[1:4]):
            assert np.array_equal(x[:n], w)
    assert 0 < int(rule.csr_from_matrix(common, denom, dist, 0.05)[0][-1]) < 400


@pytest.mark.parametrize("case", ["plain", "mirrored", "zero"])
def test_extreme_hash_values(lib, case):
    """lists that hold 2^64 - 1 (the vacant-slot marker of the range table) and hash 0 (the padding of the rows)"""
    qrys, refs, s = ec.with_zero() if case == "zero" else ec.batch(40, case == "mirrored")
    assert any(len(v) and v[0] == 0 for v in refs) if case == "zero" else ec.holders(refs)
    common, denom, dist = ec.oracle_matrix(qrys, refs, s)
    for max_dist in (0.0, 0.01, 0.03, 1.0):
        want = rule.csr_from_matrix(common, denom, dist, max_dist)
        check(run(qrys, refs, s, max_dist), want)
    assert 0 < int(rule.csr_from_matrix(common, denom, dist, 0.03)[0][-1]) < common.size


def test_capacity_and_the_counting_form(lib):
    refs, qrys = wc.case_set()
    Q, ql, R, rl, stride = padded(qrys, refs)
    want = wc.expected(0.02)
    n = int(want[0][-1])
    found = ctypes.c_uint64(0)

    def host(cap, store=True):
        row_off = np.full(wc.NQ + 1, 9, np.uint64)
        out = [np.full(max(cap, 1), 9, np.uint32) for _ in range(3)]
        p = [a.ctypes.data if store else None for a in out]
        rc = lib.mhx_dist_within(Q.ctypes.data, ql.ctypes.data, wc.NQ, R.ctypes.data, rl.ctypes.data, wc.NR, stride, K, wc.S, 0.02, row_off.ctypes.data,
                                 p[0], p[1], p[2], None, cap, ctypes.byref(found), 0)
        return rc, row_off, out

    rc, row_off, out = host(n - 1)
    assert rc == engine.MHX_E_CAPACITY and found.value == n and np.array_equal(row_off, want[0]) and str(n).encode() in lib.mhx_last_error()
    rc, row_off, out = host(n)
    assert rc == engine.MHX_OK and found.value == n and np.array_equal(row_off, want[0])
    assert all(np.array_equal(a, w) for a, w in zip(out, want[1:4]))
    rc, row_off, out = host(0, store=False)
    assert rc == engine.MHX_OK and found.value == n and np.array_equal(row_off, want[0]) and all((a == 9).all() for a in out)
    assert np.array_equal(engine.dist_within_counts(Q, ql, R, rl, K, wc.S, 0.02), want[0])
    got = engine.dist_within(Q, ql, R, rl, K, wc.S, 0.02, cap=10)   # the wrapper's one retry
    check(got, want)
    # the device form: the same protocol, row_off complete beside a list that did not fit
    d = on_device(Q, ql, R, rl)
    with pytest.raises(engine.EngineError) as e:
        run_device(d, wc.NQ, wc.NR, stride, wc.S, 0.02, n - 1)
    assert e.value.code == engine.MHX_E_CAPACITY and str(n) in e.value.message
    a = run_device(d, wc.NQ, wc.NR, stride, wc.S, 0.02, n)
    assert a[0] == n and np.array_equal(a[1], want[0]) and all(np.array_equal(x, w) for x, w in zip(a[2:5], want[1:4]))
    dev = d[0].device
    row_off = torch.full((wc.NQ + 1,), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert engine.dist_within_device(d[0].data_ptr(), d[1].data_ptr(), wc.NQ, d[2].data_ptr(), d[3].data_ptr(), wc.NR, stride, K, wc.S, 0.02,
                                     row_off.data_ptr(), 0, 0, 0, 0, 0) == n
    assert np.array_equal(row_off.cpu().numpy().view(np.uint64), want[0])


def test_empty_sets_and_bad_arguments(lib):
    refs, qrys = wc.case_set()
    Q, ql = tc.pad_rows(qrys[:5], 128)
    R, rl = tc.pad_rows(refs[:5], 128)
    out = [np.full(25, 9, np.uint32) for _ in range(3)]
    row_off = np.full(6, 9, np.uint64)
    found = ctypes.c_uint64(9)

    def call(q=Q, qlen=ql, nq=5, r=R, rlen=rl, nr=5, stride=128, k=K, s_=wc.S, max_dist=1.0, outs=None, off=row_off, cap=25, n_out=found):
        o = [a.ctypes.data for a in out] if outs is None else outs
        p = lambda a: a.ctypes.data if a is not None else None
        return lib.mhx_dist_within(p(q), p(qlen), nq, p(r), p(rlen), nr, stride, k, s_, max_dist, p(off), o[0], o[1], o[2], None, cap,
                                   ctypes.byref(n_out) if n_out is not None else None, 0)

    assert call(nq=0) == engine.MHX_OK and (row_off == 9).all() and found.value == 9           # nothing written
    assert call(nq=0, q=None, qlen=None, off=None, n_out=None, outs=[None] * 3) == engine.MHX_OK
    assert call(nr=0) == engine.MHX_OK and (row_off == 0).all() and found.value == 0           # no references: every row is empty
    for bad in (dict(max_dist=float("nan")), dict(k=0), dict(k=33), dict(s_=0), dict(s_=1 << 20), dict(stride=0), dict(q=None), dict(qlen=None),
                dict(r=None), dict(rlen=None), dict(off=None), dict(n_out=None), dict(outs=[None, out[1].ctypes.data, out[2].ctypes.data]),
                dict(outs=[out[0].ctypes.data, None, out[2].ctypes.data]), dict(outs=[out[0].ctypes.data, out[1].ctypes.data, None]),
                dict(outs=[None] * 3, cap=3)):
        assert call(**bad) == engine.MHX_E_ARG, bad
    long = ql.copy()
    long[3] = 129
    assert call(qlen=long) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    long = rl.copy()
    long[4] = 2000
    assert call(rlen=long) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    assert call() == engine.MHX_OK and found.value == 25 and row_off.tolist() == [0, 5, 10, 15, 20, 25]   # 25 pairs: the generic kernel alone
    assert lib.mhx_last_dist_fallback_blocks() == -1 and lib.mhx_last_dist_ranges() == 0
    want = wc.expected(1.0, 5, 5)
    assert all(np.array_equal(a, w) for a, w in zip(out, want[1:4]))
    assert call(max_dist=0.02) == engine.MHX_OK and np.array_equal(row_off, wc.expected(0.02, 5, 5)[0])


def records(rng, n):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [rng.choice(acgt, size=int(m)) for m in rng.integers(300, 3000, size=n)], acgt


def test_device_pointers_from_the_segmented_sketch(lib):
    """two streams of about 40 records, sketched record by record on the device (sketch_segments_device), one the queries, the
    other the references, near copies between them; nothing returns to the host in between.  The oracle sketches every record on
    its own; the rule over its pairs is what the device CSR must hold."""
    rng = np.random.default_rng(4242)
    k, s, stride, D = 21, 200, 208, 0.1
    ref_recs, acgt = records(rng, 41)
    qry_recs, _ = records(rng, 38)
    for i in range(0, 38, 3):   # near copies of references, some of the same one
        src = ref_recs[(i * 5) % 12].copy()
        at = rng.integers(0, src.size, size=max(1, src.size // (15 * (i + 1))))
        src[at] = rng.choice(acgt, size=at.size)
        qry_recs[i] = src
    for j in range(13, 20):     # and several references close to query 0
        src = ref_recs[0].copy()
        at = rng.integers(0, src.size, size=j)
        src[at] = rng.choice(acgt, size=at.size)
        ref_recs[j] = src
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
    qs = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in qry_recs]
    rs = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in ref_recs]
    want = rule.csr_from_matrix(*sc.oracle_matrix(qs, rs, s, k), D)
    n = int(want[0][-1])
    per = np.diff(want[0].astype(np.int64))
    assert (per > 5).any() and (per == 0).any() and (per == 1).any()
    a = run_device([q_rows, q_len, r_rows, r_len], nq, nr, stride, s, D, n, k=k)
    assert a[0] == n and np.array_equal(a[1], want[0])
    for x, w in zip(a[2:5], want[1:4]):
        assert np.array_equal(x[:n], w)

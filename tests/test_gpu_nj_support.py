"""Jackknife support of the neighbour-joining tree on the GPU (mhx_resample_rows, mhx_dist_nj_support) against the rules of
tests/resample_rule.py and tests/nj_support_rule.py: one replicate of a set byte for byte in both pointer forms, the main
records, every replicate's sketch size and joins and the support values in both forms, twice, the argument checks, the memory
budget, a replicate that keeps nothing, and mhx_dist_nj behind the call."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import nj_cases as nc
from tests import nj_rule as nr
from tests import nj_support_rule as ns
from tests import resample_rule as rr
from tests import triangle_cases as tc
from tests.test_gpu_nj import check
from tests.test_resample_emulation import ladder_lists

pytestmark = pytest.mark.gpu
K = nc.K
R, KEEP, SEED = 4, 0.5, 42
CASES = [("set70", ()), ("tiny", (2,)), ("tiny", (3,)), ("tiny", (33,)), ("tiny", (65,)), ("short", ()), ("identical", (70,)), ("disjoint", (70,))]


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def dev():
    return f"cuda:{torch.cuda.current_device()}"


def resample_device(M, lens, s, seed, r, keep):
    """the device-pointer form on copies of M and lens, the outputs filled with something else before"""
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev())
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev())
    o_rows = torch.full(M.shape, -2, dtype=torch.int64, device=dev())
    o_len = torch.full(lens.shape, -1, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    s_r = ctypes.c_uint32(0)
    v = ctypes.c_void_p
    engine._check(engine.load().mhx_resample_rows(v(d_rows.data_ptr()), v(d_len.data_ptr()), M.shape[0], M.shape[1], s, seed, r, keep, v(o_rows.data_ptr()),
                                                  v(o_len.data_ptr()), ctypes.byref(s_r), 1))
    return o_rows.cpu().numpy().view(np.uint64), o_len.cpu().numpy().view(np.uint32), s_r.value


def resample_sets():
    out = [("set70",) + nc.lists_of("set70") + (None,), ("short",) + nc.lists_of("short") + (None,)]
    for stride in (1000, 1008, 1024):   # len == stride; no multiple of 64; a multiple of 64
        out.append(("ladder/%d" % stride, ladder_lists(), 1000, stride))
    return out


@pytest.mark.parametrize("keep", [0.5, 1.0, 0.03])
def test_one_replicate_equals_the_rule_in_both_forms(lib, keep):
    for tag, lists, s, stride in resample_sets():
        M, lens = tc.pad_rows(lists, stride)
        for seed, r in ((SEED, 0), (2 ** 64 - 1, 7)):
            want, want_s = rr.replicate(lists, s, seed, r, keep)
            want_M, want_len = tc.pad_rows(want, M.shape[1])
            for form in ("host", "device"):
                rows, ln, s_r = engine.resample_rows(M, lens, s, seed, r, keep) if form == "host" else resample_device(M, lens, s, seed, r, keep)
                assert s_r == want_s, (tag, form, seed, r)
                assert ln.tobytes() == want_len.tobytes(), (tag, form, seed, r)
                assert rows.tobytes() == want_M.tobytes(), (tag, form, seed, r)
            assert keep < 1.0 or (want_s == s and want_M.tobytes() == M.tobytes())


def support_device(M, lens, s, replicates, keep, seed):
    """the device-pointer form: (the seven main outputs as numpy arrays, support, rep_join_a, rep_join_b, rep_s)"""
    n = M.shape[0]
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev())
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev())
    o32 = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev()) for _ in range(2)]
    o64 = [torch.full((n - 1,), -1, dtype=torch.int64, device=dev()) for _ in range(3)]
    f64 = [torch.full((n - 1,), -7.0, dtype=torch.float64, device=dev()) for _ in range(2)]
    torch.cuda.synchronize()
    rest = engine.dist_nj_support_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, replicates, keep, seed,
                                         *(o.data_ptr() for o in o32 + o64 + f64))
    main = tuple(o.cpu().numpy().view(np.uint32) for o in o32) + tuple(o.cpu().numpy().view(np.uint64) for o in o64) + tuple(o.cpu().numpy() for o in f64)
    assert d_rows.cpu().numpy().view(np.uint64).tobytes() == M.tobytes()   # the caller's rows are read only
    return main, rest


def check_support(got, want):
    sup, rep_a, rep_b, rep_s = got
    want_sup, want_a, want_b, want_s = want
    assert rep_s.tolist() == want_s.tolist()
    assert rep_a.tobytes() == want_a.tobytes() and rep_b.tobytes() == want_b.tobytes()
    assert sup.tolist() == want_sup.tolist()


@pytest.mark.parametrize("name,args", CASES)
def test_main_records_replicates_and_support_equal_the_rule_in_both_forms_twice(lib, name, args):
    lists, s = nc.lists_of(name, args)
    M, lens = tc.pad_rows(lists)
    want_main = nc.expected(name, args)
    want = ns.expected(name, args, R, KEEP, SEED)
    if name == "set70":   # on the rule's values: otherwise the test could not tell counting from a constant
        assert any(0 < c < R for c in want[0].tolist()), want[0].tolist()
    for _ in range(2):
        got = engine.dist_nj_support(M, lens, K, s, R, KEEP, SEED)
        check(got[:7], want_main)
        check_support(got[7:], want)
        assert lib.mhx_last_nj_clamps() == want_main[1] and lib.mhx_last_dist_kernel_ms() > 0
        main, rest = support_device(M, lens, s, R, KEEP, SEED)
        check(main, want_main)
        check_support(rest, want)
        assert lib.mhx_last_nj_clamps() == want_main[1]
    print(name, args, "support", want[0].tolist(), "s_r", want[3].tolist())
    # behind the call mhx_dist_nj gives what it gave: the shared tree holds no stale state
    check(engine.dist_nj(M, lens, K, s), want_main)


def test_keep_one_gives_full_support(lib):
    for name, args in (("set70", ()), ("tiny", (33,)), ("short", ())):
        lists, s = nc.lists_of(name, args)
        M, lens = tc.pad_rows(lists)
        got = engine.dist_nj_support(M, lens, K, s, 3, 1.0, SEED)
        check(got[:7], nc.expected(name, args))
        assert (got[7] == 3).all() and (got[10] == s).all()
        assert (got[8] == got[0]).all() and (got[9] == got[1]).all()   # every replicate is the main tree


def test_no_replicates_is_the_main_tree_alone(lib):
    lists, s = nc.lists_of("tiny", (33,))
    M, lens = tc.pad_rows(lists)
    n = len(lists)
    ja, jb, sup = (np.full(n - 1, 77, np.uint32) for _ in range(3))
    d, ra, rb = (np.zeros(n - 1, np.uint64) for _ in range(3))
    p = lambda x: ctypes.c_void_p(x.ctypes.data)   # noqa: E731
    for support in (p(sup), None):   # a null support is fine without replicates
        assert lib.mhx_dist_nj_support(p(M), p(lens), n, M.shape[1], K, s, 0, 0.5, SEED, p(ja), p(jb), p(d), p(ra), p(rb), None, None, support, None, None, None,
                                       0) == engine.MHX_OK
        assert list(zip(ja.tolist(), jb.tolist(), d.tolist(), ra.tolist(), rb.tolist())) == nc.expected("tiny", (33,))[0]
    assert (sup == 77).all()   # untouched
    # support alone, without the replicates' joins and sizes
    assert lib.mhx_dist_nj_support(p(M), p(lens), n, M.shape[1], K, s, R, KEEP, SEED, p(ja), p(jb), p(d), p(ra), p(rb), None, None, p(sup), None, None, None,
                                   0) == engine.MHX_OK
    assert sup.tolist() == ns.expected("tiny", (33,), R, KEEP, SEED)[0].tolist()


def test_device_pointers_from_the_segmented_sketch(lib):
    """24 records of one stream, sketched record by record on the device (sketch_segments_device): the result goes straight in"""
    rng = np.random.default_rng(4242)
    k, s, stride, n = 21, 200, 208, 24
    acgt = np.frombuffer(b"ACGT", np.uint8)
    recs = [rng.choice(acgt, size=int(x)) for x in rng.integers(300, 3000, size=n)]
    for i in range(3, n, 3):   # some records are near copies of the one before
        src = recs[i - 1].copy()
        at = rng.integers(0, src.size, size=max(1, src.size // (10 * i)))
        src[at] = rng.choice(acgt, size=at.size)
        recs[i] = src
    data = b"".join(r.tobytes() for r in recs)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([r.size for r in recs], dtype=np.uint64)
    d_bytes = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev())
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev())
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev())
    d_rows = torch.zeros((n, stride), dtype=torch.int64, device=dev())
    d_len = torch.zeros(n, dtype=torch.int32, device=dev())
    o32 = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev()) for _ in range(2)]
    o64 = [torch.full((n - 1,), -1, dtype=torch.int64, device=dev()) for _ in range(3)]
    f64 = [torch.full((n - 1,), -7.0, dtype=torch.float64, device=dev()) for _ in range(2)]
    torch.cuda.synchronize()
    engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), n, k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
    got = engine.dist_nj_support_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s, R, KEEP, SEED, *(o.data_ptr() for o in o32 + o64 + f64))
    sketches = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in recs]
    common, denom, _ = tc.oracle_pairs(sketches, s, k)
    records, clamps = nr.records_of(common, denom, n, k)
    main = tuple(o.cpu().numpy().view(np.uint32) for o in o32) + tuple(o.cpu().numpy().view(np.uint64) for o in o64) + tuple(o.cpu().numpy() for o in f64)
    check(main, (records, clamps) + nr.all_lengths(records))
    trees = ns.replicate_trees(sketches, s, k, R, KEEP, SEED)
    assert got[3].tolist() == [t[1] for t in trees]
    assert [list(zip(a, b)) for a, b in zip(got[1].tolist(), got[2].tolist())] == [t[0] for t in trees]
    assert got[0].tolist() == ns.support(ns.joins_of(records), [t[0] for t in trees], n)


def test_bad_arguments_leave_the_sentinels(lib):
    lists, s = nc.lists_of("set70")
    M, lens = tc.pad_rows(lists[:5])
    o32, o64, f64 = np.full(64, 77, np.uint32), np.full(8, 77, np.uint64), np.full(8, 77.0, np.float64)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)   # noqa: E731

    def call(n=5, k=K, s_=s, reps=R, keep=KEEP, rows=M, ln=lens, a=o32, d=o64, la=f64, lb=f64, sup=o32, rep_a=o32, rep_b=o32):
        return lib.mhx_dist_nj_support(p(rows), p(ln), n, M.shape[1], k, s_, reps, keep, SEED, p(a), p(a), p(d), p(d), p(d), p(la), p(lb), p(sup), p(rep_a),
                                       p(rep_b), p(o32), 0)
    for keep in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(keep=keep) == engine.MHX_E_ARG and b"keep" in lib.mhx_last_error()
        assert call(keep=keep, reps=0) == engine.MHX_E_ARG and call(keep=keep, n=1) == engine.MHX_E_ARG
    assert call(reps=10001) == engine.MHX_E_ARG and b"replicates" in lib.mhx_last_error()
    assert call(sup=None) == engine.MHX_E_ARG and b"null argument" in lib.mhx_last_error()
    assert call(rep_a=None) == engine.MHX_E_ARG and call(rep_b=None) == engine.MHX_E_ARG
    # anything mhx_dist_nj refuses
    assert call(s_=1 << 20) == engine.MHX_E_ARG and b"sketch size too large" in lib.mhx_last_error()
    was = int(lens[3])
    lens[3] = M.shape[1] + 1
    assert call() == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    lens[3] = was
    assert call(n=65537, rows=None, ln=None) == engine.MHX_E_ARG
    for k, s_bad in ((0, s), (33, s), (K, 0)):
        assert call(k=k, s_=s_bad) == engine.MHX_E_ARG
    assert call(rows=None) == engine.MHX_E_ARG and call(ln=None) == engine.MHX_E_ARG
    for kw in ({"a": None}, {"d": None}, {"la": None}, {"lb": None}):
        assert call(**kw) == engine.MHX_E_ARG and b"null argument" in lib.mhx_last_error()
    assert (o32 == 77).all() and (o64 == 77).all() and (f64 == 77.0).all()
    assert call(n=1) == engine.MHX_OK and call(n=0) == engine.MHX_OK and (o32 == 77).all()   # n <= 1: nothing written
    got = engine.dist_nj_support(M, lens, K, s, R, KEEP, SEED)   # the same arguments in buffers of their own: accepted
    assert got[7][-1] == R and got[0].tolist() == engine.dist_nj(M, lens, K, s)[0].tolist()
    # n == 2: the one join holds every leaf
    got = engine.dist_nj_support(M[:2], lens[:2], K, s, 3, KEEP, SEED)
    assert got[7].tolist() == [3]
    # the replicate of a set, too
    s_r = ctypes.c_uint32(99)
    out, out_len = np.full_like(M, 77), np.full_like(lens, 77)
    for keep in (0.0, 1.5, float("nan")):
        assert lib.mhx_resample_rows(p(M), p(lens), 5, M.shape[1], s, SEED, 0, keep, p(out), p(out_len), ctypes.byref(s_r), 0) == engine.MHX_E_ARG
    assert lib.mhx_resample_rows(p(M), p(lens), 5, M.shape[1], s, SEED, 0, 0.5, None, p(out_len), ctypes.byref(s_r), 0) == engine.MHX_E_ARG
    assert lib.mhx_resample_rows(p(M), p(lens), 5, M.shape[1], 0, SEED, 0, 0.5, p(out), p(out_len), ctypes.byref(s_r), 0) == engine.MHX_E_ARG
    assert s_r.value == 99 and (out == 77).all() and (out_len == 77).all()


def test_the_budget_refuses_what_does_not_fit(lib, monkeypatch):
    lists, s = nc.lists_of("set70")
    M, lens = tc.pad_rows(lists)
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "0")
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_nj_support(M, lens, K, s, R, KEEP, SEED)
    assert exc.value.code == engine.MHX_E_CAPACITY and "MHX_LINKAGE_STORE_MB" in exc.value.message
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "1")
    assert engine.dist_nj_support(M, lens, K, s, R, KEEP, SEED)[7].tolist() == ns.expected("set70", (), R, KEEP, SEED)[0].tolist()


def test_a_replicate_that_keeps_nothing_is_refused(lib):
    """keep = 2^-31 admits two values of 2^32: no hash of a full list of set70 passes"""
    lists, s = nc.lists_of("set70")
    M, lens = tc.pad_rows(lists)
    with pytest.raises(ValueError):
        rr.replicate(lists, s, SEED, 0, 2.0 ** -31)
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_nj_support(M, lens, K, s, R, 2.0 ** -31, SEED)
    assert exc.value.code == engine.MHX_E_ARG and "replicate 0" in exc.value.message and "keep" in exc.value.message
    with pytest.raises(engine.EngineError) as exc:
        engine.resample_rows(M, lens, s, SEED, 3, 2.0 ** -31)
    assert exc.value.code == engine.MHX_E_ARG and "replicate 3" in exc.value.message
    check(engine.dist_nj(M, lens, K, s), nc.expected("set70"))

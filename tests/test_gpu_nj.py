"""Neighbour joining over one sketch set on the GPU (mhx_dist_nj) against the rule of tests/nj_rule.py -- brute force over the
oracle's pairs in exact integers: records and branch lengths byte for byte in the host form and in the device-pointer form,
twice, the count of clamped updates, the argument checks and the memory budget."""
import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import nj_cases as nc
from tests import nj_rule as nr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = nc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def check(got, want):
    """join_a, join_b, d, r_a, r_b equal the rule's records, len_a and len_b are its doubles bit for bit"""
    ja, jb, d, ra, rb, la, lb = got
    records, _, want_la, want_lb = want
    rows = list(zip(ja.tolist(), jb.tolist(), d.tolist(), ra.tolist(), rb.tolist()))
    assert len(rows) == len(records)
    bad = [t for t in range(len(records)) if rows[t] != records[t]]
    assert not bad, (bad[:5], [rows[t] for t in bad[:5]], [records[t] for t in bad[:5]])
    assert la.tobytes() == want_la.tobytes() and lb.tobytes() == want_lb.tobytes()


def device_call(M, lens, s, with_lengths=True):
    """the device-pointer form on copies of M and lens: the seven outputs as numpy arrays (lengths: the sentinel when not asked)"""
    dev = f"cuda:{torch.cuda.current_device()}"
    n = M.shape[0]
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    o32 = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    o64 = [torch.full((n - 1,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
    f64 = [torch.full((n - 1,), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    m = engine.dist_nj_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, *(o.data_ptr() for o in o32), *(o.data_ptr() for o in o64),
                              *((o.data_ptr() for o in f64) if with_lengths else (0, 0)))
    assert m == n - 1
    return tuple(o.cpu().numpy().view(np.uint32) for o in o32) + tuple(o.cpu().numpy().view(np.uint64) for o in o64) + tuple(o.cpu().numpy() for o in f64)


@pytest.mark.parametrize("name,args", nc.CASES)
def test_records_and_lengths_equal_the_rule_in_both_forms_twice(lib, name, args):
    lists, s = nc.lists_of(name, args)
    M, lens = tc.pad_rows(lists)
    want = nc.expected(name, args)
    for _ in range(2):
        check(engine.dist_nj(M, lens, K, s), want)
        assert lib.mhx_last_nj_clamps() == want[1]
        assert lib.mhx_last_dist_kernel_ms() > 0
        check(device_call(M, lens, s), want)
        assert lib.mhx_last_nj_clamps() == want[1]
    print(name, args, "clamps", want[1])


def test_lengths_may_be_left_out(lib):
    lists, s = nc.lists_of("tiny", (33,))
    M, lens = tc.pad_rows(lists)
    want = nc.expected("tiny", (33,))
    got = device_call(M, lens, s, with_lengths=False)
    assert (got[5] == -7.0).all() and (got[6] == -7.0).all()
    records = list(zip(*(x.tolist() for x in got[:5])))
    assert records == want[0]
    m = len(lists) - 1
    ja, jb = (np.zeros(m, np.uint32) for _ in range(2))
    d, ra, rb = (np.zeros(m, np.uint64) for _ in range(3))
    assert lib.mhx_dist_nj(M.ctypes.data, lens.ctypes.data, m + 1, M.shape[1], K, s, ja.ctypes.data, jb.ctypes.data, d.ctypes.data, ra.ctypes.data,
                           rb.ctypes.data, None, None, 0) == engine.MHX_OK
    assert list(zip(ja.tolist(), jb.tolist(), d.tolist(), ra.tolist(), rb.tolist())) == want[0]


def test_device_pointers_from_the_segmented_sketch(lib):
    """24 records of one stream, sketched record by record on the device (sketch_segments_device) and joined without a host
    round trip; the oracle sketches every record on its own"""
    rng = np.random.default_rng(4141)
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
    dev = f"cuda:{torch.cuda.current_device()}"
    d_bytes = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_rows = torch.zeros((n, stride), dtype=torch.int64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    o32 = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    o64 = [torch.full((n - 1,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
    f64 = [torch.full((n - 1,), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), n, k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
    engine.dist_nj_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s, *(o.data_ptr() for o in o32 + o64 + f64))
    sketches = [mo.bruteforce_sketch([r.tobytes()], k, s)[0] for r in recs]
    common, denom, _ = tc.oracle_pairs(sketches, s, k)
    records, clamps = nr.records_of(common, denom, n, k)
    got = tuple(o.cpu().numpy().view(np.uint32) for o in o32) + tuple(o.cpu().numpy().view(np.uint64) for o in o64) + tuple(o.cpu().numpy() for o in f64)
    check(got, (records, clamps) + nr.all_lengths(records))
    assert lib.mhx_last_nj_clamps() == clamps
    assert any(0 < x < nr.ONE for x in got[2].tolist())


def test_tiny_sets_and_bad_arguments(lib):
    lists, s = nc.lists_of("set70")
    M, lens = tc.pad_rows(lists[:5])
    for n in (0, 1):
        got = engine.dist_nj(M[:n], lens[:n], K, s)
        assert all(a.size == 0 for a in got)
        assert lib.mhx_last_nj_clamps() == 0
    # refused before anything is launched: the sentinels stay
    o32, o64, f64 = np.full(8, 77, np.uint32), np.full(8, 77, np.uint64), np.full(8, 77.0, np.float64)

    def call(n, k=K, s_=s, rows=M, ln=lens, a=o32, b=o32, d=o64, ra=o64, rb=o64, la=f64, lb=f64):
        p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
        return lib.mhx_dist_nj(p(rows), p(ln), n, M.shape[1], k, s_, p(a), p(b), p(d), p(ra), p(rb), p(la), p(lb), 0)
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
    for kw in ({"a": None}, {"b": None}, {"d": None}, {"ra": None}, {"rb": None}, {"la": None}, {"lb": None}):
        assert call(5, **kw) == engine.MHX_E_ARG and b"null argument" in lib.mhx_last_error()
    assert (o32 == 77).all() and (o64 == 77).all() and (f64 == 77.0).all()
    assert call(1) == engine.MHX_OK and (o32 == 77).all()   # n <= 1: nothing written
    assert call(5) == engine.MHX_OK


def test_the_budget_refuses_what_does_not_fit(lib, monkeypatch):
    """set70 holds 2415 pairs, 19 320 bytes of words: refused under a budget of 0 MB with a message that names the variable,
    accepted under 1 MB"""
    lists, s = nc.lists_of("set70")
    M, lens = tc.pad_rows(lists)
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "0")
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_nj(M, lens, K, s)
    assert exc.value.code == engine.MHX_E_CAPACITY and "MHX_LINKAGE_STORE_MB" in exc.value.message
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "1")
    check(engine.dist_nj(M, lens, K, s), nc.expected("set70"))

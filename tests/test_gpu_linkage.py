"""Complete and average linkage of one sketch set on the GPU (mhx_dist_linkage) against the rule of tests/linkage_rule.py --
brute force over the oracle's pairs in exact integers: merges, sizes, values and heights in the host form, the device-pointer
form (the same integers twice), the cut, the argument checks and the memory budget."""
import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from tests import linkage_cases as lc
from tests import linkage_rule as lr
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = lc.K


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def check(got, name, args, linkage):
    """merge_a, merge_b, size, num, den equal the rule's, dist is bit-equal"""
    ma, mb, size, num, den, dist = got
    want, want_dist = lc.expected(name, args, linkage)
    rows = list(zip(ma.tolist(), mb.tolist(), size.tolist(), num.tolist(), den.tolist()))
    assert len(rows) == len(want)
    bad = [t for t in range(len(want)) if rows[t] != want[t]]
    assert not bad, (bad[:5], [rows[t] for t in bad[:5]], [want[t] for t in bad[:5]])
    assert np.array_equal(dist, want_dist)


@pytest.mark.parametrize("linkage", lc.LINKAGES)
@pytest.mark.parametrize("name,args", lc.CASES)
def test_merges_values_and_heights_equal_the_rule(lib, name, args, linkage):
    lists, s = lc.lists_of(name, args)
    n = len(lists)
    M, lens = tc.pad_rows(lists)
    check(engine.dist_linkage(M, lens, K, s, linkage), name, args, linkage)
    rescans = lib.mhx_last_linkage_rescans()
    print(name, args, "rescans", rescans, "per step", rescans / (n - 1))
    assert rescans >= n - 1 > 0   # the merged row at least, every step
    if name in ("identical", "disjoint"):
        assert rescans == n - 1   # every value ties: the id order decides, list 0's cluster stays every row's first partner
    assert lib.mhx_last_dist_kernel_ms() > 0


@pytest.mark.parametrize("linkage", lc.LINKAGES)
def test_names_of_the_linkages(lib, linkage):
    lists, s = lc.lists_of("tiny", (33,))
    M, lens = tc.pad_rows(lists)
    by_name = engine.dist_linkage(M, lens, K, s, {lr.COMPLETE: "complete", lr.AVERAGE: "average"}[linkage])
    check(by_name, "tiny", (33,), linkage)
    with pytest.raises(ValueError):
        engine.dist_linkage(M, lens, K, s, "single")


@pytest.mark.parametrize("linkage", lc.LINKAGES)
@pytest.mark.parametrize("name,args", [("set200", ()), ("short", ()), ("tiny", (65,))])
def test_device_pointers_give_the_same_integers_twice(lib, name, args, linkage):
    dev = f"cuda:{torch.cuda.current_device()}"
    lists, s = lc.lists_of(name, args)
    M, lens = tc.pad_rows(lists)
    n = len(lists)
    host = engine.dist_linkage(M, lens, K, s, linkage)
    check(host, name, args, linkage)
    d_rows = torch.from_numpy(M.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    for with_dist in (True, False, True):
        o32 = [torch.full((n - 1,), -1, dtype=torch.int32, device=dev) for _ in range(3)]
        o64 = [torch.full((n - 1,), -1, dtype=torch.int64, device=dev) for _ in range(2)]
        dist = torch.full((n - 1,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        m = engine.dist_linkage_device(d_rows.data_ptr(), d_len.data_ptr(), n, M.shape[1], K, s, linkage, *(o.data_ptr() for o in o32),
                                       *(o.data_ptr() for o in o64), dist.data_ptr() if with_dist else 0)
        assert m == n - 1 and lib.mhx_last_dist_kernel_ms() > 0 and lib.mhx_last_linkage_rescans() >= n - 1
        for got, want in zip(o32, host[:3]):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
        for got, want in zip(o64, host[3:5]):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
        if with_dist:   # the device's arithmetic: within a few ulp of the host's double
            assert np.allclose(dist.cpu().numpy(), host[5], rtol=1e-12, atol=1e-15)
        else:
            assert (dist.cpu().numpy() == -1.0).all()


@pytest.mark.parametrize("linkage", lc.LINKAGES)
def test_cut_equals_the_rules(lib, linkage):
    for name, bounds in (("set200", [-0.1, 0.0, 0.005, 0.02, 0.05, 0.3, 1.0]), ("short", [0.0, 0.01, 0.1, 0.5, 1.0])):
        lists, s = lc.lists_of(name)
        n = len(lists)
        M, lens = tc.pad_rows(lists)
        ma, mb, _, _, _, dist = engine.dist_linkage(M, lens, K, s, linkage)
        merges, want_dist = lc.expected(name, (), linkage)
        for bound in bounds:
            want, want_clusters, _ = lr.labels(merges, want_dist, n, bound)
            label, clusters = engine.linkage_labels(ma, mb, dist, n, bound)
            assert clusters == want_clusters and np.array_equal(label, want), (name, bound)


def test_tiny_sets_and_bad_arguments(lib):
    lists, s = lc.lists_of("set70")
    M, lens = tc.pad_rows(lists[:5])
    for n in (0, 1):
        got = engine.dist_linkage(M[:n], lens[:n], K, s, lr.AVERAGE)
        assert all(a.size == 0 for a in got)
        assert lib.mhx_last_linkage_rescans() == 0
    # refused before anything is launched: the sentinels stay
    o32, o64 = np.full(8, 77, np.uint32), np.full(8, 77, np.uint64)

    def call(n, k=K, s_=s, rows=M, ln=lens, linkage=lr.COMPLETE, a=o32, sz=o32, nm=o64, dn=o64):
        p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
        return lib.mhx_dist_linkage(p(rows), p(ln), n, M.shape[1], k, s_, linkage, p(a), p(o32), p(sz), p(nm), p(dn), None, 0)
    for bad in (0, 3, -1):
        assert call(5, linkage=bad) == engine.MHX_E_ARG and b"linkage must be" in lib.mhx_last_error()
        assert call(1, linkage=bad) == engine.MHX_E_ARG
    assert call(5, s_=1 << 20) == engine.MHX_E_ARG and b"sketch size too large" in lib.mhx_last_error()
    was = int(lens[3])
    lens[3] = M.shape[1] + 1
    assert call(5) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    lens[3] = was
    assert call(65537, rows=None, ln=None) == engine.MHX_E_ARG
    for k, s_bad in ((0, s), (33, s), (K, 0)):
        assert call(5, k=k, s_=s_bad) == engine.MHX_E_ARG
    assert call(5, rows=None) == engine.MHX_E_ARG and call(5, ln=None) == engine.MHX_E_ARG
    for kw in ({"a": None}, {"sz": None}, {"nm": None}, {"dn": None}):
        assert call(5, **kw) == engine.MHX_E_ARG
    assert (o32 == 77).all() and (o64 == 77).all()
    assert call(1) == engine.MHX_OK and (o32 == 77).all()   # n <= 1: nothing written
    assert call(5) == engine.MHX_OK


def test_the_budget_refuses_what_does_not_fit(lib, monkeypatch):
    """set70 holds 2415 pairs, 19 320 bytes of words: refused under a budget of 0 MB with a message that names the variable,
    accepted under 1 MB"""
    lists, s = lc.lists_of("set70")
    M, lens = tc.pad_rows(lists)
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "0")
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_linkage(M, lens, K, s, lr.COMPLETE)
    assert exc.value.code == engine.MHX_E_CAPACITY and "MHX_LINKAGE_STORE_MB" in exc.value.message
    monkeypatch.setenv("MHX_LINKAGE_STORE_MB", "1")
    check(engine.dist_linkage(M, lens, K, s, lr.COMPLETE), "set70", (), lr.COMPLETE)

"""The rule of complete and average linkage (tests/linkage_rule.py) on the CPU: the exports, the fixed-point distance of the
library against the Python restatement and against the oracle's distance, the heights along the merges, the guarantee of
complete linkage at every cut, and the library's own cut (engine.linkage_labels) against the rule's."""
import numpy as np
import pytest

from auriclass_amd import engine
from tests import cluster_rule as cr
from tests import linkage_cases as lc
from tests import linkage_rule as lr

NEW = ["mhx_dist_linkage", "mhx_last_linkage_rescans", "mhx_linkage_labels", "mhx_linkage_fixed_distance", "mhx_linkage_files"]


@pytest.fixture(scope="module")
def lib():
    return engine.load()


def test_linkage_symbols_are_declared_and_exported(lib):
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    for fn in ("dist_linkage", "dist_linkage_device", "linkage_labels", "linkage_fixed_distance", "linkage_files"):
        assert callable(getattr(engine, fn))
    assert engine.ctypes.sizeof(engine.LinkageOpts) == 32


def _sweep():
    """(denom, [common ...] ascending) of the sweep: every common <= denom for denom <= 119 and for denom = 1000, 3000 random
    ones each for denom = 50 000 and 2^20 - 1"""
    rng = np.random.default_rng(76)
    for d in list(range(120)) + [1000]:
        yield d, list(range(d + 1))
    for d in (50_000, (1 << 20) - 1):
        yield d, sorted(set(rng.integers(0, d + 1, 3000).tolist()) | {0, 1, d - 1, d})


@pytest.mark.parametrize("k", [1, 16, 21, 27, 32])
def test_fixed_distance_equals_the_restatement_and_follows_the_distance(lib, k):
    """the library's integers are the rule's; within 4 units of 2^-32 of the oracle's double; never greater for a greater common"""
    worst = 0.0
    for d, commons in _sweep():
        q = [engine.linkage_fixed_distance(c, d, k) for c in commons]
        assert q == [lr.fixed_distance(c, d, k) for c in commons], (d, k)
        want = np.array([cr.distance(c, d, k) for c in commons]) * 2.0 ** 32
        off = np.abs(np.array(q, np.float64) - want)
        worst = max(worst, float(off.max()))
        assert off.max() <= 4.0, (d, k, commons[int(off.argmax())])
        assert all(q[x + 1] <= q[x] for x in range(len(q) - 1)), (d, k)
    print("k", k, "largest difference", worst, "units of 2^-32")
    assert engine.linkage_fixed_distance(0, 0, k) == 0 and engine.linkage_fixed_distance(0, 7, k) == 1 << 32
    assert engine.linkage_fixed_distance(7, 7, k) == 0
    assert engine.linkage_fixed_distance(8, 7, k) == 2 ** 64 - 1   # outside the domain


def test_value_order_and_combine_on_hand_written_cases():
    C, A = lr.COMPLETE, lr.AVERAGE
    assert lr.closer(C, (1, 2), (2, 4)) == 0 and lr.closer(C, (0, 0), (5, 5)) == 0 and lr.closer(C, (3, 4), (1, 2)) == -1
    assert lr.closer(C, (0, 3), (1, 1000)) == 1
    assert lr.combine(C, (1, 2), (2, 4)) == (2, 4) and lr.combine(C, (2, 4), (1, 2)) == (2, 4)   # equal indices: the greater denom
    assert lr.combine(C, (0, 0), (5, 5)) == (5, 5) and lr.combine(C, (3, 4), (1, 2)) == (1, 2)    # otherwise the worse
    assert lr.closer(A, (3, 2), (6, 4)) == 0 and lr.closer(A, (1 << 62, 1 << 30), ((1 << 62) - 1, 1 << 30)) == 1
    assert lr.combine(A, (3, 2), (6, 4)) == (9, 6)
    # three lists by hand: 0 and 2 are closest, the chain 1 - 0 - 2 shows the difference between the linkages
    common, denom = np.array([4, 9, 1], np.uint32), np.array([10, 10, 10], np.uint32)   # pairs (1, 0), (2, 0), (2, 1)
    assert lr.agglomerate(common, denom, 3, 21, C) == [(2, 0, 2, 9, 10), (1, 0, 3, 1, 10)]
    q = [lr.fixed_distance(c, 10, 21) for c in (4, 9, 1)]
    assert lr.agglomerate(common, denom, 3, 21, A) == [(2, 0, 2, q[1], 1), (1, 0, 3, q[0] + q[2], 2)]


@pytest.mark.parametrize("linkage", lc.LINKAGES)
@pytest.mark.parametrize("name,args", lc.CASES)
def test_heights_do_not_decrease(name, args, linkage):
    """both linkages are reducible: no merge lies below the one before it (average: up to one ulp of its rounded doubles)"""
    merges, dist = lc.expected(name, args, linkage)
    n = len(lc.lists_of(name, args)[0])
    assert len(merges) == n - 1 and all(a > b for a, b, *_ in merges)
    assert merges[-1][2] == n if merges else True
    floor = dist[:-1] if linkage == lr.COMPLETE else np.nextafter(dist[:-1], -np.inf)
    assert (dist[1:] >= floor).all()
    assert ((dist >= 0.0) & (dist <= 1.0)).all()


def _members(label):
    groups = {}
    for i, l in enumerate(label.tolist()):
        groups.setdefault(l, []).append(i)
    return groups


def test_complete_linkage_keeps_every_cluster_within_the_bound():
    """set70, at every distinct height and at the double just below it: every two members of a cluster have an oracle distance
    <= the bound"""
    lists, _ = lc.lists_of("set70")
    n = len(lists)
    merges, dist = lc.expected("set70", (), lr.COMPLETE)
    pair_dist = lc.pairs("set70")[2]
    at = lambda i, j: i * (i - 1) // 2 + j   # noqa: E731
    for T in np.unique(dist).tolist():
        for bound in (T, float(np.nextafter(T, -np.inf))):
            label, clusters, applied = lr.labels(merges, dist, n, bound)
            assert clusters == n - applied
            for members in _members(label).values():
                for x, i in enumerate(members):
                    assert all(pair_dist[at(i, j)] <= bound for j in members[:x]), (bound, members)


@pytest.mark.parametrize("linkage", lc.LINKAGES)
def test_library_cut_equals_the_rules(lib, linkage):
    for name, args in (("set70", ()), ("short", ()), ("tiny", (3,)), ("identical", (70,))):
        n = len(lc.lists_of(name, args)[0])
        merges, dist = lc.expected(name, args, linkage)
        ma, mb = (np.array([m[x] for m in merges], np.uint32) for x in (0, 1))
        bounds = [-0.5, 1.0, 2.0] + [b for T in np.unique(dist).tolist() for b in (T, float(np.nextafter(T, -np.inf)))]
        for bound in bounds:
            want, want_clusters, applied = lr.labels(merges, dist, n, bound)
            label, clusters = engine.linkage_labels(ma, mb, dist, n, bound)
            assert clusters == want_clusters == n - applied and np.array_equal(label, want), (name, bound)
            assert (label <= np.arange(n)).all() and (label[label] == label).all()   # a label is a cluster's lowest member
        assert engine.linkage_labels(ma, mb, dist, n, -0.5)[1] == n and engine.linkage_labels(ma, mb, dist, n, 1.0)[1] == 1


def test_library_cut_refuses_bad_arguments(lib):
    ma, mb, dist = np.array([1, 2], np.uint32), np.array([0, 0], np.uint32), np.array([0.1, 0.2])
    label, clusters = engine.linkage_labels(ma, mb, dist, 3, 0.15)
    assert label.tolist() == [0, 0, 2] and clusters == 2
    assert engine.linkage_labels(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0), 0, 0.5)[1] == 0
    assert engine.linkage_labels(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0), 1, 0.5)[1] == 1
    p = lambda a: a.ctypes.data   # noqa: E731
    label = np.full(3, 9, np.uint32)
    assert lib.mhx_linkage_labels(p(ma), p(mb), p(dist), 3, float("nan"), p(label)) == engine.MHX_E_ARG
    assert lib.mhx_linkage_labels(None, p(mb), p(dist), 3, 0.5, p(label)) == engine.MHX_E_ARG
    assert lib.mhx_linkage_labels(p(ma), p(mb), p(dist), 3, 0.5, None) == engine.MHX_E_ARG
    for bad_a, bad_b in (([1, 3], [0, 0]), ([1, 1], [0, 1]), ([0, 2], [1, 0])):
        a, b = np.array(bad_a, np.uint32), np.array(bad_b, np.uint32)
        assert lib.mhx_linkage_labels(p(a), p(b), p(dist), 3, 0.5, p(label)) == engine.MHX_E_ARG
        with pytest.raises(engine.EngineError):
            engine.linkage_labels(a, b, dist, 3, 0.5)
    assert (label == 9).all()

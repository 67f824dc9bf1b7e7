"""The rule of the sharded merge (tests/merge_rule.py) against the library's host merge, mhx_merge_shard_partials, on every
crafted case of tests/merge_cases.py, and against results written out by hand."""
import numpy as np
import pytest

from auriclass_amd import engine
from tests import merge_cases as mc
from tests import merge_rule as mr

MAX64, MAX32 = mr.MAX64, mr.MAX32


def host_merge(ranks, k, s, m):
    """the gathered data as merge_slabs_impl hands it to the host merge: the first n_r entries of every slab without the
    vacant-slot key, and header word 3 as one entry 2^64-1 of a rank whose threshold never fell.  (That the engine itself
    leaves the key out is not seen here but on the device: test_gpu_merge_crafted.py, the vacant-key cases.)"""
    hs, cs, ts = [], [], []
    for hdr, h, c in ranks:
        n = int(hdr[0])
        h, c = np.asarray(h, np.uint64)[:n], np.asarray(c, np.uint32)[:n]
        keep = h != np.uint64(MAX64)
        h, c = h[keep], c[keep]
        if int(hdr[3]) and int(hdr[1]) == MAX64:
            h, c = np.append(h, np.uint64(MAX64)), np.append(c, np.uint32(min(int(hdr[3]), MAX32)))
        hs.append(h); cs.append(c); ts.append(int(hdr[1]))
    try:
        return engine.merge_shard_partials(hs, cs, ts, k, s, m)
    except engine.EngineError as e:
        assert e.code == engine.MHX_E_CAPACITY
        return mr.CAPACITY


def same(a, b):
    if isinstance(a, str) or isinstance(b, str):
        return isinstance(a, str) and isinstance(b, str) and a == b
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("case", mc.all_cases(), ids=repr)
def test_rule_equals_the_host_merge(case):
    ranks = mc.ranks(case)
    assert same(mr.merge(ranks, case.k, case.s, case.m), host_merge(ranks, case.k, case.s, case.m))


def R(T, entries, n=None, maxkey=0):
    h = np.array([e[0] for e in entries], np.uint64)
    c = np.array([e[1] for e in entries], np.uint32)
    return mc.header(len(entries) if n is None else n, T, maxkey), h, c


HAND = [
    # sums straddle m; 30 lies above T_min = 20; s cuts the list
    ("sums", [R(20, [(5, 1), (9, 2), (20, 1)]), R(40, [(9, 1), (20, 1), (30, 9), (3, 1)])], 21, 2, 2, ([9, 20], [3, 2])),
    ("first s", [R(20, [(5, 1), (9, 2), (20, 1)]), R(40, [(9, 1), (3, 1)])], 21, 2, 1, ([3, 5], [1, 1])),
    # three qualify, s = 4, T_min below hash_max: not exact
    ("short", [R(20, [(5, 1), (9, 2), (20, 1)]), R(40, [(9, 1)])], 21, 4, 1, mr.CAPACITY),
    # ... but at k = 16 with every T at 2^32-1 the short list is the sketch
    ("short at hash_max", [R(MAX32, [(5, 1), (9, 2)]), R(MAX32, [(9, 1)])], 16, 4, 1, ([5, 9], [1, 3])),
    # entries behind n are not there; 2^64-1 inside a slab is a vacant slot
    ("n and vacant", [R(MAX64, [(7, 1), (MAX64, 5), (8, 1)], n=2), R(MAX64, [(7, 1)])], 21, 4, 1, ([7], [2])),
    # 2^64-1 comes from header word 3 alone, and only when nobody's threshold fell
    ("maxkey", [R(MAX64, [(7, 1)], maxkey=1), R(MAX64, [(7, 1)], maxkey=2)], 21, 4, 3, ([MAX64], [3])),
    ("maxkey below m", [R(MAX64, [(7, 3)], maxkey=1), R(MAX64, [], maxkey=1)], 21, 4, 3, ([7], [3])),
    ("maxkey, lowered T", [R(MAX64 - 1, [(7, 1)], maxkey=4), R(MAX64, [(7, 1)], maxkey=4)], 21, 1, 1, ([7], [2])),
    # a sum past 2^32-1 is 2^32-1
    ("clamp", [R(99, [(7, MAX32)]), R(99, [(7, 1)]), R(99, [(7, MAX32), (8, 1)])], 21, 2, 2, mr.CAPACITY),
    ("clamp kept", [R(99, [(7, MAX32)]), R(99, [(7, 1)]), R(99, [(7, MAX32), (8, 2)])], 21, 2, 2, ([7, 8], [MAX32, 2])),
]


@pytest.mark.parametrize("name,ranks,k,s,m,want", HAND, ids=[h[0] for h in HAND])
def test_hand_written(name, ranks, k, s, m, want):
    if want != mr.CAPACITY:
        want = (np.array(want[0], np.uint64), np.array(want[1], np.uint32))
    assert same(mr.merge(ranks, k, s, m), want)
    assert same(host_merge(ranks, k, s, m), want)


def test_the_cases_are_what_they_say():
    """a sum of exactly m is kept and one of m - 1 is not; the wrapping sums are kept at 2^32-1; the short cases are short"""
    for m in (1, 2, 3):
        case = mc.by_name(f"counts-exact-m{m}")
        sums = mr.sums(mc.ranks(case))
        assert sorted(set(sums.values())) == [m - 1, m] and list(sums.values()).count(m) == 300
    for n in (2, 63, 64):
        for m in (1, 2):
            case = mc.by_name(f"counts-wrap-{n}x-m{m}")
            got = mr.merge(mc.ranks(case), case.k, case.s, case.m)
            at = list(got[0]).index(mc.WRAP_VALUE)
            assert got[1][at] == MAX32
    for name in ("short-binned", "short-table", "short-host", "t_min-0-m1", "t_min-1-m2"):
        case = mc.by_name(name)
        assert mr.merge(mc.ranks(case), case.k, case.s, case.m) == mr.CAPACITY
    for name in ("t_min-ffffffff-m1", "t_min-ffffffffffffffff-m2-maxkey2"):
        case = mc.by_name(name)
        assert len(mr.merge(mc.ranks(case), case.k, case.s, case.m)[0]) < case.s
    # the vacant-key cases: a 2^64-1 taken from a slab would be the last entry of a short sketch
    for name in ("vacant-key-host", "vacant-key-table"):
        case = mc.by_name(name)
        rk = mc.ranks(case)
        got = mr.merge(rk, case.k, case.s, case.m)
        assert len(got[0]) < case.s and MAX64 not in got[0].tolist() and mr.t_min_of(rk) == MAX64
        assert all(MAX64 in h[:int(hdr[0])].tolist() for hdr, h, _ in case.foreign)
    # header word 3 summing to m - 1 and to m: 2^64-1 is the last entry of the second sketch alone
    for m in (1, 2, 3):
        low = mr.merge(mc.ranks(mc.by_name(f"t_min-ffffffffffffffff-m{m}-maxkey{m - 1}")), 21, 200, m)
        high = mr.merge(mc.ranks(mc.by_name(f"t_min-ffffffffffffffff-m{m}-maxkey{m}")), 21, 200, m)
        assert MAX64 not in low[0].tolist() and high[0][-1] == MAX64 and high[1][-1] == m

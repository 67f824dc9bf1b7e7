"""The rule of the jackknife over sketch hashes (tests/resample_rule.py): the keep function against vectors worked out apart
from it, keep = 1, the cut of a set with short, full and empty lists, and the refusal of a replicate that keeps nothing."""
import numpy as np
import pytest

from tests import linkage_cases as lc
from tests import resample_rule as rr


def test_keep_function_against_hand_computed_vectors():
    # h = 0, seed = 0, r = 0: z starts at the golden-ratio constant -- the first output of SplitMix64 seeded with 0, a published value
    assert rr.mix(0, 0, 0) == 0xE220A8397B1DCDAF
    # h = 2^64 - 1, seed = 42, r = 3: the sum wraps to 41 + 4 * 0x9E3779B97F4A7C15 mod 2^64 = 0x78DDE6E5FD29F07D
    assert (2 ** 64 - 1 + 42 + 4 * 0x9E3779B97F4A7C15) % 2 ** 64 == 0x78DDE6E5FD29F07D
    assert rr.mix(2 ** 64 - 1, 42, 3) == 0x9EBEB27D522A4E8B
    # h + seed wraps on its own: 0xFF..F00 + 0xFF..FF0 = 0xFF..EF0 mod 2^64, plus the constant wraps again
    assert (0xFFFFFFFFFFFFFF00 + 0xFFFFFFFFFFFFFFF0 + 0x9E3779B97F4A7C15) % 2 ** 64 == 0x9E3779B97F4A7B05
    assert rr.mix(0xFFFFFFFFFFFFFF00, 0xFFFFFFFFFFFFFFF0, 0) == 0x3E7906841EEBEC05
    assert rr.mix(0x0123456789ABCDEF, 42, 7) == 0xF9824CC5A45E46FC
    # the decision: the upper 32 bits against T
    assert rr.keeps(0, 0, 0, 0xE220A83A) and not rr.keeps(0, 0, 0, 0xE220A839)
    assert rr.keeps(2 ** 64 - 1, 42, 3, 1 << 32) and not rr.keeps(2 ** 64 - 1, 42, 3, 0x9EBEB27D)
    assert rr.keeps(0xFFFFFFFFFFFFFF00, 0xFFFFFFFFFFFFFFF0, 0, rr.threshold(0.25)) and not rr.keeps(0x0123456789ABCDEF, 42, 7, rr.threshold(0.97))


def test_threshold_of_a_keep_rate():
    assert rr.threshold(1.0) == 1 << 32 and rr.threshold(0.5) == 1 << 31 and rr.threshold(0.03) == 128849018
    assert rr.threshold(2.0 ** -32) == 1 and rr.threshold(2.0 ** -33) == 0
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rr.threshold(bad)


def test_keep_one_keeps_everything():
    lists, s = lc.short()
    for r in (0, 5):
        cut, s_r = rr.replicate(lists, s, 42, r, 1.0)
        assert s_r == s
        assert all(np.array_equal(a, b) for a, b in zip(cut, lists))


def test_the_cut_of_short_full_and_empty_lists():
    """`short`: two empty lists, lists of 1, 5, 300 .. 913 hashes and one full list of 1000.  The full list alone sets s_r; the
    others keep what the function admits, in order, up to s_r; a shared hash is kept in both lists or in neither"""
    lists, s = lc.short()
    assert [len(v) for v in lists] == [0, 0, 1, 5, 300, 450, 620, 777, 913, 1000]
    seed, r, keep = 42, 1, 0.5
    T = rr.threshold(keep)
    cut, s_r = rr.replicate(lists, s, seed, r, keep)
    kept = [[int(h) for h in v if rr.keeps(h, seed, r, T)] for v in lists]
    assert s_r == len(kept[9]) and 400 < s_r < 600
    assert len(cut[0]) == 0 and len(cut[1]) == 0
    for v, kv, c in zip(lists, kept, cut):
        assert c.tolist() == kv[:s_r] and c.dtype == np.uint64
        assert all(a < b for a, b in zip(c.tolist(), c.tolist()[1:]))   # still ascending
    assert any(len(kv) < s_r for kv in kept[4:9]) and len(cut[8]) == min(len(kept[8]), s_r)
    everything = {}
    for v in lists:
        for h in v.tolist():
            everything.setdefault(h, rr.keeps(h, seed, r, T))
    for c, v in zip(cut, lists):
        inside = set(c.tolist())
        limit = c[-1] if len(c) else -1
        assert all((h in inside) == everything[h] for h in v.tolist() if h <= limit)
    # no list is full: s_r = s
    cut, s_r = rr.replicate(lists[:9], s, seed, r, keep)
    assert s_r == s and [len(c) for c in cut] == [len(kv) for kv in kept[:9]]


def test_a_replicate_that_keeps_nothing_of_a_full_list_raises():
    lists, s = lc.short()
    with pytest.raises(ValueError) as exc:
        rr.replicate(lists, s, 42, 2, 2.0 ** -31)
    assert "replicate 2" in str(exc.value) and "keep" in str(exc.value)
    # no full list: nothing to raise about
    assert rr.replicate(lists[:4], s, 42, 2, 2.0 ** -31)[1] == s

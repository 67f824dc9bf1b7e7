"""The rule of the jackknife support of search hits (tests/support_rule.py) on the cases of tests/support_cases.py: the values
the issue states for the near-tie case, the identity the device form relies on (given s_r the cut does not change a pair's
result: one walk over the kept, uncut lists gives what mo.compare gives over the cut ones), first summing to R, and keep = 1
giving mo.compare at s in every replicate.  CPU only."""
import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import resample_rule as rr
from tests import support_cases as cases
from tests import support_rule as rule

K = cases.K


def test_keep_mask_is_the_keep_function():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.integers(0, 2 ** 64, size=300, dtype=np.uint64), np.array([0, 1, 2 ** 64 - 1, 2 ** 63], np.uint64)])
    for seed in (42, 2 ** 64 - 1, 0):
        for r in (0, 1, 9999):
            for keep in (0.5, 1.0, 0.03):
                T = rr.threshold(keep)
                assert [bool(x) for x in rule.keep_mask(v, seed, r, T)] == [rr.keeps(int(h), seed, r, T) for h in v]


def test_near_tie_values():
    (Q,), refs = cases.near_tie()
    e = rule.support(Q, refs, list(range(8)), cases.S, K, 8, 0.5, 42)
    assert {i: int(c) for i, c in enumerate(e.first) if c} == {1: 6, 4: 1, 5: 1}
    assert int(e.rep_s.min()) == 472 and int(e.rep_s.max()) == 495
    f = rule.support_fast(Q, refs, list(range(8)), cases.S, K, 8, 0.5, 42)
    for name in ("first", "rep_best", "rep_s", "rep_common", "rep_denom"):
        assert np.array_equal(getattr(e, name), getattr(f, name)), name
    e64 = cases.expected(Q, refs, range(8), cases.S, 64, 0.5, 42)
    assert int((e64.first > 0).sum()) == 5 and int(e64.first.sum()) == 64
    assert ((e64.first > 0) & (e64.first < 64)).any()   # counting can be told from a constant


def test_plain_and_fast_rule_agree_on_short_lists():
    lists, rows = cases.ladder(), cases.ladder_cands()
    for i in (0, 2, 5, len(lists) - 1):
        cands = [lists[j] for j in rows[i]]
        e = rule.support(lists[i], cands, list(rows[i]), cases.S, K, 3, 0.5, 2 ** 64 - 1)
        f = rule.support_fast(lists[i], cands, list(rows[i]), cases.S, K, 3, 0.5, 2 ** 64 - 1)
        for name in ("first", "rep_best", "rep_s", "rep_common", "rep_denom"):
            assert np.array_equal(getattr(e, name), getattr(f, name)), (i, name)


def _sets():
    (Q,), refs = cases.near_tie()
    yield "near_tie", [Q] + list(refs)
    qs, lists, rows = cases.ties()
    yield "ties", [qs[0]] + [lists[j] for j in rows[0]]
    yield "ladder", list(cases.ladder())


@pytest.mark.parametrize("keep", [0.5, 0.03, 1.0])
def test_cut_does_not_change_a_pair(keep):
    """compare(cut(A), cut(B), s_r) == the walk over kept(A), kept(B) at s_r, for every (pair, replicate): 0 disagreements"""
    checked = 0
    for name, lists in _sets():
        for seed in (42, 2 ** 64 - 1):
            for r in range(4):
                try:
                    kept, s_r = rule.kept_lists(lists, cases.S, seed, r, keep)
                except ValueError:
                    continue
                for i in range(len(lists)):
                    for j in range(len(lists)):
                        if i == j or (name != "ladder" and i != 0):
                            continue
                        want = mo.compare(kept[j][:s_r], kept[i][:s_r], s_r, K)[:2]
                        assert rule.walk(kept[j], kept[i], s_r) == want, (name, seed, r, i, j)
                        assert mo.compare(kept[j], kept[i], s_r, K)[:2] == want
                        checked += 1
    assert checked > 500


def test_first_sums_to_replicates_and_ties_go_to_the_lower_reference():
    qs, lists, rows = cases.ties()
    for q, row, low in zip(qs, rows, (5, 77)):
        e = cases.expected(q, [lists[j] for j in row], row, cases.S, 8, 0.5, 42)
        assert int(e.first.sum()) == 8
        assert (e.rep_best == low).all() and e.first[row.index(low)] == 8
    lad, cand = cases.ladder(), cases.ladder_cands()
    for i, q in enumerate(lad):
        e = cases.expected(q, [lad[j] for j in cand[i]], cand[i], cases.S, 5, 0.5, 42)
        assert int(e.first.sum()) == 5
    none = rule.support_fast(lad[3], [], [], cases.S, K, 4, 0.5, 42)
    assert (none.rep_best == rule.NONE).all() and none.first.size == 0 and (none.rep_s == cases.S).all()


def test_keep_one_is_the_plain_comparison():
    (Q,), refs = cases.near_tie()
    e = rule.support_fast(Q, refs, list(range(8)), cases.S, K, 3, 1.0, 42)
    for i, c in enumerate(refs):
        common, denom, _ = mo.compare(c, Q, cases.S, K)
        assert (e.rep_common[i] == common).all() and (e.rep_denom[i] == denom).all()
    assert (e.rep_s == cases.S).all()
    lad, cand = cases.ladder(), cases.ladder_cands()
    i = len(lad) - 1
    e = rule.support_fast(lad[i], [lad[j] for j in cand[i]], list(cand[i]), cases.S, K, 2, 1.0, 7)
    for x, j in enumerate(cand[i]):
        assert tuple(e.rep_common[x]) == (mo.compare(lad[j], lad[i], cases.S, K)[0],) * 2


def test_a_replicate_without_hashes_fails():
    with pytest.raises(ValueError, match="replicate 0 keeps no hash"):
        rule.support_fast(np.array([5], np.uint64), [np.array([5], np.uint64)], [0], 1, K, 4, 0.03, 42)

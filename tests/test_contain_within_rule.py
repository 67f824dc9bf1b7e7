"""The rule of the unbounded containment call (tests/contain_within_rule.py) against the two rules it is built on: its CSR is
the filter of the containment's table (tests/contain_cases.py: expected) through the search's hit test, and every row of it,
sorted by the search's order and cut to 64, is the containment search's result (tests/contain_search_rule.py: search)."""
import numpy as np
import pytest

from tests import contain_cases as cc
from tests import contain_search_rule as search_rule
from tests import contain_within_cases as cwc
from tests import contain_within_rule as rule

K = cc.K
BOUNDS = ((0.0, 1), (0.9, 1), (0.95, 10), (1.0, 1), (1.5, 1))


def filtered(shared, n_qry, n_ref, min_identity, min_shared):
    """the table filtered pair by pair, with nothing of the rule module but the hit test it names"""
    nq, nr = shared.shape
    row_off, flat = [0], []
    for q in range(nq):
        for r in range(nr):
            if search_rule.is_hit(int(shared[q, r]), int(n_ref[q, r]), K, min_identity, min_shared):
                flat.append((r, int(shared[q, r]), int(n_ref[q, r]), int(n_qry[q, r])))
        row_off.append(len(flat))
    return row_off, flat


@pytest.mark.parametrize("name", ("crafted",) + cc.NAMES)
def test_csr_is_the_filtered_table_and_its_rows_are_the_search(name):
    counts = cc.expected(name)
    for min_identity, min_shared in BOUNDS:
        got = rule.csr(*counts, K, min_identity, min_shared)
        row_off, flat = filtered(*counts, min_identity, min_shared)
        assert got[0].dtype == np.uint64 and got[0].tolist() == row_off and all(a.dtype == np.uint32 for a in got[1:])
        assert list(zip(*(a.tolist() for a in got[1:]))) == flat
        per_query = rule.rows_of_arrays(got)
        assert all(h == sorted(h) for h in per_query)                        # ascending by reference
        assert [search_rule.ranked(h)[:64] for h in per_query] == search_rule.search(*counts, K, 64, min_identity, min_shared)
        if min_identity > 1:
            assert not flat
        if min_identity <= 0:
            assert len(flat) == int((counts[0] >= min_shared).sum())   # every pair that shares at least min_shared hashes


def test_crowd_at_every_bound():
    counts = cwc.matrix()
    for min_identity, min_shared in cwc.bounds():
        got = cwc.expected(min_identity, min_shared)
        row_off, flat = filtered(*counts, min_identity, min_shared)
        assert got[0].tolist() == row_off and list(zip(*(a.tolist() for a in got[1:]))) == flat
        cut = [search_rule.ranked(h)[:64] for h in rule.rows_of_arrays(got)]
        assert cut == search_rule.search(*counts, K, 64, min_identity, min_shared)
    assert max(len(h) for h in rule.rows_of_arrays(cwc.expected(*cwc.MAIN[0]))) > 64   # what the search cannot return


def test_text_orders_and_the_p_value_filter():
    shared, n_qry, n_ref = cwc.matrix()
    refs = [f"r{i}" for i in range(cwc.NR)]
    qrys = [f"q{i}" for i in range(cwc.NQ)]
    sizes = [5000.0] * cwc.NQ
    best = rule.text_rows(refs, qrys, sizes, shared, n_qry, n_ref, K, 0.95, 10, order="best")
    by_ref = rule.text_rows(refs, qrys, sizes, shared, n_qry, n_ref, K, 0.95, 10, order="ref")
    assert sorted(best) == sorted(by_ref) and best != by_ref and len(best) == int(cwc.expected(0.95, 10)[0][-1])
    assert [r[1] for r in best] == sorted((r[1] for r in best), key=lambda n: int(n[1:]))   # queries in order, none without hits
    some = rule.text_rows(refs, qrys, sizes, shared, n_qry, n_ref, K, 0.0, 1, max_p_value=1e-10, order="ref")
    every = rule.text_rows(refs, qrys, sizes, shared, n_qry, n_ref, K, 0.0, 1, order="ref")
    assert 0 < len(some) < len(every) and some == [r for r in every if r[3] <= 1e-10]

"""The rule of the winner-take-all containment (tests/contain_winner_rule.py) on its own: the consequences it must have on
every shared case, the values of the small cases worked out by hand, and the property the mode exists for on the clades.
CPU only."""
import numpy as np
import pytest

from tests import contain_cases as cc
from tests import contain_rule as rule
from tests import contain_winner_cases as wc
from tests import contain_winner_rule as wrule


@pytest.mark.parametrize("name", wc.NAMES)
def test_consequences(name):
    won, shared, n_qry, n_ref, distinct, winners = wc.expected(name)
    lengths = wc.rows_of(name)[6]
    wrule.check_consequences(won, shared, n_qry, n_ref, distinct, lengths)
    plain = cc.expected(name) if name in cc.NAMES or name == "crafted" else None
    if plain is not None:   # shared, n_qry, n_ref are the plain call's
        for a, b in zip((shared, n_qry, n_ref), plain):
            assert np.array_equal(a, b)
    Q, q_len, R, r_len, s_q, s_r, _ = wc.rows_of(name)
    rl = [rule.the_list(R[j], r_len[j], s_r) for j in range(len(r_len))]
    for i in range(min(len(winners), 12)):   # the sum over r is the number of distinct values found, counted another way
        q = rule.the_list(Q[i], q_len[i], s_q)
        union = set()
        for r in rl:
            union |= wrule.found(q, r, s_q, s_r)
        assert set(winners[i]) == union and len(union) == distinct[i]


def test_tau_and_ties():
    won, shared, n_qry, n_ref, distinct, winners = wc.expected("tau_and_ties")
    assert shared.tolist() == [[8, 4, 8, 3, 1]] and n_ref.tolist() == [[8, 5, 8, 8, 2]]
    assert won.tolist() == [[8, 2, 0, 0, 1]] and distinct.tolist() == [11]
    assert winners[0][90] == 1 and winners[0][100] == 1   # A holds them only behind its bound
    assert winners[0][160] == 4                           # tau is inclusive
    won2, shared2, _, n_ref2, distinct2, _ = wc.expected("tau_and_ties_lengths")
    assert np.array_equal(shared2, shared) and np.array_equal(n_ref2, n_ref)
    assert won2.tolist() == [[0, 2, 8, 0, 1]] and distinct2.tolist() == [11]


def test_crafted():
    won, shared, n_qry, n_ref, distinct, winners = wc.expected("crafted")
    assert won.tolist() == [[0, 0, 0, 0, 0], [0, 3, 0, 0, 0], [0, 3, 5, 0, 0], [0, 0, 0, 0, 0], [0, 3, 0, 3, 0], [0, 1, 1, 3, 0]]
    assert distinct.tolist() == [0, 3, 8, 0, 6, 5]
    assert winners[5][2 ** 64 - 1] == 3   # 2^64 - 1 is a hash like any other and can be won


def test_clades_separate():
    """what the mode exists for: the plain rows of a clade are near-identical, the winner rows point to one reference"""
    won, shared, n_qry, n_ref, distinct, winners = wc.expected("clades")
    assert won.shape == (7, 14)
    for c in range(3):   # each base wins all of its n_ref for its own genome ...
        assert won[c, 4 * c] == n_ref[c, 4 * c] == 200
        assert (shared[c, 4 * c:4 * c + 4] >= 180).all()   # ... where the plain counts cannot tell the members apart
    m = wc.CLADE_MIXED_QUERY
    assert won[m, 0] == n_ref[m, 0] == 200 and won[m, 8] == n_ref[m, 8] == 200   # ... and for the mixed culture
    assert (shared[m, 0:4] >= 180).all() and (shared[m, 8:12] >= 180).all()
    # a query equal to the 0.2 % copy ties with its base at 200 / 200: the lower index wins
    q = wc.CLADE_COPY_QUERY
    assert shared[q, 0] == n_ref[q, 0] == 200 and shared[q, 1] == n_ref[q, 1] == 200
    assert won[q, 0] == 200 and won[q, 1] == int(distinct[q]) - 200 - int(won[q, 2:].sum())
    # a 17-hash query: the 40-hash reference at 17 / 40 beats three full references at 17 / 200
    q, r = wc.CLADE_SHORT_QUERY, wc.CLADE_SHORT_REF
    assert (shared[q, r], n_ref[q, r], won[q, r]) == (17, 40, 17)
    full = [j for j in range(14) if shared[q, j] == 17 and n_ref[q, j] == 200]
    assert len(full) == 3 and won[q, full].sum() == 0 and distinct[q] == 17


def test_rows_print_won():
    won, shared, n_qry, n_ref, distinct, _ = wc.expected("tau_and_ties")
    rows = wrule.expected_rows(list("ABCDE"), ["q"], [16], won, n_qry, n_ref, 21)
    assert [(r[0], r[4], r[5]) for r in rows] == [("A", 8, 8), ("B", 2, 5), ("C", 0, 8), ("D", 0, 8), ("E", 1, 2)]
    assert rows[0][2] == 1.0 and rows[2][2] == 0.0 and rows[2][3] == 1.0
    assert rows[1][2] == rule.identity(2, 5, 21) and rows[1][3] == rule.p_value(2, 5, 16, 21)

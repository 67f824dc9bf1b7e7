"""The rule of the containment from sketches (tests/contain_rule.py) against brute-force Python sets on the shared cases, the
property that motivates the mode, and the row text.  CPU only."""
import numpy as np
import pytest

from tests import contain_cases as cc
from tests import contain_rule as rule
from tests import triangle_cases as tc

FULL = 2 ** 64 - 1


def brute(q, r, s_q, s_r):
    """the statement itself, with sets"""
    q, r = [int(x) for x in q[:s_q]], [int(x) for x in r[:s_r]]
    bq = q[-1] if len(q) == s_q else FULL
    br = r[-1] if len(r) == s_r else FULL
    tau = min(bq, br)
    A, B = {x for x in q if x <= tau}, {x for x in r if x <= tau}
    return len(A & B), len(A), len(B)


@pytest.mark.parametrize("name", cc.NAMES)
def test_rule_equals_brute_force(name):
    qs, rs, s_q, s_r = cc.case(name)
    shared, n_qry, n_ref = cc.expected(name)
    step = 7 if len(qs) * len(rs) > 4000 else 1   # every seventh pair of the large case
    at = 0
    for i, q in enumerate(qs):
        for j, r in enumerate(rs):
            at += 1
            if at % step:
                continue
            assert (int(shared[i, j]), int(n_qry[i, j]), int(n_ref[i, j])) == brute(q, r, s_q, s_r), (name, i, j)
    assert (shared <= np.minimum(n_qry, n_ref)).all()


def test_crafted_edge_cases():
    Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows()
    shared, n_qry, n_ref = cc.expected("crafted")
    got = lambda i, j: (int(shared[i, j]), int(n_qry[i, j]), int(n_ref[i, j]))
    for i in range(6):
        for j in range(5):
            assert got(i, j) == brute(Q[i][:min(q_len[i], s_q)], R[j][:min(r_len[j], s_r)], s_q, s_r), (i, j)
    assert got(0, 0) == (0, 0, 0) and got(0, 2) == (0, 0, 8)         # an empty list has no bound: the other list's counts
    assert got(1, 1) == (3, 3, 3) and got(1, 4) == (1, 3, 3)         # two short lists: tau = 2^64 - 1, everything counts
    assert got(2, 2) == (8, 8, 8)                                    # tau = 40, held by both; 45 and 50 lie behind s_r
    assert got(4, 2) == (3, 16, 6)                                   # tau = 32 between 30 and 35 of the reference
    assert got(3, 2) == (0, 0, 8)                                    # disjoint: the query begins above tau
    assert got(5, 3) == (3, 16, 8) and got(5, 4) == (1, 16, 3)       # 2^64 - 1 is a hash both lists hold
    assert got(2, 1) == (3, 16, 3) and got(1, 2) == (3, 3, 8)        # short against full, both ways round


@pytest.mark.parametrize("s_q,s_r", [(1000, 1000), (1000, 200), (200, 1000), (50000, 1000), (300, 5000), (100000, 100000)])
def test_a_superset_query_holds_every_reference_hash_of_the_window(s_q, s_r):
    """The property the mode exists for: a query genome that contains the reference genome gives shared == n_ref at any pair
    of sketch sizes, however much else it holds -- where the Jaccard index of the same pair falls with every foreign hash."""
    rng = np.random.default_rng([s_q, s_r])
    ref = cc.genome(rng, 20000)
    for extra in (0, 5000, 60000, 220000):
        qry = cc.union(ref, cc.genome(rng, extra)) if extra else ref
        shared, n_qry, n_ref = rule.counts(rule.the_list(qry, len(qry), s_q), rule.the_list(ref, len(ref), s_r), s_q, s_r)
        assert shared == n_ref > 0 and n_qry >= n_ref, (extra, shared, n_qry, n_ref)
        assert rule.identity(shared, n_ref, 21) == 1.0
    unrelated = cc.genome(rng, 80000)
    shared, n_qry, n_ref = rule.counts(rule.the_list(unrelated, len(unrelated), s_q), rule.the_list(ref, len(ref), s_r), s_q, s_r)
    assert shared == 0 and rule.identity(shared, n_ref, 21) == 0.0


def test_identity_and_p_value_at_the_corners():
    assert rule.identity(0, 0, 21) == 0.0 and rule.p_value(0, 0, 1e6, 21) == 1.0
    assert rule.identity(5, 5, 21) == 1.0 and rule.identity(0, 5, 21) == 0.0 and rule.p_value(0, 5, 1e6, 21) == 1.0
    assert rule.identity(3, 4, 2) == pytest.approx(0.75 ** 0.5)
    assert 0.0 < rule.p_value(3, 4, 1e6, 21) < 1e-10


def test_row_text_round_trip():
    shared, n_qry, n_ref = (np.array(x, np.uint32) for x in ([[5, 0], [2, 0]], [[9, 4], [7, 0]], [[5, 3], [4, 0]]))
    rows = rule.expected_rows(["r0", "r1"], ["q0", "q1"], [1e6, 2e6], shared, n_qry, n_ref, 21)
    assert [(r[0], r[1], r[4], r[5], r[6]) for r in rows] == [("r0", "q0", 5, 5, 9), ("r1", "q0", 0, 3, 4), ("r0", "q1", 2, 4, 7), ("r1", "q1", 0, 0, 0)]
    text = "".join("%s\t%s\t%g\t%g\t%d/%d\t%d/%d\n" % (r[0], r[1], r[2], r[3], r[4], r[5], r[4], r[6]) for r in rows)
    assert rule.same_rows(rule.rows_of_text(text), rows)
    kept = rule.expected_rows(["r0", "r1"], ["q0", "q1"], [1e6, 2e6], shared, n_qry, n_ref, 21, min_identity=0.5)
    assert [(r[0], r[1]) for r in kept] == [("r0", "q0"), ("r0", "q1")]
    assert not rule.same_rows(rule.rows_of_text(text), kept)

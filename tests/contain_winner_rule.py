"""The rule of the winner-take-all containment from sketches (mhx_dist_contain_winner, mhx_contain_files_winner) as a plain
statement in Python integers and Fraction, on top of tests/contain_rule.py (list, bound, tau, shared, n_qry, n_ref stay as
they are there).  Shared by the winner tests; not a test module itself.  Nothing here is mash's.

Per query q:

    found(q, r)  = {x in list(q) and list(r): x <= tau(q, r)}; its size is the plain shared(q, r).  A value a reference holds
                   only above its own bound is not found there, neither is a value behind a list's effective length.
    r ranks before r' by the greater exact ratio shared(q, r) / n_ref(q, r) (Fraction), then the greater genome length
                   ref_length[r] (all equal when none are given), then the LOWER INDEX.  A reference with n_ref == 0 has found
                   nothing and never competes.
    winner(q, x) = for every x in the union of found(q, r) over r: the best-ranked r with x in found(q, r)
    won(q, r)    = #{x in found(q, r): winner(q, x) = r}

    won <= shared; won == shared for the best-ranked reference of a query; sum_r won(q, r) = #distinct values found for q.
    identity and p-value of a winner row follow from `won` with n_ref and the set size unchanged (tests/screen_winner_rule.py
    does the same for the screen); the row prints `won` in both fractions.
"""
import bisect
from fractions import Fraction

import numpy as np

from tests import contain_rule as rule


def rank_key(shared, n_ref, length, index):
    """greater is better; only references with n_ref > 0 are ever compared"""
    return (Fraction(int(shared), int(n_ref)), int(length), -int(index))


def found(q, r, s_q, s_r):
    """the set of values found for the pair of two lists (rule.the_list)"""
    tau = min(rule.bound(q, s_q), rule.bound(r, s_r))
    return set(q[:bisect.bisect_right(q, tau)]).intersection(r[:bisect.bisect_right(r, tau)])


def of_lists(ql, rl, s_q, s_r, ref_length=None):
    """(won, shared, n_qry, n_ref [nq, nr], distinct [nq], winners) over lists (rule.the_list); winners[q] maps every found
    value of query q to the index of its winner"""
    nq, nr = len(ql), len(rl)
    lengths = [0] * nr if ref_length is None else [int(x) for x in ref_length]
    assert len(lengths) == nr
    out = np.zeros((4, nq, nr), np.uint32)
    distinct = np.zeros(nq, np.int64)
    winners = []
    for i, q in enumerate(ql):
        sets = []
        for j, r in enumerate(rl):
            out[1:, i, j] = rule.counts(q, r, s_q, s_r)
            sets.append(found(q, r, s_q, s_r))
            assert len(sets[j]) == out[1, i, j]
        key = [rank_key(out[1, i, j], out[3, i, j], lengths[j], j) if out[3, i, j] else None for j in range(nr)]
        best = {}
        for j in range(nr):
            for x in sets[j]:
                h = best.get(x)
                if h is None or key[j] > key[h]:
                    best[x] = j
        for x, j in best.items():
            out[0, i, j] += 1
        distinct[i] = len(best)
        winners.append(best)
    return out[0], out[1], out[2], out[3], distinct, winners


def matrix(qs, rs, s_q, s_r, ref_length=None):
    """over lists given as arrays, each cut at its set's sketch size"""
    return of_lists([rule.the_list(v, len(v), s_q) for v in qs], [rule.the_list(v, len(v), s_r) for v in rs], s_q, s_r, ref_length)


def matrix_of_rows(Q, q_len, R, r_len, s_q, s_r, ref_length=None):
    """the same over row matrices with lengths (what the device calls take)"""
    return of_lists([rule.the_list(Q[i], q_len[i], s_q) for i in range(len(q_len))], [rule.the_list(R[j], r_len[j], s_r) for j in range(len(r_len))],
                    s_q, s_r, ref_length)


def best_ranked(shared, n_ref, ref_length=None):
    """per query the index of the best-ranked reference, -1 where none competes"""
    nq, nr = shared.shape
    lengths = [0] * nr if ref_length is None else [int(x) for x in ref_length]
    out = []
    for i in range(nq):
        keys = [(rank_key(shared[i, j], n_ref[i, j], lengths[j], j), j) for j in range(nr) if n_ref[i, j]]
        out.append(max(keys)[1] if keys else -1)
    return out


def check_consequences(won, shared, n_qry, n_ref, distinct, ref_length=None):
    """what follows from the rule, asserted on its own output and on anything that claims to equal it"""
    assert (won <= shared).all()
    assert np.array_equal(won.sum(axis=1, dtype=np.int64), distinct)
    for i, j in enumerate(best_ranked(shared, n_ref, ref_length)):
        if j >= 0:
            assert won[i, j] == shared[i, j], (i, j)
    assert (won[n_ref == 0] == 0).all()


def expected_rows(ref_names, qry_names, qry_sizes, won, n_qry, n_ref, k, min_identity=0.0, max_p_value=1.0):
    """the rows of contain -w: contain_rule.expected_rows with `won` in the place of `shared`"""
    return rule.expected_rows(ref_names, qry_names, qry_sizes, won, n_qry, n_ref, k, min_identity, max_p_value)

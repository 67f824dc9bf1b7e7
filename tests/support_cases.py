"""The cases of the jackknife support of search hits (mhx_dist_support), shared by the rule test, the CPU emulation test and the
GPU tests; what the rule (tests/support_rule.py) says about a case is computed once per process.  Not a test module itself.

    near_tie   a base list, six copies with 20 % of the hashes replaced, the base's first 300 hashes and an independent list as
               references; the query is another 20 % copy: at keep 0.5, seed 42 the winner changes from replicate to
               replicate (R = 8: reference 1 six times, 4 and 5 once; s_r 472 .. 495)
    ties       queries 24 and 25 of search_cases (copies of lists 5 and 141) against candidates that hold the identical
               references 5, 190, 191, 196 and the duplicates 77, 141: the lower index wins every replicate
    ladder     the lists of test_resample_emulation.ladder_lists (lengths 0, 1, 63, 64, 65, 255, 256, 257, 1000, ...; 0 and
               2^64 - 1 among the hashes), each as a query against the others: complete sets, unions below s_r, denom < s_r, and
               the empty query against the empty reference (0/0)
    long       three candidates and a query of 50 000 hashes (AuriClass's sketch size)
"""
import functools

import numpy as np

from tests import search_cases as sc
from tests import support_rule as rule
from tests import triangle_cases as tc

K = 21
S = 1000


@functools.lru_cache(maxsize=None)
def near_tie():
    """(queries, references)"""
    rng = np.random.default_rng(20261019)
    base = tc.sketch_like(rng, 1000)
    refs = [tc.mutate(rng, base, 0.2) for _ in range(6)] + [base[:300].copy(), tc.sketch_like(rng, 1000)]
    return (tc.mutate(rng, base, 0.2),), tuple(refs)


TIE_REFS = (196, 5, 77, 191, 141, 190, 3, 10)   # not in index order: the order of the candidates must not matter


@functools.lru_cache(maxsize=None)
def ties():
    """(queries, references, candidate rows): the references are all of set200, the candidates index into them"""
    lists, _ = tc.set200()
    return (sc.queries()[24], sc.queries()[25]), lists, (TIE_REFS, TIE_REFS)


@functools.lru_cache(maxsize=None)
def ladder():
    from tests.test_resample_emulation import ladder_lists
    lists = ladder_lists()
    lists.insert(1, np.zeros(0, np.uint64))   # a second empty list: the empty query meets an empty reference
    return tuple(lists)


def ladder_cands():
    """per query of ladder() the indices of the others"""
    n = len(ladder())
    return tuple(tuple(j for j in range(n) if j != i) for i in range(n))


@functools.lru_cache(maxsize=None)
def long():
    lists, s = tc.long_set(4, 50000)
    return (lists[3],), (lists[2], lists[0], lists[1]), s


def _key(a):
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def _expected(qkey, ckeys, refs, s, replicates, keep, seed):
    Q = np.frombuffer(qkey, np.uint64)
    cands = [np.frombuffer(c, np.uint64) for c in ckeys]
    return rule.support_fast(Q, cands, list(refs), s, K, replicates, keep, seed)


def expected(Q, cands, refs, s, replicates, keep, seed):
    """the rule for one query, remembered"""
    return _expected(_key(Q), tuple(_key(c) for c in cands), tuple(int(x) for x in refs), s, replicates, keep, seed)


def expected_call(queries, references, cand_rows, top, s, replicates, keep, seed):
    """The arrays a call returns: first [nq, top], rep_best, rep_s [nq, R], rep_common, rep_denom [nq, top, R] (zero where the
    rule says nothing) and a mask of the (query, candidate) cells that count."""
    nq = len(queries)
    first = np.zeros((nq, top), np.uint32)
    best, rs = np.zeros((nq, replicates), np.uint32), np.zeros((nq, replicates), np.uint32)
    common, denom = np.zeros((nq, top, replicates), np.uint32), np.zeros((nq, top, replicates), np.uint32)
    valid = np.zeros((nq, top), bool)
    for i, Q in enumerate(queries):
        row = list(cand_rows[i])
        e = expected(Q, [references[j] for j in row], row, s, replicates, keep, seed)
        m = len(row)
        first[i, :m], best[i], rs[i], common[i, :m], denom[i, :m], valid[i, :m] = e.first, e.rep_best, e.rep_s, e.rep_common, e.rep_denom, True
    return first, best, rs, common, denom, valid

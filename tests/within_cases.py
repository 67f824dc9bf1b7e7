"""The case set of the bounded neighbourhood call (mhx_dist_within), shared by the CPU tests and the GPU tests, and what the
oracle says about it: mo.compare of every (query, reference) pair, computed once per process; the expected CSR is those
pairs put through tests/within_rule.py.

k = 21, s = 128.  330 references -- 11 slices, the last of 10 lists -- against 70 queries (not a multiple of 4):
    references  a base list B of 128 hashes; the even indices 0 .. 298 are mutations of B whose share of replaced hashes runs
                evenly from 0.005 to 0.6 -- a crowd of 150 lists spread over ten slices; 301 is empty, 303 is B[:17], 305, 307 and
                329 are copies of B, the rest are independent
    queries     0 is B, 1 a 10 % mutation of B, 2 empty, 3 is B[:17], the other 66 independent
so queries 0 and 1 have more than the 64 hits a search list holds at bounds that are real thresholds (0.02 cuts the crowd in
two: 89 and 71 hits with this seed; 0.05 keeps nearly all of it: 152 and 151), queries 4 .. 69 have no hit below 1, and at
max_dist = 0 the hits are 3, 0, 1, 1.  (The seed was chosen among those for which these conditions hold: a 0.5 % mutation of
128 hashes is a copy of B more often than not, which would add a fourth hit at 0.)

big(): the same construction with 1920 references (60 slices), for the run of one query per block over more blocks than one
group of flag words.
"""
import functools

import numpy as np

from tests import search_cases as sc
from tests import triangle_cases as tc
from tests import within_rule as rule

K = 21
S = 128
NQ = 70
NR = 330


def build(nr, seed):
    rng = np.random.default_rng(seed)
    B = tc.sketch_like(rng, S)
    drops = np.linspace(0.005, 0.6, 150)
    refs = [tc.mutate(rng, B, drops[i // 2])[:S] if i % 2 == 0 and i < 300 else tc.sketch_like(rng, S) for i in range(nr)]
    refs[301] = np.zeros(0, np.uint64)
    refs[303] = B[:17].copy()
    for i in (305, 307, 329):
        refs[i] = B.copy()
    qrys = [B.copy(), tc.mutate(rng, B, 0.10)[:S], np.zeros(0, np.uint64), B[:17].copy()]
    qrys += [tc.sketch_like(rng, S) for _ in range(NQ - len(qrys))]
    return tuple(refs), tuple(qrys)


@functools.lru_cache(maxsize=None)
def case_set():
    """(references, queries)"""
    return build(NR, 61)


@functools.lru_cache(maxsize=None)
def matrix():
    refs, qrys = case_set()
    return sc.oracle_matrix(qrys, refs, S, K)


@functools.lru_cache(maxsize=None)
def big():
    """(references, queries, (common, denom, dist)) of the 1920-reference set"""
    refs, qrys = build(1920, 99)
    return refs, qrys, sc.oracle_matrix(qrys, refs, S, K)


@functools.lru_cache(maxsize=None)
def exact_bound():
    """a bound that IS the distance of an occurring pair: query 1 against the middle one of its hits below 0.05, by distance"""
    d = matrix()[2][1]
    inside = np.sort(d[(d > 0.0) & (d < 0.05)])
    return float(inside[len(inside) // 2])


def bounds():
    x = exact_bound()
    return [-1.0, 0.0, 0.005, 0.02, x, float(np.nextafter(x, 0.0)), 0.05, 1.0]


def hits_per_query(max_dist, nq=NQ, nr=NR):
    return (matrix()[2][:nq, :nr] <= max_dist).sum(axis=1)


@functools.lru_cache(maxsize=None)
def expected(max_dist, nq=NQ, nr=NR):
    """the rule's CSR for queries [:nq] against the first nr references"""
    common, denom, dist = matrix()
    return rule.csr_from_matrix(common[:nq, :nr], denom[:nq, :nr], dist[:nq, :nr], max_dist)

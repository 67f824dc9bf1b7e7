"""The case set of the unbounded containment call (mhx_dist_contain_within), shared by the CPU tests and the GPU tests, and what
the rule (tests/contain_within_rule.py over tests/contain_rule.py) says about it, computed once per process.  Not a test
module itself.  A "genome" is a set of random hashes, a sketch its s smallest (tests/contain_cases.py).

crowd: k = 21, s_q = 128, s_r = 64.  330 references -- ten full slices and one of 10 -- against 70 queries (not a multiple of 4):
    references  a base genome B of 2000 hashes; the indices i with i % 11 < 5 -- 150 of them, in all eleven slices, 320 .. 323
                of the last -- are mutations of B whose shares of replaced hashes run evenly from 0 to 0.98, dealt out so that every
                slice gets mild and heavy ones; 7 is empty, 18 is a genome of 23 hashes (a short list), the rest are
                independent genomes
    queries     0 .. 29: B (even) or a mutation of B by 1 % .. 15 % (odd), united with a contaminant of one to three times its
                size; 30 .. 66 unrelated genomes; 67 empty; 68 the short list B[:23]; 69 reference 18's genome inside a larger one
so the queries that hold B hold a crowd of its copies: at identity 0.9 a share of 0.9^21 = 0.11 passes and the crowd is nearly
all of the 150, at 0.95 (a share of 0.34) about two thirds of it, both well beyond the 64 hits a search list holds; the
unrelated queries hold nothing, and at (0, 1) the call has more hits than the 4096 a file-level batch has room for at first.
The conditions on the set are asserted at import.
"""
import functools

import numpy as np

from tests import contain_cases as cc
from tests import contain_rule as cr
from tests import contain_within_rule as rule
from tests import triangle_cases as tc

K = cc.K
S_Q = 128
S_R = 64
NQ = 70
NR = 330
MAIN = ((0.9, 1), (0.95, 10))   # the two main bounds


@functools.lru_cache(maxsize=None)
def crowd():
    """(queries, references, s_q, s_r), a case as tests/contain_cases.py has them"""
    rng = np.random.default_rng(330070)
    B = cc.genome(rng, 2000)
    in_crowd = [i for i in range(NR) if i % 11 < 5]
    drops = np.linspace(0.0, 0.98, len(in_crowd))
    refs = [cc.genome(rng, 2000) for _ in range(NR)]
    for j, i in enumerate(in_crowd):
        refs[i] = tc.mutate(rng, B, drops[(37 * j) % len(drops)])
    refs[7] = np.zeros(0, np.uint64)
    refs[18] = cc.genome(rng, 23)
    qrys = [cc.union(B if i % 2 == 0 else tc.mutate(rng, B, 0.01 * (i // 2 + 1)), cc.genome(rng, 2000 * (1 + i % 3))) for i in range(30)]
    qrys += [cc.genome(rng, 2000 + 100 * i) for i in range(37)]
    qrys += [np.zeros(0, np.uint64), B[:23].copy(), cc.union(refs[18], cc.genome(rng, 300))]
    assert len(in_crowd) == 150 and len(qrys) == NQ and len(refs) == NR
    return tuple(qrys), tuple(refs), S_Q, S_R


@functools.lru_cache(maxsize=None)
def matrix():
    """(shared, n_qry, n_ref) [70, 330] by the rule of the containment"""
    return cr.matrix(*crowd())


def rows_of():
    """crowd as the row matrices a device call takes (tests/contain_cases.py: rows_of)"""
    qs, rs, s_q, s_r = crowd()
    qs, rs = tuple(v[:s_q + 3] for v in qs), tuple(v[:s_r + 3] for v in rs)
    Q, q_len = tc.pad_rows(list(qs), 144)
    R, r_len = tc.pad_rows(list(rs), 144)
    return Q, q_len, R, r_len, s_q, s_r


@functools.lru_cache(maxsize=None)
def exact_bound():
    """a bound that IS the identity of an occurring pair: query 1 against the middle one, by identity, of its pairs with an
    identity strictly between 0.9 and 1"""
    shared, _, n_ref = matrix()
    ids = sorted({cr.identity(int(c), int(b), K) for c, b in zip(shared[1], n_ref[1]) if b})
    inside = [x for x in ids if 0.9 < x < 1.0]
    return float(inside[len(inside) // 2])


def bounds():
    """the (min_identity, min_shared) pairs of the tests"""
    x = exact_bound()
    return [(0.0, 1), MAIN[0], MAIN[1], (x, 1), (float(np.nextafter(x, 0.0)), 1), (float(np.nextafter(x, 2.0)), 1), (1.0, 1), (1.5, 1)]


@functools.lru_cache(maxsize=None)
def expected(min_identity, min_shared, nq=NQ, nr=NR):
    """the rule's CSR for queries [:nq] against the first nr references: (row_off, ref, shared, n_ref, n_qry)"""
    shared, n_qry, n_ref = matrix()
    return rule.csr(shared[:nq, :nr], n_qry[:nq, :nr], n_ref[:nq, :nr], K, min_identity, min_shared)


def hits_per_query(min_identity, min_shared):
    return np.diff(expected(min_identity, min_shared)[0].astype(np.int64))


def _conditions():
    a, b = hits_per_query(*MAIN[0]), hits_per_query(*MAIN[1])
    assert ((a > 64).sum() >= 2 or (b > 64).sum() >= 2), "at one of the two main bounds at least two queries pass 64 hits"
    big = np.flatnonzero((a > 64) | (b > 64))
    assert (a[big] != b[big]).all(), "their counts differ between the two bounds"
    assert (hits_per_query(0.0, 1) == 0).any(), "a query without a hit"
    assert hits_per_query(0.0, 1).sum() > 4096, "more hits than the first buffers of a file-level batch hold"
    slices = set((expected(*MAIN[0])[1] // 32).tolist())
    assert slices == set(range(11)), "hits in every slice, the last one included"
    x = exact_bound()
    at, below, above = (int(expected(v, 1)[0][-1]) for v in (x, float(np.nextafter(x, 0.0)), float(np.nextafter(x, 2.0))))
    assert below == at > above, "the bound that is a pair's identity keeps the pair, the next double above drops it"


_conditions()

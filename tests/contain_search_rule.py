"""The rule of the containment search (mhx_dist_contain_search, mhx_contain_files_search) as a plain statement in Python
integers, built on the rule of the containment itself (tests/contain_rule.py).  Shared by the containment search tests; not a
test module itself.  Nothing here is mash's: mash has no such command.

    candidate(q, r) = (r, shared, n_ref, n_qry): the three integers of contain_rule.counts for that pair
    hit        = shared >= min_shared (min_shared >= 1: a pair that shares nothing is never a hit, nor one with n_ref == 0) and
                 identity(shared, n_ref, k) >= min_identity, the identity of contain_rule: 1 when shared == n_ref, otherwise
                 (shared / n_ref) ** (1 / k) in libm doubles
    rank       = a is better than b iff its share shared / n_ref is larger, compared exactly as a cross product in integers;
                 on equal shares the larger `shared` (200/200 before 3/3); on equal `shared` the lower reference index.
                 References are distinct: a total order.
    result     = per query the first min(top, hits) hits in rank order, top = 1 .. 64
    need[n]    = the least `shared` that is a hit at n_ref = n, n + 1 when there is none: what the host hands to the device
    text       = for every query sketch, in argument order and then file order, its result as contain rows
                 "reference\\tquery\\tidentity\\tp\\tshared/n_ref\\tshared/n_qry\\n", best first; rows with p > max_p_value are
                 dropped from the result already chosen -- nothing moves up into their place
"""
import functools

import numpy as np

from tests import contain_rule as cr

MAX_TOP = 64


def is_hit(shared, n_ref, k, min_identity=0.0, min_shared=1):
    return n_ref > 0 and shared >= max(1, min_shared) and cr.identity(shared, n_ref, k) >= min_identity


def better(a, b):
    """a, b = (ref, shared, n_ref, ...)"""
    l, r = a[1] * b[2], b[1] * a[2]
    if l != r:
        return l > r
    if a[1] != b[1]:
        return a[1] > b[1]
    return a[0] < b[0]


def ranked(cands):
    return sorted(cands, key=functools.cmp_to_key(lambda a, b: -1 if better(a, b) else (1 if better(b, a) else 0)))


def select(cands, k, top, min_identity=0.0, min_shared=1):
    """cands = [(ref, shared, n_ref, n_qry)] of one query -> its result"""
    assert 1 <= top <= MAX_TOP and min_shared >= 1
    return ranked([c for c in cands if is_hit(c[1], c[2], k, min_identity, min_shared)])[:top]


def search(shared, n_qry, n_ref, k, top, min_identity=0.0, min_shared=1):
    """the [nq, nr] matrices of contain_rule.matrix in, per query [(ref, shared, n_ref, n_qry)]"""
    nq, nr = shared.shape
    return [select([(r, int(shared[q, r]), int(n_ref[q, r]), int(n_qry[q, r])) for r in range(nr)], k, top, min_identity, min_shared) for q in range(nq)]


def need_table(limit, k, min_identity=0.0, min_shared=1):
    """need[0 .. limit] by the definition, one n after the other"""
    out = []
    for n in range(limit + 1):
        out.append(next((c for c in range(1, n + 1) if is_hit(c, n, k, min_identity, min_shared)), n + 1))
    return out


def arrays(results, top):
    """the results as the host form's outputs: (hit_ref, hit_shared, hit_n_ref, hit_n_qry) [nq, top], zero behind n_hits [nq]"""
    out = np.zeros((4, len(results), top), np.uint32)
    for q, hits in enumerate(results):
        for t, h in enumerate(hits):
            out[:, q, t] = h
    return out[0], out[1], out[2], out[3], np.array([len(h) for h in results], np.uint32)


def search_np(shared, n_qry, n_ref, need, top):
    """arrays(search(..)) for sets too large for the plain form, vectorised: the hit test through the need table (which
    tests/test_contain_search_rule.py ties to is_hit), the order as one sort by (share, shared, index) with the share as a
    double.  That is exact below n_ref = 2^26: two different fractions with such denominators lie more than 2^-52 apart, so
    the correctly rounded quotients differ too and in the same direction, and equal fractions give the same double."""
    nq, nr = shared.shape
    assert int(n_ref.max()) < 2 ** 26
    hit = shared.astype(np.int64) >= np.asarray(need, np.int64)[n_ref]
    out = np.zeros((4, nq, top), np.uint32)
    n_hits = np.zeros(nq, np.uint32)
    for q in range(nq):
        idx = np.flatnonzero(hit[q])   # need[0] = 1: a hit has n_ref > 0
        c, b = shared[q, idx].astype(np.int64), n_ref[q, idx].astype(np.int64)
        best = idx[np.lexsort((idx, -c, -(c / b)))[:top]]
        n_hits[q] = best.size
        out[:, q, :best.size] = (best, shared[q, best], n_ref[q, best], n_qry[q, best])
    return out[0], out[1], out[2], out[3], n_hits


def search_text(ref_names, qry_names, qry_sizes, shared, n_qry, n_ref, k, top, min_identity=0.0, min_shared=1, max_p_value=1.0):
    """[(reference, query, identity, p, shared, n_ref, n_qry)] in print order (the tuples of contain_rule.rows_of_text)"""
    rows = []
    for q, hits in enumerate(search(shared, n_qry, n_ref, k, top, min_identity, min_shared)):
        for r, c, b, a in hits:
            p = cr.p_value(c, b, qry_sizes[q], k)
            if p <= max_p_value:
                rows.append((ref_names[r], qry_names[q], cr.identity(c, b, k), p, c, b, a))
    return rows

"""The case set of the reference-set search (mhx_dist_search), shared by the CPU emulation test and the GPU tests, and what
the oracle says about it: mo.compare of every (query, reference) pair, computed once per process; the expected lists are
those pairs put through tests/search_rule.py.

References: the 200 lists of triangle_cases.set200() -- seven slices, the last of 8 lists.  Queries: 150 lists, the ones
that matter first, so that queries()[:40] keeps them:
    0 .. 23   for each of the eight clade bases lists[3 + 23 c] a copy with 1 %, 10 % and 50 % of the hashes replaced
    24        a copy of list 5 (references 5, 190, 191 and 196 are identical: a four-way tie in that index order)
    25        a copy of list 141 (references 77 and 141 are duplicates)
    26        an empty list (against the empty reference 33 the oracle gives 0/0 and distance 0: its only hit at max_dist = 0)
    27        the first 17 hashes of list 10
    28 ..     independent lists
"""
import functools

import numpy as np

from oracle import mash_oracle as mo
from tests import search_rule as rule
from tests import triangle_cases as tc

K = 21
NQ = 150


def references():
    return tc.set200()


@functools.lru_cache(maxsize=None)
def queries():
    lists, s = tc.set200()
    rng = np.random.default_rng(150150)
    out = []
    for c in range(8):
        base = lists[3 + 23 * c]
        out += [tc.mutate(rng, base, drop) for drop in (0.01, 0.10, 0.50)]
    out += [lists[5].copy(), lists[141].copy(), np.zeros(0, np.uint64), lists[10][:17].copy()]
    out += [tc.sketch_like(rng, s) for _ in range(NQ - len(out))]
    return tuple(out)


def oracle_matrix(qs, rs, s, k):
    """(common, denom, dist) [nq, nr] of mo.compare(reference, query)"""
    common = np.zeros((len(qs), len(rs)), np.uint32)
    denom = np.zeros_like(common)
    dist = np.zeros(common.shape, np.float64)
    for i, q in enumerate(qs):
        for j, r in enumerate(rs):
            common[i, j], denom[i, j], dist[i, j] = mo.compare(r, q, s, k)
    return common, denom, dist


@functools.lru_cache(maxsize=None)
def matrix():
    refs, s = references()
    return oracle_matrix(queries(), refs, s, K)


def lists_from(common, denom, dist, top, max_dist):
    """the rule over a matrix of pairs: (ref, common, denom, dist [nq, top] zero-filled, n_hits [nq]) as the host form returns them"""
    nq, nr = common.shape
    out = [np.zeros((nq, top), np.uint32) for _ in range(3)] + [np.zeros((nq, top), np.float64), np.zeros(nq, np.uint32)]
    for q in range(nq):
        got = rule.select([(r, int(common[q, r]), int(denom[q, r]), float(dist[q, r])) for r in range(nr)], top, max_dist)
        out[4][q] = len(got)
        for t, hit in enumerate(got):
            for a in range(4):
                out[a][q, t] = hit[a]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(top, max_dist, nq=NQ, nr=200):
    """the rule's lists for queries()[:nq] against the first nr references"""
    common, denom, dist = matrix()
    return lists_from(common[:nq, :nr], denom[:nq, :nr], dist[:nq, :nr], top, max_dist)


def hits_per_query(max_dist, nq=NQ, nr=200):
    return (matrix()[2][:nq, :nr] <= max_dist).sum(axis=1)


@functools.lru_cache(maxsize=None)
def batch_boundary():
    """(references, [lists of query file 0, 1, 2]) at s = 16 for the file-level calls, which send their queries to the device in
    batches of 4096 sketches: 8 references and query files of 3000, 1200 and 50 random lists -- the first batch ends behind
    file 1, the last holds file 2 alone.  Every 47th query is a reference and every 41st a close copy of one, in all three files."""
    rng = np.random.default_rng(4250)
    refs = [tc.sketch_like(rng, 16) for _ in range(8)]
    files, i = [], 0
    for n in (3000, 1200, 50):
        lists = []
        for _ in range(n):
            lists.append(refs[i % 8].copy() if i % 47 == 0 else tc.mutate(rng, refs[i % 8], 0.25) if i % 41 == 0 else tc.sketch_like(rng, 16))
            i += 1
        files.append(lists)
    return refs, files

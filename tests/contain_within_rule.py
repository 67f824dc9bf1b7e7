"""The rule of the unbounded containment call (mhx_dist_contain_within, mhx_contain_files_within; `contain --all`) as a plain
statement in Python integers, built on the rule of the containment itself (tests/contain_rule.py) and on the hit test and the
order of the containment search (tests/contain_search_rule.py: is_hit, better), neither restated.  Shared by the tests of the
call; not a test module itself.  Nothing here is mash's: mash has no such command.

    hit        = contain_search_rule.is_hit(shared, n_ref, k, min_identity, min_shared), min_shared >= 1: min_identity <= 0
                 keeps every pair that shares at least min_shared hashes, min_identity > 1 none
    result     = row_off [nq + 1], row_off[0] = 0, and per hit (ref, shared, n_ref, n_qry); the hits of query q lie at
                 [row_off[q], row_off[q + 1]), ascending by reference index.  There is no cap.
    text       = for every query sketch, in argument order and then file order, one contain row per hit
                 "reference\\tquery\\tidentity\\tp\\tshared/n_ref\\tshared/n_qry\\n"; order `ref`: a query's hits in reference order,
                 order `best`: sorted by contain_search_rule.better; rows with p > max_p_value are dropped; a query without
                 hits prints nothing
"""
import numpy as np

from tests import contain_rule as cr
from tests import contain_search_rule as csr_rule


def hits_of(shared_row, n_ref_row, n_qry_row, k, min_identity=0.0, min_shared=1, memo=None):
    """[(ref, shared, n_ref, n_qry)] of one query, ascending by reference.  memo: decisions by (shared, n_ref), which are all
    a decision depends on at one bound"""
    assert min_shared >= 1
    memo = {} if memo is None else memo
    out = []
    for r in range(len(shared_row)):
        c, b = int(shared_row[r]), int(n_ref_row[r])
        if (c, b) not in memo:
            memo[(c, b)] = csr_rule.is_hit(c, b, k, min_identity, min_shared)
        if memo[(c, b)]:
            out.append((r, c, b, int(n_qry_row[r])))
    return out


def rows(shared, n_qry, n_ref, k, min_identity=0.0, min_shared=1):
    """the [nq, nr] matrices of contain_rule.matrix in, per query [(ref, shared, n_ref, n_qry)] in reference order"""
    memo = {}
    return [hits_of(shared[q], n_ref[q], n_qry[q], k, min_identity, min_shared, memo) for q in range(shared.shape[0])]


def arrays(per_query):
    """rows(..) as the call's outputs: (row_off uint64 [nq + 1], ref, shared, n_ref, n_qry uint32 [n_out])"""
    row_off = np.zeros(len(per_query) + 1, np.uint64)
    row_off[1:] = np.cumsum([len(h) for h in per_query], dtype=np.uint64)
    flat = [h for hits in per_query for h in hits]
    cols = np.array(flat, np.uint32).reshape(len(flat), 4)
    return row_off, cols[:, 0].copy(), cols[:, 1].copy(), cols[:, 2].copy(), cols[:, 3].copy()


def csr(shared, n_qry, n_ref, k, min_identity=0.0, min_shared=1):
    return arrays(rows(shared, n_qry, n_ref, k, min_identity, min_shared))


def rows_of_arrays(got):
    """the call's outputs back as per query [(ref, shared, n_ref, n_qry)]"""
    row_off = [int(v) for v in got[0]]
    return [list(zip(*(a[row_off[q]:row_off[q + 1]].tolist() for a in got[1:5]))) for q in range(len(row_off) - 1)]


def text_rows(ref_names, qry_names, qry_sizes, shared, n_qry, n_ref, k, min_identity=0.0, min_shared=1, max_p_value=1.0, order="best"):
    """[(reference, query, identity, p, shared, n_ref, n_qry)] in print order (the tuples of contain_rule.rows_of_text)"""
    assert order in ("best", "ref")
    out = []
    for q, hits in enumerate(rows(shared, n_qry, n_ref, k, min_identity, min_shared)):
        for r, c, b, a in (csr_rule.ranked(hits) if order == "best" else hits):
            p = cr.p_value(c, b, qry_sizes[q], k)
            if p <= max_p_value:
                out.append((ref_names[r], qry_names[q], cr.identity(c, b, k), p, c, b, a))
    return out

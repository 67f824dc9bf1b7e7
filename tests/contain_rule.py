"""The rule of the containment from sketches (mhx_dist_contain, mhx_contain_files) as a plain statement in Python integers.
Shared by the containment tests; not a test module itself.  Nothing here is mash's: mash has no such command.

    list        = the first min(len, stride, s) entries of a row: ascending, duplicate-free u64; s is the sketch size of ITS
                  set (s_q or s_r, >= 1)
    full        = it holds s entries
    bound(list) = its last entry if full, else 2^64 - 1   (a list shorter than s holds every hash of its input; the empty one too)
    tau         = min(bound(query), bound(reference))
    n_qry       = #{x in query:     x <= tau}
    n_ref       = #{x in reference: x <= tau}
    shared      = #{x in both:      x <= tau}              (tau is inclusive; 2^64 - 1 is a legitimate hash)

    identity    = 1 if shared == n_ref > 0, 0 if shared == 0 (also when n_ref == 0), else (shared / n_ref) ** (1 / k)
    p           = 1 if n_ref == 0, else the screen's p-value of (shared, n_ref) at the set size of the QUERY sketch
    row         = reference <TAB> query <TAB> identity <TAB> p <TAB> shared/n_ref <TAB> shared/n_qry     (%g)
"""
import bisect

import numpy as np

from tests import screen_rule as sr

FULL = 2 ** 64 - 1


def the_list(row, length, s, stride=None):
    """the list of a row as Python integers"""
    row = [int(x) for x in row]
    n = min(int(length), len(row) if stride is None else int(stride), int(s))
    return row[:n]


def bound(lst, s):
    return lst[-1] if len(lst) == s else FULL


def counts(q, r, s_q, s_r):
    """(shared, n_qry, n_ref) of two lists (the_list)"""
    tau = min(bound(q, s_q), bound(r, s_r))
    n_qry, n_ref = bisect.bisect_right(q, tau), bisect.bisect_right(r, tau)
    shared = len(set(q[:n_qry]).intersection(r[:n_ref]))
    return shared, n_qry, n_ref


def matrix(qs, rs, s_q, s_r):
    """(shared, n_qry, n_ref) [nq, nr] over lists given as arrays, each cut at its set's sketch size"""
    ql = [the_list(v, len(v), s_q) for v in qs]
    rl = [the_list(v, len(v), s_r) for v in rs]
    out = np.zeros((3, len(ql), len(rl)), np.uint32)
    for i, q in enumerate(ql):
        for j, r in enumerate(rl):
            out[:, i, j] = counts(q, r, s_q, s_r)
    return out[0], out[1], out[2]


def matrix_of_rows(Q, q_len, R, r_len, s_q, s_r):
    """the same over row matrices with lengths (what the device calls take)"""
    ql = [the_list(Q[i], q_len[i], s_q) for i in range(len(q_len))]
    rl = [the_list(R[j], r_len[j], s_r) for j in range(len(r_len))]
    out = np.zeros((3, len(ql), len(rl)), np.uint32)
    for i, q in enumerate(ql):
        for j, r in enumerate(rl):
            out[:, i, j] = counts(q, r, s_q, s_r)
    return out[0], out[1], out[2]


def identity(shared, n_ref, k):
    return 0.0 if shared == 0 else sr.identity(shared, n_ref, k)


def p_value(shared, n_ref, set_size, k):
    return 1.0 if n_ref == 0 else sr.p_value(shared, n_ref, set_size, k)


def expected_rows(ref_names, qry_names, qry_sizes, shared, n_qry, n_ref, k, min_identity=0.0, max_p_value=1.0):
    """[(reference, query, identity, p, shared, n_ref, n_qry)] in print order, the dropped rows left out"""
    rows = []
    for i, qn in enumerate(qry_names):
        for j, rn in enumerate(ref_names):
            c, a, b = int(shared[i, j]), int(n_qry[i, j]), int(n_ref[i, j])
            ident, p = identity(c, b, k), p_value(c, b, qry_sizes[i], k)
            if ident >= min_identity and p <= max_p_value:
                rows.append((rn, qn, ident, p, c, b, a))
    return rows


def rows_of_text(text):
    """[(reference, query, identity, p, shared, n_ref, n_qry)] of the printed rows; the two fractions must agree on `shared`"""
    rows = []
    for line in text.splitlines():
        rn, qn, ident, p, of_ref, of_qry = line.split("\t")
        c, b = of_ref.split("/")
        c2, a = of_qry.split("/")
        assert c == c2, line
        rows.append((rn, qn, float(ident), float(p), int(c), int(b), int(a)))
    return rows


def same_rows(got, want):
    """names and integers exact, identity and p to the sixth digit (the resolution of a %g column)"""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if (g[0], g[1], g[4], g[5], g[6]) != (w[0], w[1], w[4], w[5], w[6]):
            return False
        for x, y in ((g[2], w[2]), (g[3], w[3])):
            if not (x == y or sr.same_to_the_sixth_digit(x, y)):
                return False
    return True

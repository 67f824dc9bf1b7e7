"""The case sets of the winner-take-all containment (mhx_dist_contain_winner), shared by the rule test, the CPU emulation
test and the GPU tests, and what the rule (tests/contain_winner_rule.py) says about each, computed once per process.  Not a
test module itself.

    tau_and_ties   1 x 5 at s_q = 16, s_r = 8 in small integers, see tau_and_ties_rows(); run without and with genome lengths
    crafted        contain_cases.crafted_rows()
    clades         7 x 14 at s_q = 1000, s_r = 200: three base genomes of 20 000 hashes, each with 0.2 %, 1 % and 5 % mutated copies
                   (references 4 c + 0 .. 4 c + 3 are clade c, the base first), a 40-hash short reference cut from base 0 and an
                   unrelated genome; queries: the three bases, the union of base 0 and base 2 (a mixed culture), the 0.2 % copy
                   of base 0, the first 17 hashes of base 0, an unrelated genome
    and small, mixed, plasmids, plasmids_swapped, crowded, extreme, extreme_mirrored, long_pair of contain_cases
"""
import functools

import numpy as np

from tests import contain_cases as cc
from tests import contain_winner_rule as wrule
from tests import triangle_cases as tc

TAU_LENGTHS = (5, 5, 9, 5, 5)
CLADE_SHORT_REF, CLADE_MIXED_QUERY, CLADE_COPY_QUERY, CLADE_SHORT_QUERY = 12, 3, 4, 5


def tau_and_ties_rows():
    """(Q, q_len, R, r_len, s_q, s_r) at stride 16.  The query is 10, 20 .. 160.
        A  10 .. 80 full, with 90, 100 behind a length above the sketch size: it holds them only behind its bound
        B  [70 80 90 100 105 999], a short list: tau = 160, it finds 70 .. 100 and wins 90 and 100
        C  a copy of A: ties with A, the genome length or the lower index decides
        D  [5 10 15 20 25 30 33 35] full: tau = 35
        E  [155 160]: tau = 160 is inclusive, it wins 160"""
    s_q, s_r, stride = 16, 8, 16
    A = list(range(10, 110, 10))
    refs = [A, [70, 80, 90, 100, 105, 999], list(A), [5, 10, 15, 20, 25, 30, 33, 35], [155, 160]]
    R, r_len = tc.pad_rows([np.array(v, np.uint64) for v in refs], stride)
    Q, q_len = tc.pad_rows([np.arange(10, 170, 10, dtype=np.uint64)], stride)
    assert r_len[0] > s_r
    return Q, q_len, R, r_len, s_q, s_r


@functools.lru_cache(maxsize=None)
def clades():
    rng = np.random.default_rng(7)
    bases = [cc.genome(rng, 20000) for _ in range(3)]
    refs = []
    for b in bases:
        refs += [b] + [tc.mutate(rng, b, d) for d in (0.002, 0.01, 0.05)]
    refs += [bases[0][:40], cc.genome(rng, 20000)]
    # the 17-hash query: the first window of 17 among base 0's lowest 40 hashes that exactly three clade members hold whole
    holds = lambda w: sum(int(np.isin(w, refs[j][:200]).all()) for j in range(4))
    short = next(bases[0][a:a + 17] for a in range(24) if holds(bases[0][a:a + 17]) == 3)
    qrys = list(bases) + [cc.union(bases[0], bases[2]), refs[1], short, cc.genome(rng, 20000)]
    assert len(qrys) == 7 and len(refs) == 14
    return tuple(qrys), tuple(refs), 1000, 200


def clade_lengths():
    """distinct genome lengths for the file-level test: they fall with the index, so every tie goes where the index sends it"""
    return [5_000_000 - 1000 * j for j in range(14)]


REUSED = ("small", "mixed", "plasmids", "plasmids_swapped", "crowded", "extreme", "extreme_mirrored", "long_pair")
NAMES = ("tau_and_ties", "tau_and_ties_lengths", "crafted", "clades") + REUSED


def rows_of(name):
    """(Q, q_len, R, r_len, s_q, s_r, ref_length or None): the case as the row matrices a device call takes"""
    if name == "tau_and_ties":
        return tau_and_ties_rows() + (None,)
    if name == "tau_and_ties_lengths":
        return tau_and_ties_rows() + (np.array(TAU_LENGTHS, np.uint64),)
    if name == "crafted":
        return cc.crafted_rows() + (None,)
    if name == "clades":
        qs, rs, s_q, s_r = clades()
        qs, rs = tuple(v[:s_q + 3] for v in qs), tuple(v[:s_r + 3] for v in rs)
        Q, q_len = tc.pad_rows(list(qs), 1008)
        R, r_len = tc.pad_rows(list(rs), 1008)
        return Q, q_len, R, r_len, s_q, s_r, None
    return cc.rows_of(name) + (None,)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(won, shared, n_qry, n_ref [nq, nr], distinct [nq], winners) by the rule"""
    Q, q_len, R, r_len, s_q, s_r, lengths = rows_of(name)
    return wrule.matrix_of_rows(Q, q_len, R, r_len, s_q, s_r, lengths)

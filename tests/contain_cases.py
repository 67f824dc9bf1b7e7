"""The case sets of the containment from sketches (mhx_dist_contain), shared by the rule test, the CPU emulation test and the
GPU tests, and what the rule (tests/contain_rule.py) says about each, computed once per process.  A "genome" is a set of
20 000 to 240 000 random hashes, a sketch its s smallest.  Not a test module itself.

A case is (queries, references, s_q, s_r): tuples of ascending uint64 arrays that may be LONGER than their set's sketch size
(the list is what the rule cuts out of them).

    crafted     6 x 5 at s_q = 16, s_r = 8 in small integers: the pair kernel's edge cases, see crafted_rows()
    small       12 x 9 at s_q = 200, s_r = 100: 16 value ranges
    mixed       40 x 33 at s_q = 1000, s_r = 200: 64 value ranges, two reference slices, the second of one list
    set200      search_cases.queries() x triangle_cases.set200() at s = 1000 both
    extreme, extreme_mirrored   extreme_cases.batch(40): 2^64 - 1 next to a value of the same home slot, short lists whose tau is 2^64 - 1
    crowded     triangle_cases.crowded(40) against itself: nearly everything in one value range (flagged blocks)
    plasmids, plasmids_swapped   short lists over the whole hash space against full lists of 240 000-hash genomes (flagged blocks)
    long_pair   one pair of 70 000 entries: no geometry of the base form
"""
import functools

import numpy as np

from tests import contain_rule as rule
from tests import extreme_cases as xc
from tests import search_cases as sc
from tests import triangle_cases as tc

K = 21
FULL = np.uint64(2 ** 64 - 1)


def genome(rng, n):
    return tc.sketch_like(rng, n)


def union(*parts):
    return np.unique(np.concatenate(parts))


def crafted_rows():
    """(Q, q_len, R, r_len, s_q, s_r) at stride 24, rows with padding behind len -- 2^64 - 1 as the segmented sketch leaves it,
    zeros, or further ascending values behind a len above the sketch size (which a reference shares: they must not count).
        references  0 empty | 1 short [10 20 30] | 2 full, bound 40, len 10 | 3 full, ends in 2^64 - 1 | 4 short, ends in 2^64 - 1
        queries     0 empty | 1 short, identical to reference 1 | 2 full 5 .. 80, len 20 | 3 full, disjoint from everything
                    4 full 2 .. 32 | 5 full, ends in 2^64 - 1
    query 2 x reference 2: tau = 40, a value both hold; query 4 x reference 2: tau = 32, which the query alone holds, strictly
    between 30 and 35 of the reference; query 1 x reference 4 and 1 x 1: two short lists, tau = 2^64 - 1; 5 x 3 and 5 x 4 share
    2^64 - 1 itself."""
    s_q, s_r, stride = 16, 8, 24
    full = int(FULL)
    refs = [([], full), ([10, 20, 30], full), ([5, 10, 15, 20, 25, 30, 35, 40, 45, 50], 0), ([1, 2, 3, 4, 5, 6, 7, full], 0), ([20, 40, full], 0)]
    qrys = [([], full), ([10, 20, 30], full), (list(range(5, 105, 5)), full), (list(range(1001, 1017)), 0), (list(range(2, 34, 2)), full),
            (list(range(3, 48, 3)) + [full], full)]

    def pack(lists):
        M = np.zeros((len(lists), stride), np.uint64)
        for i, (v, fill) in enumerate(lists):
            M[i, :] = np.uint64(fill)
            M[i, :len(v)] = np.array(v, np.uint64)
        return M, np.array([len(v) for v, _ in lists], np.uint32)

    Q, q_len = pack(qrys)
    R, r_len = pack(refs)
    assert q_len[2] > s_q and r_len[2] > s_r
    return Q, q_len, R, r_len, s_q, s_r


@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(16016)
    G = [genome(rng, 20000) for _ in range(9)]
    refs = list(G)
    refs[4] = G[4][:40]                      # a short list: a 40-hash input
    refs[6] = np.zeros(0, np.uint64)
    qrys = [union(G[i], genome(rng, 5000)) for i in range(4)]            # supersets
    qrys += [tc.mutate(rng, G[i], 0.02 * (i + 1)) for i in range(4)]     # close copies
    qrys += [genome(rng, 20000), np.zeros(0, np.uint64), G[2][:23], union(G[7], G[8])]
    return tuple(qrys), tuple(refs), 200, 100


@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(4033)
    G = [genome(rng, 20000) for _ in range(33)]
    refs = list(G)
    refs[7] = G[7][:50]
    refs[9] = np.zeros(0, np.uint64)
    qrys = [union(G[i], genome(rng, 20000 * (1 + i % 3))) for i in range(10)]          # the reference plus a contaminant
    qrys += [tc.mutate(rng, G[i], (0.01, 0.05, 0.2)[i % 3]) for i in range(10, 20)]
    qrys[12] = union(G[32], genome(rng, 30000))                                        # the lone reference of the second slice
    qrys += [genome(rng, 20000 + 4000 * i) for i in range(10)]
    qrys += [np.zeros(0, np.uint64), G[3][:17], G[5][:700]]
    qrys += [union(G[2 * i], G[2 * i + 1]) for i in range(7)]                           # mixed cultures
    assert len(qrys) == 40
    return tuple(qrys), tuple(refs), 1000, 200


def set200():
    refs, s = tc.set200()
    return sc.queries(), refs, s, s


def extreme():
    q, r, s = xc.batch(40)
    return q, r, s, s


def extreme_mirrored():
    q, r, s = xc.batch(40, True)
    return q, r, s, s


def crowded():
    lists, s = tc.crowded(40)
    return lists, lists, s, s


@functools.lru_cache(maxsize=None)
def plasmids():
    """queries: full lists of 240 000-hash genomes; references: eight short lists (30 .. 300 hashes over the whole hash space,
    three of them inside a query's genome) and two full lists"""
    rng = np.random.default_rng(240000)
    P = [genome(rng, 30 + 38 * i) for i in range(8)]
    G = [genome(rng, 240000) for _ in range(8)]
    G[0], G[1], G[5] = union(G[0], P[0]), union(G[1], P[3], P[4]), union(G[5], P[3])
    return tuple(G), tuple(P) + (G[2], tc.mutate(rng, G[3], 0.03)), 1000, 1000


def plasmids_swapped():
    q, r, s_q, s_r = plasmids()
    return r, q, s_r, s_q


@functools.lru_cache(maxsize=None)
def long_pair():
    rng = np.random.default_rng(70000)
    g = genome(rng, 100000)
    return (tc.mutate(rng, g, 0.1),), (g,), 70000, 70000


@functools.lru_cache(maxsize=None)
def two_groups():
    """140 x 960 lists of 64 hashes at s = 64 both (30 slices, 16 value ranges): with one query per block that is 4200 blocks,
    the last 104 -- query 136 from slice 16 on and queries 137 to 139 -- in a second group of flag words.  The references are
    close copies of 30 bases and independent lists; queries 136 to 139 derive from references of slices 21, 28 and 29, so that
    blocks of the second group hold counts that are not zero.  Not in NAMES: only the GPU test of the group boundary runs it."""
    rng = np.random.default_rng(4200)
    s, nq, nr = 64, 140, 960
    bases = [tc.sketch_like(rng, s) for _ in range(30)]
    refs = [tc.mutate(rng, bases[j % 30], 0.02 * (j % 11)) if j % 3 else tc.sketch_like(rng, s) for j in range(nr)]
    qrys = [tc.mutate(rng, refs[(7 * i) % nr], 0.03 * (i % 9)) for i in range(nq)]
    qrys[136], qrys[137], qrys[138], qrys[139] = refs[700][::2].copy(), refs[900].copy(), refs[930][5:].copy(), tc.mutate(rng, refs[959], 0.1)
    return tuple(qrys), tuple(refs), s, s


NAMES = ("small", "mixed", "set200", "extreme", "extreme_mirrored", "crowded", "plasmids", "plasmids_swapped", "long_pair")


def case(name):
    return globals()[name]()


def rows_of(name, stride=None):
    """the case as the row matrices a device call takes (zero behind a list's end; a list longer than its sketch size keeps
    three entries too many, which the call has to cut)"""
    qs, rs, s_q, s_r = case(name)
    qs, rs = tuple(v[:s_q + 3] for v in qs), tuple(v[:s_r + 3] for v in rs)
    if stride is None:
        stride = (max(max(map(len, qs + rs)), 1) + 15) // 16 * 16
    Q, q_len = tc.pad_rows(list(qs), stride)
    R, r_len = tc.pad_rows(list(rs), stride)
    return Q, q_len, R, r_len, s_q, s_r


@functools.lru_cache(maxsize=None)
def expected(name):
    """(shared, n_qry, n_ref) [nq, nr] by the rule"""
    if name == "crafted":
        return rule.matrix_of_rows(*crafted_rows())
    return rule.matrix(*case(name))

"""The case of the containment search (mhx_dist_contain_search) that tests/contain_cases.py does not hold: ties.  Shared by the
emulation test and the GPU tests; not a test module itself.

    ties    6 queries at s_q = 1000 against 70 references at s_r = 200 (three slices: 32, 32 and 6).  References 3, 35 and 67
            are the same list -- a tie across all three slices, which only the index breaks; reference 10 is a short list
            (the 50 hashes of a 50-hash input), so a query that holds it whole has 50/50 next to the 200/200 of a full
            reference it holds: equal share, different `shared`.
            queries  0  genomes 3, 10, 11 and a contaminant: 200/200 for 3, 11, 35, 67 (by index), then 50/50
                     1  genome 3 and a contaminant twice its size
                     2  a 5 % mutant of genome 3: the same share below 1 three times
                     3  unrelated: no hits (or as good as none)
                     4  the empty list: n_qry = 0, nothing shared
                     5  genomes 20, 40 and 66, one in every slice
"""
import functools

import numpy as np

from tests import contain_cases as cc
from tests import contain_rule as rule
from tests import triangle_cases as tc

K = cc.K


@functools.lru_cache(maxsize=None)
def ties():
    rng = np.random.default_rng(70367)
    G = [cc.genome(rng, 20000) for _ in range(70)]
    refs = list(G)
    refs[35] = refs[67] = G[3]
    refs[10] = G[10][:50]
    qrys = [cc.union(G[3], G[10][:50], G[11], cc.genome(rng, 20000)), cc.union(G[3], cc.genome(rng, 40000)), tc.mutate(rng, G[3], 0.05),
            cc.genome(rng, 20000), np.zeros(0, np.uint64), cc.union(G[20], G[40], G[66])]
    return tuple(qrys), tuple(refs), 1000, 200


def rows():
    """the case as the row matrices a device call takes (as contain_cases.rows_of)"""
    qs, rs, s_q, s_r = ties()
    qs, rs = tuple(v[:s_q + 3] for v in qs), tuple(v[:s_r + 3] for v in rs)
    stride = (max(max(map(len, qs + rs)), 1) + 15) // 16 * 16
    Q, q_len = tc.pad_rows(list(qs), stride)
    R, r_len = tc.pad_rows(list(rs), stride)
    return Q, q_len, R, r_len, s_q, s_r


@functools.lru_cache(maxsize=None)
def expected():
    """(shared, n_qry, n_ref) [6, 70] by the rule of the containment"""
    return rule.matrix(*ties())


@functools.lru_cache(maxsize=None)
def many_blocks():
    """8 queries x 16 640 references of 16-hash lists at s = 16 both: with one query per block that is 8 x 520 = 4160 blocks,
    64 more than the group of 4096 whose flag words come back together.  The values are small integers, so that lists share
    hashes by chance: (Q, q_len, R, r_len, s, s) as row matrices at stride 16, every list full."""
    rng = np.random.default_rng(4160)
    nq, nr, s = 8, 16640, 16

    def lists(n):
        M = np.sort(rng.integers(1, 400, size=(n, 3 * s), dtype=np.uint64), axis=1)
        out = np.zeros((n, s), np.uint64)
        for i in range(n):
            out[i] = np.unique(M[i])[:s]   # (48 draws of 399 values: far more than 16 distinct ones)
        return out

    Q, R = lists(nq), lists(nr)
    R[16000:16008] = Q    # the last 20 slices lie behind block 4096 for the last query only: plant every query's own list there
    return Q, np.full(nq, s, np.uint32), R, np.full(nr, s, np.uint32), s, s


@functools.lru_cache(maxsize=None)
def flagged_groups():
    """150 queries x 900 references (29 slices) at s = 64 both (16 ranges): with one query per block that is 4350 blocks, the
    last 254 in a second group of flag words.  Slice 27 holds 32 lists crowded into one value range -- 2048 keys for a range
    table of 1536 --, so exactly one block per query raises its flag, in both groups, and is redone by the pair kernel; a
    flag word left standing from the first group would show as one fallback more.  Queries 145 and 147, of the second group,
    derive from references of that slice: their best hits are what the pair kernel computed there.
    (queries, references, s, s) as lists (the construction of the search's test of the same name)"""
    rng = np.random.default_rng(4350)
    s, nq, nr = 64, 150, 900
    bases = [tc.sketch_like(rng, s) for _ in range(30)]
    refs = [tc.mutate(rng, bases[j % 30], 0.02 * (j % 11)) if j % 3 else tc.sketch_like(rng, s) for j in range(nr)]
    for j in range(27 * 32, 28 * 32):
        refs[j] = np.uint64(1 << 62) + tc.sketch_like(rng, s, hi=2 ** 20)
    qrys = [tc.mutate(rng, refs[(7 * i) % nr], 0.03 * (i % 9)) for i in range(nq)]
    qrys[145], qrys[147], qrys[3] = refs[870].copy(), refs[880][5:].copy(), refs[866][::2].copy()
    assert 145 * 29 + 27 >= 4096 and len(np.unique(np.concatenate(refs[27 * 32:28 * 32]))) > 1536
    return tuple(qrys), tuple(refs), s, s


@functools.lru_cache(maxsize=None)
def flagged_groups_expected():
    return rule.matrix(*flagged_groups())


@functools.lru_cache(maxsize=None)
def many_blocks_expected():
    """(shared, n_qry, n_ref) [8, 16640] by the rule of the containment, vectorised: both lists are full, so tau is the smaller
    of the two last entries and the counts are prefix sizes and an intersection size below it (checked against
    contain_rule.counts on a sample of the pairs)"""
    Q, q_len, R, r_len, s, _ = many_blocks()
    nq, nr = len(q_len), len(r_len)
    tau = np.minimum(Q[:, None, -1], R[None, :, -1])                     # [nq, nr]
    n_qry = (Q[:, None, :] <= tau[:, :, None]).sum(axis=2)
    n_ref = (R[None, :, :] <= tau[:, :, None]).sum(axis=2)
    shared = np.zeros((nq, nr), np.int64)
    for j in range(s):   # every query entry: is it in the reference, and at or below tau
        v = Q[:, None, j:j + 1]
        shared += ((R[None, :, :] == v).any(axis=2) & (v[:, :, 0] <= tau))
    out = shared.astype(np.uint32), n_qry.astype(np.uint32), n_ref.astype(np.uint32)
    for q, r in ((0, 0), (3, 77), (7, 16639), (5, 16005), (2, 4095), (6, 9999)):
        want = rule.counts([int(x) for x in Q[q]], [int(x) for x in R[r]], s, s)
        assert (int(out[0][q, r]), int(out[1][q, r]), int(out[2][q, r])) == want, (q, r)
    return out

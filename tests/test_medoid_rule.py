"""The rule of the medoids (tests/medoid_rule.py) on its own, on the CPU: a hand-written example with its sums written out,
what the existing case sets hold for the feature and its tie rule, the pick key at its limits, and the new entry points in
the header and in the binding."""
import numpy as np
import pytest

from auriclass_amd import engine
from tests import cluster_cases as cc
from tests import linkage_rule as lr
from tests import medoid_rule as mr
from tests import triangle_cases as tc

K = cc.K


def test_five_lists_by_hand():
    """s = 8, one cluster of five.  Shared values of the ten pairs (denom 8 each): list 2 shares 4 with everybody; 0-1, 0-3 and
    1-4 share 2; 0-4 and 3-4 share 3; 1-3 share nothing.  q(4/8) = 82 926 637, q(3/8) = 123 968 259, q(2/8) = 187 401 844 and
    q(0) = 2^32 in units of 2^-32 at k = 21, so
        sum[0] = q2 + q4 + q2 + q3, sum[1] = q2 + q4 + 2^32 + q2, sum[2] = 4 q4, sum[3] = q2 + 2^32 + q4 + q3, sum[4] = q3 + q2 + q4 + q3
    and the medoid is list 2: neither the first member nor the longest one (list 4, 11 hashes)."""
    lists = [np.array(x, np.uint64) for x in ([10, 20, 30, 40, 55, 65, 75, 85], [10, 20, 35, 45, 50, 60, 75, 85], [10, 20, 30, 40, 50, 60, 70, 80],
                                              [15, 25, 30, 40, 50, 60, 70, 85], [10, 22, 30, 40, 50, 62, 70, 80, 90, 95, 99])]
    s = 8
    pairs = tc.oracle_pairs(lists, s, K)
    assert pairs[0].tolist() == [2, 4, 4, 2, 0, 4, 3, 2, 4, 3] and pairs[1].tolist() == [8] * 10
    q4, q3, q2, one = (lr.fixed_distance(c, 8, K) for c in (4, 3, 2, 0))
    assert (q4, q3, q2, one) == (82926637, 123968259, 187401844, 1 << 32)
    medoid, total, common, denom = mr.medoids_of(lists, s, K, [0] * 5, pairs)
    assert total == [2 * q2 + q4 + q3, 2 * q2 + q4 + one, 4 * q4, q2 + one + q4 + q3, 2 * q3 + q2 + q4]
    assert total == [581698584, 4752697621, 331706548, 4689264036, 518264999]
    assert medoid == [2] * 5 and max(range(5), key=lambda i: len(lists[i])) == 4
    assert (common, denom) == ([4, 4, 8, 4, 4], [8] * 5)   # the pair (2, 2) goes through the rule: 8 / 8
    # the same lists as two clusters and a singleton: {0, 1, 4}, {2}, {3}
    label = [0, 0, 2, 3, 0]
    total = mr.sums(mr.pair_table(pairs[0], pairs[1], 5, K), label)
    assert total == [q2 + q3, q2 + q2, 0, 0, q3 + q2] and mr.medoids(total, label) == [0, 0, 2, 3, 0]   # 0 and 4 tie: the lower index
    assert not mr.valid([0, 2, 2, 3, 0]) and not mr.valid([0, 0, 1, 3, 0]) and not mr.valid([1, 1, 2, 3, 4]) and mr.valid(label)


def _clusters(name, bound):
    lists, s = getattr(cc, name)()
    label = [int(l) for l in cc.expected(name, bound)[0]]
    medoid, total, _, _ = mr.medoids_of(lists, s, K, label, cc.pairs(name))
    out = []
    for root in [i for i, l in enumerate(label) if l == i]:
        members = [i for i, l in enumerate(label) if l == root]
        if len(members) > 1:
            best = sorted(total[i] for i in members)
            out.append((root, medoid[root], best[0] == best[1]))
    return out


def test_the_case_sets_exercise_the_feature_and_its_tie_rule():
    chains = _clusters("chains", cc.CHAINS_BOUND)
    assert len(chains) == 3 and all(medoid != root for root, medoid, _ in chains)   # no medoid is its cluster's first member
    set70 = _clusters("set70", 0.02)
    assert sum(tie for _, _, tie in set70) == 1                                      # one cluster whose two best members tie
    set200 = _clusters("set200", 0.05)
    assert len(set200) == 9 and sum(tie for _, _, tie in set200) == 3


def test_the_key_at_its_limits():
    top = 65535 << 32
    assert mr.MAX_SUM == top
    word = mr.key(top, 65535)
    assert word == (1 << 64) - (1 << 48) + 65535 and word < (1 << 64) - 1 and mr.unkey(word) == (top, 65535)
    assert mr.key(0, 0) == 0 and mr.unkey(0) == (0, 0)
    assert mr.key(5, 9) < mr.key(6, 0) and mr.key(5, 3) < mr.key(5, 9)   # the sum first, then the index


def test_the_entry_points_are_declared_and_bound():
    declared = engine.declared_symbols()
    for name in ("mhx_dist_medoids", "mhx_dist_to", "mhx_last_medoid_blocks", "mhx_cluster_reps_files"):
        assert name in declared
    engine.build()
    lib = engine.load()
    assert len(lib.mhx_dist_medoids.argtypes) == 12 and len(lib.mhx_dist_to.argtypes) == 10 and len(lib.mhx_cluster_reps_files.argtypes) == 7
    import ctypes
    assert ctypes.sizeof(engine.ClusterRepsOpts) == 24
    assert engine.CLUSTER_REPS == {"first": 0, "longest": 1}   # the old calls keep their two kinds
    with pytest.raises(ValueError):
        engine.cluster_reps_files([], 0.05, rep="shortest")
    with pytest.raises(ValueError):
        engine.cluster_reps_files([], 0.05, linkage="ward")

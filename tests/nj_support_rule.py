"""The rule of the jackknife support of the neighbour-joining tree (mhx_dist_nj_support, mhx_nj_split_support,
mhx_nj_files_opts) as a plain statement, plain and slow, over Python sets and integers.  Shared by the support tests; not a
test module itself.

    leaf sets   = the leaf set of the node made by join t is the union of the leaf sets of its two ids (an id that no join has
                  made yet stands for its leaf alone)
    canon       = canon(X) = X if leaf 0 is not in X, else its complement
    splits      = of a tree: canon of the leaf sets of all its n - 1 joins
    support     = support[t] of the main tree (the unresampled records of nj_rule) = the number of replicates whose split set
                  holds canon(leaf set of join t); a split with 0, 1, n - 1 or n leaves on a side counts as present in every
                  tree and gets R.  All of it integers
    replicates  = replicate r is resample_rule.replicate of the lists; its tree nj_rule.records_of over the oracle's triangle of
                  the cut lists at sketch size s_r, the same k
    table       = nj_rule's row and a seventh column "c/R"
    newick      = nj_rule's text; the node of every join t <= n - 4 (the inner nodes but the root) carries floor(100 c / R)
                  between ")" and ":".  The trifurcation carries none: the split of join n - 3 is the complement of its third
                  child's, and the two counts agree (asserted here)
"""
import functools

import numpy as np

from tests import nj_cases as nc
from tests import nj_rule as nr
from tests import resample_rule as rr
from tests import triangle_cases as tc


def leaf_sets(joins, n):
    """the leaf set of the node of every join, [(a, b)] in join order"""
    of = {i: frozenset([i]) for i in range(n)}
    out = []
    for a, b in joins:
        of[b] = of[b] | of.pop(a)
        out.append(of[b])
    return out


def canon(X, n):
    return X if 0 not in X else frozenset(range(n)) - X


def trivial(X, n):
    return len(X) in (0, 1, n - 1, n)


def splits(joins, n):
    return {canon(X, n) for X in leaf_sets(joins, n)}


def support(main, reps, n):
    """support[t] of the joins `main` among the replicate trees `reps` (each [(a, b)])"""
    theirs = [splits(joins, n) for joins in reps]
    return [len(reps) if trivial(X, n) else sum(canon(X, n) in S for S in theirs) for X in leaf_sets(main, n)]


def joins_of(records):
    return [(r[0], r[1]) for r in records]


def replicate_trees(lists, s, k, replicates, keep, seed):
    """[(joins, s_r)] of the replicates 0 .. R - 1"""
    out = []
    for r in range(replicates):
        cut, s_r = rr.replicate(lists, s, seed, r, keep)
        common, denom, _ = tc.oracle_pairs(cut, s_r, k)
        out.append((joins_of(nr.records_of(common, denom, len(lists), k)[0]), s_r))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, args, replicates, keep, seed, k=nc.K):
    """(support, rep_join_a, rep_join_b [R, n - 1], rep_s [R]) of a case set of tests/nj_cases.py"""
    lists, s = nc.lists_of(name, args)
    n = len(lists)
    trees = replicate_trees(lists, s, k, replicates, keep, seed)
    main = joins_of(nc.expected(name, args, k)[0])
    sup = support(main, [t[0] for t in trees], n)
    rep_a = np.array([[a for a, _ in t[0]] for t in trees], np.uint32).reshape(replicates, n - 1)
    rep_b = np.array([[b for _, b in t[0]] for t in trees], np.uint32).reshape(replicates, n - 1)
    return np.array(sup, np.uint32), rep_a, rep_b, np.array([t[1] for t in trees], np.uint32)


# ---- text ---------------------------------------------------------------------------------------------------------------------
def newick(names, records, sup, replicates):
    """nj_rule.newick with the labels of the inner nodes but the root"""
    from tests import tree_rule as tl

    n = len(names)
    if n <= 3:
        return nr.newick(names, records)       # no inner node but the root
    la, lb = nr.all_lengths(records)
    branch = lambda x: "%g" % max(0.0, float(x))   # noqa: E731
    text = {i: tl.quoted(names[i]) for i in range(n)}
    made = {}                                   # the join that made the node of an id
    for t in range(n - 3):
        a, b = records[t][:2]
        text[b] = "(%s:%s,%s:%s)%d" % (text[b], branch(lb[t]), text.pop(a), branch(la[t]), 100 * sup[t] // replicates)
        made[b] = t
        made.pop(a, None)
    a, b = records[n - 3][:2]
    other = [i for i in records[n - 2][:2] if i != b]
    assert len(other) == 1 and sorted(text) == sorted([a, b, other[0]])
    # the split of join n - 3 is the complement of the third child's: one count, and the third child carries it
    assert sup[n - 3] == (sup[made[other[0]]] if other[0] in made else replicates)
    kids = sorted([(b, lb[n - 3]), (a, la[n - 3]), (other[0], records[n - 2][2] * nr.SCALE)])
    return "(" + ",".join("%s:%s" % (text[i], branch(x)) for i, x in kids) + ");\n"


def file_support(F, replicates, keep, seed):
    """(records, support) of a SketchFile (oracle.mash_oracle)"""
    lists = [np.asarray(r.hashes, np.uint64) for r in F.references]
    records = nr.records_of_file(F)
    trees = replicate_trees(lists, F.sketch_size, F.kmer_size, replicates, keep, seed)
    return records, support(joins_of(records), [t[0] for t in trees], len(lists))


def table_text(F, replicates, keep, seed, comment=False):
    _, sup = file_support(F, replicates, keep, seed)
    rows = nr.table_text(F, comment).splitlines()
    assert len(rows) == len(sup)
    return "".join("%s\t%d/%d\n" % (row, c, replicates) for row, c in zip(rows, sup))


def newick_text(F, replicates, keep, seed, comment=False):
    records, sup = file_support(F, replicates, keep, seed)
    return newick([(r.comment if comment else r.name) for r in F.references], records, sup, replicates)

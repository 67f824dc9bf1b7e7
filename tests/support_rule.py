"""The rule of the jackknife support of search hits (mhx_dist_support, mhx_search_files_support; auriclass_amd/csrc/
mhx_support.h) as a plain statement in Python integers, built from the rules that are stated already: the jackknife
(tests/resample_rule.py), the mash-pinned pair rule (mo.compare) and the order of the search (tests/search_rule.py).  Shared by
the support tests; not a test module itself.

    inputs      = a query list Q, candidate reference lists C_0 .. C_{m-1} (m <= 64) with their reference indices, sketch size s,
                  k, `replicates` = R, keep, seed
    replicate r = (lists_r, s_r) = resample_rule.replicate([Q, C_0, ..], s, seed, r, keep): the keep function, "full" means
                  len == s, s_r the smallest kept count among the full lists of THIS set, s when none is full; s_r == 0 fails
    pair        = (common, denom) of candidate i = mo.compare(lists_r[1 + i], lists_r[0], s_r, k)
    best        = the first candidate in the order search_rule.ranked: the Jaccard index compared exactly in integers,
                  common == denom as 1/1 (0/0 included), ties by the lower reference index
    first[i]    = the number of replicates whose best candidate is i; they sum to R for a query that has candidates
    rep_best[r] = the reference index of the best candidate, 0xFFFFFFFF without candidates

The cut does not matter.  Given s_r, compare(cut(A), cut(B), s_r) == compare(kept(A), kept(B), s_r), where kept(X) is what the
replicate keeps of X and cut(X) its first min(len, s_r) hashes.  compare counts, among the first s_r distinct values of the
union of its two lists (all of them when there are fewer), those that both lists hold, and gives min(s_r, size of the union)
as denom.  If a kept list holds at least s_r hashes, its s_r-th hash is a value of the union with at least s_r - 1 union
values below it, so the s_r-th distinct value of the union lies at or below that list's cut: everything the comparison counts
lies below both cuts, where cut and kept lists agree, and the union has s_r values either way.  If neither list reaches s_r
neither is cut.  So the device needs the kept counts (for s_r) and ONE ascending walk over the distinct values of A u B per
pair: per replicate u counts the kept distinct values and c those present in both lists while u <= s_r; then common = c and
denom = min(s_r, u) -- `walk` below, checked against the rule by tests/test_support_rule.py.

    text        = search_rule.search_text's rows with a sixth column "c/R", c = first of the row's reference among the query's
                  hits (within max_dist, at most top, before max_p_value drops rows); with clades {reference name: clade} two
                  more: the clade of the row's reference and "g/R", g = the replicates whose best candidate has that clade
"""
import numpy as np

from oracle import mash_oracle as mo
from tests import resample_rule as rr
from tests import search_rule as sr

NONE = 0xFFFFFFFF


class Support:
    """first [m], rep_best [R], rep_s [R], rep_common and rep_denom [m, R] of one query"""

    def __init__(self, m, R):
        self.first = np.zeros(m, np.uint32)
        self.rep_best = np.full(R, NONE, np.uint32)
        self.rep_s = np.zeros(R, np.uint32)
        self.rep_common = np.zeros((m, R), np.uint32)
        self.rep_denom = np.zeros((m, R), np.uint32)


def _finish(out, r, s_r, refs, pairs):
    out.rep_s[r] = s_r
    for i, (common, denom) in enumerate(pairs):
        out.rep_common[i, r], out.rep_denom[i, r] = common, denom
    if pairs:
        best = sr.ranked([(refs[i], c, d, i) for i, (c, d) in enumerate(pairs)])[0]
        out.rep_best[r] = best[0]
        out.first[best[3]] += 1


def support(Q, cands, refs, s, k, replicates, keep, seed):
    """The rule, plain and slow.  cands: the candidate lists, refs: their reference indices (distinct)."""
    out = Support(len(cands), replicates)
    for r in range(replicates):
        lists, s_r = rr.replicate([Q] + list(cands), s, seed, r, keep)
        _finish(out, r, s_r, refs, [mo.compare(lists[1 + i], lists[0], s_r, k)[:2] for i in range(len(cands))])
    return out


# ---- the same, quicker: the keep function over whole arrays ----------------------------------------------------------------
def keep_mask(v, seed, r, T):
    """resample_rule.keeps for every hash of the uint64 array v (numpy's uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        z = v.astype(np.uint64) + np.uint64((seed + (r + 1) * rr.GAMMA) & rr.MASK)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(rr.MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(rr.MUL2)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)).astype(np.int64) < T


def kept_lists(lists, s, seed, r, keep):
    """(the kept lists of replicate r, UNCUT, and s_r); ValueError as resample_rule.replicate"""
    T = rr.threshold(keep)
    kept = [np.asarray(v, np.uint64)[keep_mask(np.asarray(v, np.uint64), seed, r, T)] for v in lists]
    full = [len(kv) for v, kv in zip(lists, kept) if len(v) == s]
    s_r = min(full) if full else s
    if s_r == 0:
        raise ValueError("replicate %d keeps no hash of a full list at keep = %g" % (r, keep))
    return kept, s_r


def support_fast(Q, cands, refs, s, k, replicates, keep, seed):
    """support() with the keep function over arrays; the same values (tests/test_support_rule.py)"""
    out = Support(len(cands), replicates)
    for r in range(replicates):
        kept, s_r = kept_lists([Q] + list(cands), s, seed, r, keep)
        _finish(out, r, s_r, refs, [mo.compare(kept[1 + i][:s_r], kept[0][:s_r], s_r, k)[:2] for i in range(len(cands))])
    return out


def walk(A, B, s_r):
    """(common, denom) of two KEPT, uncut lists by the walk the device form takes: ascending over the distinct values of
    A u B, u the values so far, c those in both lists while u <= s_r"""
    a, b = set(int(x) for x in A), set(int(x) for x in B)
    u = c = 0
    for v in sorted(a | b):
        u += 1
        if u <= s_r and v in a and v in b:
            c += 1
    return c, min(s_r, u)


def search_support_text(R, query_files, top=5, max_dist=1.0, max_p_value=1.0, replicates=0, keep=0.5, seed=42, clades=None):
    """R and query_files are mo.SketchFile; clades {reference name: clade} or None"""
    k = R.kmer_size
    rows = []
    for Q in query_files:
        s = max(1, min(R.sketch_size, Q.sketch_size))
        for q in Q.references:
            hits = sr.search([q.hashes], [x.hashes for x in R.references], s, k, top, max_dist)[0]
            sup = support_fast(q.hashes, [R.references[h[0]].hashes for h in hits], [h[0] for h in hits], s, k, replicates, keep, seed)
            for t, (r, common, denom, d) in enumerate(hits):
                ref = R.references[r]
                p = mo.p_value(common, ref.length, q.length, 4.0 ** k, denom)
                if not p <= max_p_value:
                    continue
                row = "%s\t%s\t%s\t%s\t%d/%d\t%d/%d" % (ref.name, q.name, mo.fmt_g(d), mo.fmt_g(p), common, denom, sup.first[t], replicates)
                if clades is not None:
                    g = sum(int(sup.first[x]) for x, h in enumerate(hits) if clades[R.references[h[0]].name] == clades[ref.name])
                    row += "\t%s\t%d/%d" % (clades[ref.name], g, replicates)
                rows.append(row + "\n")
    return "".join(rows)

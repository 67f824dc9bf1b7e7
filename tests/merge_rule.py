"""The rule of the sharded path's merge, in plain Python (what mhx_sketcher_merge_slabs / _merge_gathered must compute on
every path: binned, table, host).  A rank is (header, hashes, counts): the 8-word header [n, T, flags, #(2^64-1),
occupied, 0, 0, 0] and its slab, which may be longer than n.

1. an entry counts when its index < n_r and its hash <= T_min = min_r T_r; 2^64-1 is never taken from a slab (it marks a
   vacant slot) and enters only through header word 3, when T_min = 2^64-1;
2. the counts of equal hashes are summed in Python integers and clamped at 2^32-1;
3. the sums >= m, ascending, first s, are the sketch;
4. fewer than s of them while T_min < hash_max (2^32-1 for k <= 16) is MHX_E_CAPACITY: the partials do not determine the
   sketch of the union."""
import numpy as np

MAX64 = (1 << 64) - 1
MAX32 = (1 << 32) - 1
CAPACITY = "MHX_E_CAPACITY"


def hash_max(k):
    return MAX32 if k <= 16 else MAX64


def t_min_of(ranks):
    return min(int(hdr[1]) for hdr, _, _ in ranks)


def taken(ranks):
    """[(hash, count)] of step 1, as Python integers, rank after rank"""
    t_min = t_min_of(ranks)
    out = []
    for hdr, hashes, counts in ranks:
        n = int(hdr[0])
        h = np.asarray(hashes, dtype=np.uint64)[:n]
        c = np.asarray(counts, dtype=np.uint32)[:n]
        keep = (h <= np.uint64(t_min)) & (h != np.uint64(MAX64))
        out += zip(h[keep].tolist(), c[keep].tolist())
    if t_min == MAX64:
        out += [(MAX64, int(hdr[3])) for hdr, _, _ in ranks if int(hdr[3])]
    return out


def sums(ranks):
    """{hash: clamped sum} of step 2"""
    acc = {}
    for h, c in taken(ranks):
        acc[h] = acc.get(h, 0) + c
    return {h: min(c, MAX32) for h, c in acc.items()}


def merge(ranks, k, s, m):
    """(hashes uint64, counts uint32) of the union's sketch, or CAPACITY"""
    m = max(1, m)
    kept = sorted((h, c) for h, c in sums(ranks).items() if c >= m)[:s]
    if len(kept) < s and t_min_of(ranks) < hash_max(k):
        return CAPACITY
    return np.array([h for h, _ in kept], dtype=np.uint64), np.array([c for _, c in kept], dtype=np.uint32)

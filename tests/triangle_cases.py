"""Sketch sets for the all-pairs distance (mhx_dist_triangle), shared by the CPU emulation test and the GPU tests, and what
the oracle says about each: mo.compare of every pair j < i, packed at i (i - 1) / 2 + j.  Sets and expectations are
computed once per process."""
import functools

import numpy as np

from oracle import mash_oracle as mo


def sketch_like(rng, n, hi=2 ** 64):
    return np.unique(rng.integers(0, hi, size=n, dtype=np.uint64))


def mutate(rng, base, drop, hi=2 ** 64):
    """`base` with a share `drop` of its hashes replaced by fresh ones"""
    keep = rng.random(len(base)) >= drop
    return np.unique(np.concatenate([base[keep], sketch_like(rng, int((~keep).sum()), hi)]))


def pad_rows(lists, stride=None):
    if stride is None:
        stride = (max(max(map(len, lists)), 1) + 15) // 16 * 16   # rows of whole 128-byte lines
    M = np.zeros((len(lists), stride), np.uint64)
    for i, v in enumerate(lists):
        M[i, :len(v)] = v
    return M, np.array([len(v) for v in lists], np.uint32)


@functools.lru_cache(maxsize=None)
def set70():
    """70 lists at s = 1000: a base list with 10 close copies, the rest independent; one empty list, one of 17 hashes, one
    exact duplicate, one cut to a third of the value space, one with only values >= 2^63.  Three slices, the last partial."""
    rng = np.random.default_rng(7070)
    s = 1000
    base = sketch_like(rng, s)
    lists = [base] + [mutate(rng, base, 0.004 * (j + 1)) for j in range(10)]
    lists += [sketch_like(rng, s) for _ in range(70 - len(lists))]
    lists[20] = np.zeros(0, np.uint64)
    lists[21] = lists[21][:17]
    lists[40] = lists[15].copy()
    lists[23] = lists[23][lists[23] < np.uint64(2 ** 64 // 3)]
    lists[66] = lists[66][lists[66] >= np.uint64(1 << 63)]
    return tuple(lists), s


@functools.lru_cache(maxsize=None)
def set200():
    """200 lists at s = 1000: eight clades of ten lists whose members lie 0.2 % .. 90 % of their hashes from the clade's
    base (distances all over 0 .. 0.3 at k = 21), four identical lists and another exact duplicate, a short and an empty list, the rest independent."""
    rng = np.random.default_rng(200200)
    s = 1000
    lists = [sketch_like(rng, s) for _ in range(200)]
    for c in range(8):
        base = lists[3 + 23 * c]
        for m in range(10):
            lists[(3 + 23 * c + 7 * (m + 1)) % 200] = mutate(rng, base, min(0.9, 0.002 * 2.0 ** (m + c % 3)))
    lists[190] = lists[5].copy()
    lists[191] = lists[5].copy()
    lists[196] = lists[5].copy()
    lists[77] = lists[141].copy()
    lists[150] = lists[150][:17]
    lists[33] = np.zeros(0, np.uint64)
    return tuple(lists), s


@functools.lru_cache(maxsize=None)
def long_set(n, length):
    """n lists of `length` hashes: every fourth a close copy of its neighbour, one short, the rest independent"""
    rng = np.random.default_rng([n, length])
    lists = [sketch_like(rng, length) for _ in range(n)]
    for i in range(3, n, 4):
        lists[i] = mutate(rng, lists[i - 1], 0.01 * i)
    lists[1] = lists[1][:length // 3]
    return tuple(lists), length


@functools.lru_cache(maxsize=None)
def crowded(n=40):
    """The non-uniform construction of test_crowded_values_raise_the_flag: 3000 values inside 2^20 of 2^62, one list that
    reaches the top of the value space -- one value range holds nearly everything."""
    rng = np.random.default_rng(22)
    lo = 1 << 62
    refs = [lo + sketch_like(rng, 3000, hi=2 ** 20) for _ in range(8)]
    lists = [refs[i] if i < 8 else np.unique(np.concatenate([refs[i % 8][::2], lo + sketch_like(rng, 1500, hi=2 ** 20)])) for i in range(n)]
    lists[8] = np.concatenate([refs[0][:1000], np.array([2 ** 64 - 5], np.uint64)])
    return tuple(lists), 3000


@functools.lru_cache(maxsize=None)
def flagged_groups():
    """512 lists of 64 hashes at s = 64 (16 value ranges): with one query per block that is 4336 blocks, one per (slice, query)
    -- slice r0 has the queries r0 + 1 .. 511 --, the last 240 in a second group of flag words; block 4096 is (slice 384,
    query 461).  The lists are those of contain_search_cases.flagged_groups; slices 64..95 and 448..479 are then crowded into
    one value range, more keys than the 1536 of a range table, so every block of these two slices raises its flag, 447 + 63 =
    510 in all, in both groups (the table holds the references' keys only: no other block can).  Every fourth crowded list
    derives from one of four crowded bases, so that pairs inside the crowd share hashes."""
    rng = np.random.default_rng(4336)
    s, n = 64, 512
    bases = [sketch_like(rng, s) for _ in range(30)]
    lists = [mutate(rng, bases[j % 30], 0.02 * (j % 11)) if j % 3 else sketch_like(rng, s) for j in range(n)]
    crowd = [sketch_like(rng, s, hi=2 ** 20) for _ in range(4)]
    for j in list(range(64, 96)) + list(range(448, 480)):
        low = mutate(rng, crowd[(j // 4) % 4], 0.05, hi=2 ** 20) if j % 4 == 0 else sketch_like(rng, s, hi=2 ** 20)
        lists[j] = np.uint64(1 << 62) + low
    return tuple(lists), s


def flagged_groups_blocks(n=512):
    """the block of every packed pair (i, j), j < i, of flagged_groups under one query per block, in the order of oracle_pairs"""
    first = np.cumsum([0] + [n - 1 - r0 for r0 in range(0, n, 32)])   # of every slice
    ii = np.array([i for i in range(n) for j in range(i)], np.int64)
    jj = np.array([j for i in range(n) for j in range(i)], np.int64)
    r0 = jj // 32 * 32
    return first[jj // 32] + (ii - r0 - 1), r0


def oracle_pairs(lists, s, k):
    """packed (common, denom, dist) of mo.compare(list_i, list_j) for j < i"""
    n = len(lists)
    common = np.zeros(n * (n - 1) // 2, np.uint32)
    denom = np.zeros_like(common)
    dist = np.zeros(common.size, np.float64)
    at = 0
    for i in range(n):
        for j in range(i):
            common[at], denom[at], dist[at] = mo.compare(lists[i], lists[j], s, k)
            at += 1
    return common, denom, dist


@functools.lru_cache(maxsize=None)
def expected(name, k=21, *args):
    lists, s = globals()[name](*args)
    return oracle_pairs(lists, s, k)

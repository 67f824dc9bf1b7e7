"""Hash lists that hold the values uniform draws never produce, shared by the CPU emulation tests and the GPU tests of the
distance path (tests/test_gpu_dist_extreme_values.py): 2^64 - 1 -- kEmptyKey, the vacant-slot marker of the range table
(mhx_dist.h) -- next to a value `w` whose home slot in that table is the same, hash 0 in zero-padded rows, and calls whose
largest value is tiny or an exact power of two.  Not a test module itself.

The planted batch.  The range table of a value range is built reference by reference; a wave inserts its references in
program order, and references 0, 8 and 16 belong to wave 0 in every form of the range pass (index modulo 4 and modulo 8),
so what happens between these three does not depend on scheduling.  2^64 - 1 and the values w, w2 of the same home slot
all lie in the top value range of every geometry up to 2048 ranges (they are >= 2^64 - 2^53).

    plain      reference 0 ends in 2^64 - 1, reference 8 holds w; query 0 holds w, query 1 ends in 2^64 - 1.
               A table that takes 2^64 - 1 for a key leaves its slot vacant with reference 0's bit on it; w claims the slot
               and inherits the bit: (query 0, reference 0) one too HIGH.  Query 1 then walks past w to the next vacant
               slot and reads no bit: (query 1, reference 0) one too LOW.
    mirrored   reference 0 holds w, reference 8 ends in 2^64 - 1, reference 16 holds w2; query 0 holds w and w2, query 1
               ends in 2^64 - 1.  2^64 - 1 leaves reference 8's bit on the vacant slot behind w, w2 claims that slot:
               (query 0, reference 8) one too high, (query 1, reference 8) one too low.

For the top range to count at all a pair's union must stay below s (with two independent lists of s hashes the walk ends in
the middle of the value space): most lists have 450 hashes at s = 1000, a few have all 1000 (they set the geometry: 64
ranges for the triangle and the search, 1024 for mhx_dist_batch).  No other value of the top sixteenth of the value space
has its home slot within 64 slots of that of 2^64 - 1, so nothing else can claim the slots the construction is about.
Query 6 is reference 0 itself, query 7 is reference 0 without its 2^64 - 1: two lists that differ in that value alone."""
import functools

import numpy as np

from oracle import mash_oracle as mo
from tests import triangle_cases as tc

EMPTY = 2 ** 64 - 1          # kEmptyKey (mhx_device_consts.h)
S = 1000
K = 21
SLOTS = 2048                 # kDistTableSlots
TOP_SIXTEENTH = 2 ** 64 - 2 ** 60   # the top range of the coarsest geometry (16 ranges)


def slot_of(v):
    """dist_slot_of (mhx_dist.h) of an array of values"""
    v = np.atleast_1d(np.asarray(v, np.uint64))
    return (((v * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)) & np.uint64(SLOTS - 1)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def colliders():
    """w, w2: the two largest values below 2^64 - 1 with its home slot (about one value in 2048 has it)"""
    cand = np.uint64(EMPTY - 1) - np.arange(1 << 16, dtype=np.uint64)
    hit = cand[slot_of(cand) == slot_of(EMPTY)[0]]
    assert hit.size >= 2 and int(hit[1]) >= 2 ** 64 - 2 ** 53
    return int(hit[0]), int(hit[1])


def clear_of_the_slot(v):
    """v without the values of the top sixteenth whose home slot is within 64 of the slot of 2^64 - 1"""
    d = (slot_of(v) - slot_of(EMPTY)[0]) % SLOTS
    return v[~((v >= np.uint64(TOP_SIXTEENTH)) & ((d <= 64) | (d >= SLOTS - 64)))]


def add(v, *values):
    return np.unique(np.concatenate([v, np.array(values, np.uint64)]))


def plant(refs, qrys, mirrored):
    """the construction of the module docstring on lists of any length (at least 17 references, 8 queries)"""
    refs, qrys = [clear_of_the_slot(v) for v in refs], [clear_of_the_slot(v) for v in qrys]
    w, w2 = colliders()
    if not mirrored:
        refs[0], refs[8] = add(refs[0], EMPTY), add(refs[8], w)
        qrys[0] = add(qrys[0], w)
    else:
        refs[0], refs[8], refs[16] = add(refs[0], w), add(refs[8], EMPTY), add(refs[16], w2)
        qrys[0] = add(qrys[0], w, w2)
    qrys[1] = add(qrys[1], EMPTY)
    holder = refs[8] if mirrored else refs[0]
    qrys[6] = holder.copy()
    qrys[7] = holder[:-1].copy()
    assert holder[-1] == np.uint64(EMPTY) and qrys[1][-1] == np.uint64(EMPTY)
    return refs, qrys


@functools.lru_cache(maxsize=None)
def batch(nq, mirrored=False):
    """(queries, 33 references, s): two reference slices, the second of one list"""
    rng = np.random.default_rng(6464)
    refs = [tc.sketch_like(rng, 450) for _ in range(33)]
    refs[3] = tc.sketch_like(rng, S)
    qrys = [tc.mutate(rng, refs[i % 33], 0.05 + 0.07 * (i % 7)) for i in range(nq)]
    qrys[4] = tc.sketch_like(rng, S)                 # against reference 3 the walk ends in the middle of the value space
    qrys[9] = np.zeros(0, np.uint64)
    refs, qrys = plant(refs, qrys, mirrored)
    return tuple(qrys), tuple(refs), S


def holders(lists):
    """indices of the lists that end in 2^64 - 1"""
    return [i for i, v in enumerate(lists) if len(v) and v[-1] == np.uint64(EMPTY)]


def oracle_matrix(qrys, refs, s, k=K):
    """(common, denom, dist) [nq, nr] of mo.compare(reference, query)"""
    common = np.zeros((len(qrys), len(refs)), np.uint32)
    denom = np.zeros_like(common)
    dist = np.zeros(common.shape, np.float64)
    for i, q in enumerate(qrys):
        for j, r in enumerate(refs):
            common[i, j], denom[i, j], dist[i, j] = mo.compare(r, q, s, k)
    return common, denom, dist


@functools.lru_cache(maxsize=None)
def batch_expected(nq, mirrored=False):
    qrys, refs, s = batch(nq, mirrored)
    return oracle_matrix(qrys, refs, s)


@functools.lru_cache(maxsize=None)
def batch_as_one_set(nq, mirrored=False):
    """the references followed by the queries as ONE set for the triangle, and the oracle's packed pairs"""
    qrys, refs, s = batch(nq, mirrored)
    lists = refs + qrys
    return lists, s, tc.oracle_pairs(lists, s, K)


# ---- the neighbouring values ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def with_zero():
    """Lists that hold hash 0 (rows are zero-padded: only the length tells a real 0 from padding): references and queries
    that begin with 0, the list [0] alone on either side, an empty list next to it, and lists without it."""
    rng = np.random.default_rng(1000)
    refs = [tc.sketch_like(rng, 450) for _ in range(33)]
    refs[3] = tc.sketch_like(rng, S)
    qrys = [tc.mutate(rng, refs[i % 33], 0.05 + 0.07 * (i % 7)) for i in range(40)]
    for i in (0, 5, 8, 32):
        refs[i] = add(refs[i], 0)
    refs[2] = np.zeros(1, np.uint64)
    refs[4] = np.zeros(0, np.uint64)
    for i in (0, 1, 12):
        qrys[i] = add(qrys[i], 0)
    qrys[2] = np.zeros(1, np.uint64)
    qrys[3] = np.zeros(0, np.uint64)
    qrys[6] = np.array([0, 1], np.uint64)
    return tuple(qrys), tuple(refs), S


def small_values(rng, n, hi, nlists):
    return [np.unique(rng.integers(0, hi, size=n, dtype=np.uint64)) for _ in range(nlists)]


@functools.lru_cache(maxsize=None)
def below_the_ranges(hi, n, s):
    """every value below `hi`, the number of value ranges or less: dist_shift_for gives shift 0 and a value IS its range;
    lists of up to n values, one reference holds every value 0 .. min(hi, s) - 1"""
    rng = np.random.default_rng([hi, n])
    refs = small_values(rng, n, hi, 33)
    qrys = small_values(rng, n, hi, 40)
    qrys[3], qrys[4], refs[7] = refs[2].copy(), np.zeros(0, np.uint64), np.arange(min(hi, s), dtype=np.uint64)
    refs[1] = add(refs[1], hi - 1)
    return tuple(qrys), tuple(refs), s


@functools.lru_cache(maxsize=None)
def power_of_two_top(b, exact):
    """values below 2^b; the call's largest is 2^b - 1 (all ranges in use, the top one ends exactly at the largest value) or,
    `exact`, 2^b itself (one more bit: the lower half of the ranges in use and one value alone in the range above them)"""
    rng = np.random.default_rng([b, int(exact)])
    refs = [tc.sketch_like(rng, 450, hi=2 ** b) for _ in range(33)]
    refs[3] = tc.sketch_like(rng, S, hi=2 ** b)
    qrys = [tc.mutate(rng, refs[i % 33], 0.05 + 0.07 * (i % 7), hi=2 ** b) for i in range(40)]
    top = 2 ** b if exact else 2 ** b - 1
    refs[5], qrys[5], qrys[11] = add(refs[5], top), add(qrys[5], top), add(qrys[11], top)
    assert max(int(v[-1]) for v in refs + qrys if len(v)) == top
    return tuple(qrys), tuple(refs), S

"""The rule of the jackknife over the hashes of a sketch set (mhx_resample_rows; auriclass_amd/csrc/mhx_resample.h) as a plain
statement, plain and slow, in Python integers.  Shared by the resampling and support tests; not a test module itself.

    keep        = a hash h is kept in replicate r (0-based) of a call with seed `seed` iff (z >> 32) < T, all mod 2^64:
                      z = h + seed + (r + 1) * 0x9E3779B97F4A7C15
                      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
                      z = (z ^ (z >> 27)) * 0x94D049BB133111EB
                      z ^= z >> 31
                  T = floor(keep * 2^32) from the double keep, 0 < keep <= 1; T may be 2^32.  The decision depends on the hash
                  alone: a hash that two lists share is kept in both or in neither
    replicate   = list i' is the kept hashes of list i, in order; a list with len == s is full, a shorter one a complete set;
                  s_r = the smallest kept count among the full lists, s when no list is full; s_r == 0 fails; every list is cut
                  to its first min(len', s_r) hashes -- a bottom-s_r sketch -- and compared at sketch size s_r, the same k
"""
import math

import numpy as np

MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB


def mix(h, seed, r):
    z = (h + seed + (r + 1) * GAMMA) & MASK
    z = ((z ^ (z >> 30)) * MUL1) & MASK
    z = ((z ^ (z >> 27)) * MUL2) & MASK
    return z ^ (z >> 31)


def threshold(keep):
    if not (0.0 < keep <= 1.0):      # (false for a keep that is not a number, too)
        raise ValueError("keep must lie in (0, 1]: %r" % (keep,))
    return int(math.floor(keep * 2.0 ** 32))


def keeps(h, seed, r, T):
    return (mix(int(h), seed, r) >> 32) < T


def replicate(lists, s, seed, r, keep):
    """(the lists of replicate r, s_r); ValueError when a full list keeps nothing"""
    T = threshold(keep)
    kept = [[int(h) for h in v if keeps(h, seed, r, T)] for v in lists]
    full = [len(kv) for v, kv in zip(lists, kept) if len(v) == s]
    s_r = min(full) if full else s
    if s_r == 0:
        raise ValueError("replicate %d keeps no hash of a full list at keep = %g" % (r, keep))
    return [np.array(kv[:s_r], np.uint64) for kv in kept], s_r

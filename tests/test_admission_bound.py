"""The admission test of the sketch kernel's hash loop on the CPU (tests/emul/admission_bound_emul.cpp).  A window's hash is
h = xorshift33(a) + xorshift33(b) with a = ka * C2, b = kb * C2; the loop tests `Murmur3Tail{ka, kb}.high_bound() <=
admission_limit(T)`, the high word of the ONE product (ka + kb) * C2 plus one against hi(T) + 2, and only the windows that
pass do the two products.  That test must never reject a hash <= T, whatever the two carries (of the products' low words,
and of their shift-xored low words) are, and it must not pass more than the three high words around hi(T) it gives away.
The tails are built backwards from chosen products: ka = a * C2^-1."""
import ctypes

import numpy as np
import pytest

from tests import emul_build

C2 = 0xC4CEB9FE1A85EC53
EDGE_HIGH = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint64)
EDGE_LOW = np.array([0, 1, 0x80000000, 0xFFFFFFFF], dtype=np.uint64)
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
SATURATED = 0xFFFFFFFD  # from this high word of T on the bound says nothing


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("admission_bound_emul")
    L.emul_fmix_c2_inverse.restype = ctypes.c_uint64
    L.emul_tails.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_tails.restype = None
    L.emul_admission_limits.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.emul_admission_limits.restype = None
    return L


def xorshift33(x):
    return x ^ (x >> np.uint64(33))


def products():
    """The chosen (a, b): random pairs, and every pairing of edge high words -- the two taken from the list, or the second
    chosen so that the sum of the two (alone, or with a carry from the low words) is one of the list -- with low words
    from the edge list and random ones."""
    rng = np.random.default_rng(20240521)
    n = 200_000
    a = [rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]
    b = [rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]
    ha, other = (x.ravel() for x in np.meshgrid(EDGE_HIGH, EDGE_HIGH, indexing="ij"))
    high_pairs = np.concatenate([
        np.stack([ha, other]),                                    # both from the list
        np.stack([ha, (other - ha) & M32]),                       # summing to a value of the list
        np.stack([ha, (other - ha - np.uint64(1)) & M32]),        # ... once the low words carry
    ], axis=1)
    for draw in range(8):
        lows = np.concatenate([EDGE_LOW, rng.integers(0, 1 << 32, size=1, dtype=np.uint64)])
        la, lb = (x.ravel() for x in np.meshgrid(lows, lows, indexing="ij"))
        # every pair of high words with every pair of low words
        a.append(((high_pairs[0][:, None] << S32) | la[None, :]).ravel())
        b.append(((high_pairs[1][:, None] << S32) | lb[None, :]).ravel())
    return np.concatenate(a), np.concatenate(b)


@pytest.fixture(scope="module")
def tails(emul):
    a, b = products()
    inv = np.uint64(emul.emul_fmix_c2_inverse())
    assert (int(inv) * C2) % (1 << 64) == 1
    ka, kb = a * inv, b * inv  # uint64 arrays: products mod 2^64
    assert np.array_equal(ka * np.uint64(C2), a) and np.array_equal(kb * np.uint64(C2), b)
    n = len(a)
    h = np.zeros(n, np.uint64)
    low = np.zeros(n, np.uint32)
    bound = np.zeros(n, np.uint32)
    emul.emul_tails(ka.ctypes.data, kb.ctypes.data, n, h.ctypes.data, low.ctypes.data, bound.ctypes.data)
    return a, b, h, low, bound


def limits(emul, T):
    T = np.ascontiguousarray(T, dtype=np.uint64)
    out = np.zeros(len(T), np.uint32)
    emul.emul_admission_limits(T.ctypes.data, len(T), out.ctypes.data)
    return out


def thresholds(h):
    """The thresholds every tail is tested against: at the hash, around it, and at the top of the range."""
    hi = h >> S32
    return [h, h + np.uint64(1), h | M32, hi << S32, np.full_like(h, ALL), np.full_like(h, ALL - np.uint64(1)),
            np.full_like(h, ALL - (np.uint64(3) << S32))]


def test_all_carry_combinations_occur(tails):
    a, b, _, _, _ = tails
    c1 = ((a & M32) + (b & M32)) >> S32
    c2 = ((xorshift33(a) & M32) + (xorshift33(b) & M32)) >> S32
    for want1 in (0, 1):
        for want2 in (0, 1):
            assert np.count_nonzero((c1 == want1) & (c2 == want2)) >= 1000, (want1, want2)


def test_finish_is_the_hash(tails):
    a, b, h, low, _ = tails
    want = xorshift33(a) + xorshift33(b)
    assert np.array_equal(h, want)
    assert np.array_equal(low, (want & M32).astype(np.uint32))


def test_admission_limit(emul):
    hi = np.concatenate([EDGE_HIGH, np.array([3, 0xFFFFFFFB, 0xFFFFFFFC], dtype=np.uint64)])
    for lo in (0, 1, 0xFFFFFFFF):
        got = limits(emul, (hi << S32) | np.uint64(lo))
        want = np.where(hi >= SATURATED, 0xFFFFFFFF, hi + np.uint64(2)).astype(np.uint32)
        assert np.array_equal(got, want)


def test_no_hash_at_or_below_the_threshold_is_rejected(emul, tails):
    _, _, h, _, bound = tails
    for i, T in enumerate(thresholds(h)):
        below = h <= T
        assert np.count_nonzero(below) > 0, i
        rejected = below & (bound > limits(emul, T))
        assert not rejected.any(), (i, hex(int(h[rejected][0])), hex(int(T[rejected][0])))


def test_the_bound_is_not_vacuous(emul, tails):
    _, _, h, _, bound = tails
    hh = h >> S32
    rng = np.random.default_rng(7)
    checked = 0
    for T in thresholds(h) + [rng.integers(0, 1 << 64, size=len(h), dtype=np.uint64)]:
        th = T >> S32
        passed = (bound <= limits(emul, T)) & (th < SATURATED)
        ok = (hh <= th + np.uint64(2)) | (hh >= 0xFFFFFFFE)
        assert not (passed & ~ok).any()
        checked += int(np.count_nonzero(passed))
    assert checked > 100_000

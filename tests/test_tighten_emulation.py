"""CPU emulation of the tighten pass's threshold rule (auriclass_amd/csrc/mhx_tighten.h, the very functions the kernel's
last workgroup runs) against the arithmetic the kernel carried inline before (tests/emul/tighten_emul.cpp), and against
plain statements of what a pass must leave behind: T never rises, at least s qualifying entries lie at or below it."""
import ctypes

import numpy as np
import pytest

from tests import emul_build

BINS = 2048
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("tighten_emul")
    for f in (L.emul_tighten, L.emul_tighten_former):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                      ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        f.restype = ctypes.c_uint64
    for f in (L.emul_tighten_bin, L.emul_tighten_bin_former):
        f.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
        f.restype = ctypes.c_uint32
    return L


def both(L, hist, T, s, sample=1, m=1, next_cap=0, occupied=0, solid=0, state=(0, 0)):
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    assert hist.size == BINS
    out = []
    for f in (L.emul_tighten, L.emul_tighten_former):
        st = np.array(state, dtype=np.int32)
        out.append((f(hist.ctypes.data, T, s, sample, m, next_cap, occupied, solid, st.ctypes.data), int(st[0]), int(st[1])))
    assert out[0] == out[1], (T, s, sample, m, next_cap, state)
    return out[0]


def one_bin(i, n):
    h = np.zeros(BINS, np.uint32)
    h[i] = n
    return h


def test_cut_in_the_first_bin(emul):
    T = U64
    now, est, bnd = both(emul, one_bin(0, 1000), T, 1000)
    assert now == (1 << 53) - 1 and (est, bnd) == (0, 0)       # last value of bin 0 of a 64-bit range
    assert both(emul, one_bin(0, 5000), T, 1000, m=3)[:2] == ((1 << 53) - 1, 1)    # m > 1: T now follows the solid hashes


def test_cut_in_the_last_bin(emul):
    T = U64
    h = np.zeros(BINS, np.uint32)
    h[:BINS - 1] = 0
    h[5] = 999
    h[BINS - 1] = 1
    assert both(emul, h, T, 1000)[0] == T                      # the edge of the last bin is T itself: nothing to lower
    T2 = (1 << 40) + 12345                                     # a threshold inside its top bin: the last bin's edge lies above it
    top = emul.emul_tighten_bin(T2, T2)
    assert top == 1024                                         # the leading one of T, then ten zero bits
    h = one_bin(top, 1000)
    assert both(emul, h, T2, 1000)[0] == T2
    h = one_bin(top - 1, 1000)
    assert both(emul, h, T2, 1000)[0] == (1 << 40) - 1


def test_no_cut(emul):
    rng = np.random.default_rng(3)
    h = rng.multinomial(999, np.full(BINS, 1 / BINS)).astype(np.uint32)
    for T in (U64, 1 << 50, 12345678901234):
        assert both(emul, h, T, 1000) == (T, 0, 0)
    assert both(emul, np.zeros(BINS, np.uint32), U64, 1) == (U64, 0, 0)
    # ... but the byte-count cap of the next launch still applies (m > 1, not established, table not "small genome, deep")
    assert both(emul, h, U64, 1000, m=3, next_cap=1 << 60, occupied=100000, solid=999) == (1 << 60, 0, 1)
    assert both(emul, h, U64, 1000, m=3, next_cap=1 << 60, occupied=4000, solid=999) == (U64, 0, 0)       # a fifth solid
    assert both(emul, h, U64, 1000, m=3, next_cap=1 << 60, occupied=100000, solid=999, state=(1, 0)) == (U64, 1, 0)
    assert both(emul, h, 1 << 59, 1000, m=3, next_cap=1 << 60, occupied=100000, solid=999) == (1 << 59, 0, 0)  # T never rises


def test_threshold_with_fewer_than_11_significant_bits(emul):
    for T in (0, 1, 5, 1023, 2047):                            # lz > 52: bins are finer than integers, T stays
        h = one_bin(emul.emul_tighten_bin(min(T, 3), T), 5000)
        assert both(emul, h, T, 1000) == (T, 0, 0)
    assert both(emul, one_bin(0, 5000), 2048, 1000)[0] == 1    # lz = 52: the first threshold the rule can lower (bin = 2 values)
    assert both(emul, one_bin(0, 5000), 4095, 1000)[0] == 1


@pytest.mark.parametrize("sample", [1, 8])
@pytest.mark.parametrize("s", [1, 16, 1000, 8191, 50000])
def test_random_histograms_sampled_and_exact(emul, sample, s):
    rng = np.random.default_rng(1000 * sample + s)
    target = s if sample == 1 else int(np.float32(s) / np.float32(sample) + np.float32(6.0) * np.sqrt(np.float32(s) / np.float32(sample))) + 16
    for trial in range(60):
        T = int(rng.integers(1, 1 << 63)) >> int(rng.integers(0, 50)) | 1
        top = emul.emul_tighten_bin(T, T)
        total = int(target * rng.choice([0.5, 0.99, 1.0, 1.5, 4.0, 40.0]))
        h = np.zeros(BINS, np.uint32)
        if total:
            h[: top + 1] = rng.multinomial(total, np.full(top + 1, 1 / (top + 1)))
        m = int(rng.choice([1, 3]))
        cap = int(rng.choice([0, T >> 3, T << 1 & U64]))
        now, est, bnd = both(emul, h, T, s, sample=sample, m=m, next_cap=cap, occupied=int(rng.integers(0, 10 * total + 1)),
                             solid=total, state=(int(rng.integers(0, 2)), 0))
        assert now <= T
        if not bnd and now < T:                                # lowered by the histogram: enough entries at or below the new T
            bin_now = emul.emul_tighten_bin(now, T)
            assert int(h[: bin_now + 1].sum()) >= target > int(h[:bin_now].sum())


def test_bin_of_a_hash(emul):
    rng = np.random.default_rng(9)
    for _ in range(2000):
        T = (int(rng.integers(0, 1 << 63)) << 1 | 1) >> int(rng.integers(0, 64))
        key = int(rng.integers(0, T + 1)) if T < (1 << 63) else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        key = min(key, T)
        b = emul.emul_tighten_bin(key, T)
        assert b == emul.emul_tighten_bin_former(key, T) < BINS
        lz = 64 - T.bit_length() if T else 63
        assert b == ((key << lz) & U64) >> 53

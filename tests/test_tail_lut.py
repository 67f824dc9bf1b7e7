"""The tail tables of the hash (auriclass_amd/csrc/mhx_tail_lut.h) on the CPU (tests/emul/tail_lut_emul.cpp): the partial
8-byte word of Murmur's tail block, t = 1..5 bases, as a look-up indexed by bits 1..2 of every base.

  * every entry of every table against the formula, in Python integers;
  * the index for all 256 values of a byte in every position: inside the table (the hot loop also hashes windows that
    hold newlines, quality characters and N, and their load must stay inside it), the same for upper and lower case,
    A/C/G/T distinct, bytes beyond the t-th without influence;
  * murmur3_core<K> with the table against the multiply form and against the oracle's hash for K = 17..21 and 25..29, on
    windows in upper, lower and mixed case that went through canonical_words, the 8-base strand ties among them;
  * K = 16, 22, 24, 32 have no table and hash as they did."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests.test_canonical_words import GROUP, chunk_with, revcomp, windows_for

M64 = (1 << 64) - 1
C1, C2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
LETTERS = b"ACTG"                      # digit -> base: bits 1..2 of the ASCII byte
LUT_KS = [17, 18, 19, 20, 21, 25, 26, 27, 28, 29]
PLAIN_KS = [16, 22, 24, 32]


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("tail_lut_emul")
    L.emul_tail_lut_entries.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.emul_tail_lut_index.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.emul_tail_lut_applies.argtypes = [ctypes.c_int]
    L.emul_tail_hashes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def rotl(x: int, r: int) -> int:
    return ((x << r) | (x >> (64 - r))) & M64


def formula(second: bool, x: int) -> int:
    if second:
        return (rotl((x * C2) & M64, 33) * C1) & M64
    return (rotl((x * C1) & M64, 31) * C2) & M64


def index_of(emul, t: int, words: np.ndarray) -> np.ndarray:
    """words: n x 8 bytes, the partial word little-endian"""
    w = np.ascontiguousarray(words, dtype=np.uint8).view(np.uint32).reshape(-1, 2)
    lo, hi = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    out = np.zeros(len(lo), dtype=np.uint32)
    assert emul.emul_tail_lut_index(t, lo.ctypes.data, hi.ctypes.data, len(lo), out.ctypes.data) == 0
    return out


def test_bits_1_and_2_tell_the_bases_apart():
    for digit, base in enumerate(LETTERS):
        assert (base >> 1) & 3 == digit and ((base | 0x20) >> 1) & 3 == digit


@pytest.mark.parametrize("second", [False, True], ids=["k1", "k2"])
@pytest.mark.parametrize("t", range(1, 6))
def test_every_entry_is_the_formula(emul, t, second):
    got = np.zeros(1024, dtype=np.uint64)
    n = emul.emul_tail_lut_entries(t, int(second), got.ctypes.data)
    assert n == 4 ** t
    for i in range(n):
        word = bytes(LETTERS[(i >> (2 * j)) & 3] for j in range(t))
        assert int(got[i]) == formula(second, int.from_bytes(word, "little")), (t, second, i)
        # and the index of those very bases is i
    words = np.zeros((n, 8), dtype=np.uint8)
    for i in range(n):
        words[i, :t] = [LETTERS[(i >> (2 * j)) & 3] for j in range(t)]
    assert np.array_equal(index_of(emul, t, words), np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("t", range(1, 6))
def test_index_for_every_byte_value_in_every_position(emul, t):
    rng = np.random.default_rng(5100 + t)
    every = np.arange(256, dtype=np.uint8)
    for pos in range(8):
        for trial in range(8):
            # the other seven bytes: anything at all (newlines, quality characters, N, bytes beyond the t-th)
            words = np.tile(rng.integers(0, 256, size=8, dtype=np.uint8), (256, 1))
            if trial == 0:
                words[:] = 0xFF
            words[:, pos] = every
            idx = index_of(emul, t, words)
            assert idx.max() < 4 ** t, "the load must stay inside the table"
            folded = words.copy()
            folded[:, pos] ^= 0x20
            assert np.array_equal(index_of(emul, t, folded), idx), "case must not show"
            if pos < t:
                # this byte's digit is bits 1..2 of the byte, the other digits do not move
                assert np.array_equal((idx >> (2 * pos)) & 3, (every.astype(np.uint32) >> 1) & 3)
                assert len(set((idx & ~np.uint32(3 << (2 * pos))).tolist())) == 1
                four = [int(idx[b]) for b in b"ACGT"]
                assert len(set(four)) == 4
            else:
                assert len(set(idx.tolist())) == 1, "a byte beyond the t-th must not show"


def hashes(emul, k: int, j: int, windows, rng):
    nd = (GROUP + k - 1 + 3) // 4
    chunks = b"".join(chunk_with(rng, w, j, 4 * nd, i) for i, w in enumerate(windows))
    buf = np.frombuffer(chunks, np.uint8).copy().view(np.uint32)
    mul = np.zeros(len(windows), dtype=np.uint64)
    lut = np.zeros(len(windows), dtype=np.uint64)
    assert emul.emul_tail_hashes(k, j, buf.ctypes.data, len(windows), mul.ctypes.data, lut.ctypes.data) == 0
    return mul, lut


@pytest.mark.parametrize("k", LUT_KS)
def test_table_form_is_the_multiply_form_and_the_oracles_hash(emul, k):
    assert emul.emul_tail_lut_applies(k) == 1
    lib = mo.lib()
    for j in range(GROUP):
        rng = np.random.default_rng(5200 + 8 * k + j)
        windows = windows_for(rng, k)      # upper case; chunk_with puts every third in lower, every third in mixed case
        assert sum(1 for w in windows if w[:8] == revcomp(w)[:8]) >= 24, "windows whose first 8 bases tie between the strands"
        mul, lut = hashes(emul, k, j, windows, rng)
        assert np.array_equal(lut, mul)
        for i, w in enumerate(windows):
            assert int(lut[i]) == lib.mo_kmer_hash(min(w, revcomp(w)), k, 42), f"k={k} j={j} window {w!r}"


@pytest.mark.parametrize("k", PLAIN_KS)
def test_k_without_a_table_hashes_as_it_did(emul, k):
    assert emul.emul_tail_lut_applies(k) == 0
    lib = mo.lib()
    rng = np.random.default_rng(5300 + k)
    windows = windows_for(rng, k)
    mul, _ = hashes(emul, k, 3, windows, rng)
    for i, w in enumerate(windows):
        want = lib.mo_kmer_hash(min(w, revcomp(w)), k, 42)
        assert (int(mul[i]) if k > 16 else int(mul[i]) & 0xFFFFFFFF) == want, f"k={k} window {w!r}"


def test_which_k_have_a_table(emul):
    assert [k for k in range(1, 33) if emul.emul_tail_lut_applies(k) == 1] == LUT_KS

"""The tail table's offset from digits packed once per group (TailDigits<K>, auriclass_amd/csrc/mhx_tile.h) on the CPU
(tests/emul/tail_digits_emul.cpp), for every K with a table (17..21, 25..29) and every window J = 0..7 of a group.

  * offsets: the packed route's byte offset, with either strand forced, is 8 x tail_lut_index of that strand's own
    partial word, and for the strand canonical_words takes it is 8 x tail_lut_index of the partial word canonical_words
    (multiply form) yields -- on chunks of bases in upper, lower and mixed case, and with each of the 256 byte values at
    every position of the chunk (the hot loop hashes windows over headers, qualities, newlines, N and halo bytes as
    well); every offset lies inside the table;
  * hashes: the hot loop's window in the packed form (body words only, the entry at the packed offset) gives the hash of
    the multiply form and the oracle's hash of min(forward, reverse complement), strand ties on the first 8 bases
    included."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests.test_canonical_words import ACGT, GROUP, chunk_with, revcomp, windows_for

LUT_KS = [17, 18, 19, 20, 21, 25, 26, 27, 28, 29]


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("tail_digits_emul")
    L.emul_tail_digits_apply.argtypes = [ctypes.c_int]
    L.emul_tail_digit_offsets.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.emul_tail_digit_hashes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def chunk_bytes(k: int) -> int:
    return 4 * ((GROUP + k - 1 + 3) // 4)


def offsets(emul, k: int, j: int, chunks: np.ndarray) -> np.ndarray:
    """chunks: n x chunk_bytes(k) bytes -> n x 6 (see offsets<K, J> in the emulator)"""
    buf = np.ascontiguousarray(chunks, dtype=np.uint8)
    assert buf.shape[1] == chunk_bytes(k)
    out = np.zeros((len(buf), 6), dtype=np.uint32)
    assert emul.emul_tail_digit_offsets(k, j, buf.ctypes.data, len(buf), out.ctypes.data) == 0
    return out


def check_offsets(o: np.ndarray, k: int, what: str) -> None:
    t = k % 8
    assert np.array_equal(o[:, 0], o[:, 2]), f"{what}: forward strand forced"
    assert np.array_equal(o[:, 1], o[:, 3]), f"{what}: reverse strand forced"
    assert np.array_equal(np.where(o[:, 4] == 1, o[:, 1], o[:, 0]), o[:, 5]), f"{what}: the canonical strand"
    assert o[:, :2].max() < 8 * 4 ** t and np.all(o[:, :2] % 8 == 0), f"{what}: the load must stay inside the table"


def test_which_k_pack_their_digits(emul):
    # the device's hot loop packs at K = 21 alone (tail_digits_apply: the instruction counts and registers of the other K);
    # TailDigits<K> itself is checked below for every K with a table
    assert [k for k in range(1, 33) if emul.emul_tail_digits_apply(k) == 1] == [21]


@pytest.mark.parametrize("k", LUT_KS)
def test_offset_is_the_index_of_the_partial_word_on_bases(emul, k):
    nb = chunk_bytes(k)
    for j in range(GROUP):
        rng = np.random.default_rng(6100 + 8 * k + j)
        upper = rng.choice(ACGT, size=(512, nb))
        lower = upper | 0x20
        mixed = upper | (rng.integers(0, 2, size=upper.shape, dtype=np.uint8) << 5)
        for name, chunks in (("upper", upper), ("lower", lower), ("mixed", mixed)):
            o = offsets(emul, k, j, chunks)
            check_offsets(o, k, f"k={k} j={j} {name}")
            if name == "upper":
                want = o
                assert len(set(o[:, 0].tolist())) > min(4 ** (k % 8), 64) // 2 and len(set(o[:, 4].tolist())) == 2
            else:
                assert np.array_equal(o, want), "case must not show"


@pytest.mark.parametrize("k", LUT_KS)
def test_offset_for_every_byte_value_at_every_chunk_position(emul, k):
    nb = chunk_bytes(k)
    every = np.arange(256, dtype=np.uint8)
    for j in range(GROUP):
        rng = np.random.default_rng(6200 + 8 * k + j)
        parts = []
        for style in range(2):  # the other bytes: bases, or anything at all
            base = rng.choice(ACGT, size=nb) if style == 0 else rng.integers(0, 256, size=nb, dtype=np.uint8)
            for pos in range(nb):
                c = np.tile(base, (256, 1))
                c[:, pos] = every
                parts.append(c)
        parts.append(np.full((1, nb), 0xFF, dtype=np.uint8))
        parts.append(np.zeros((1, nb), dtype=np.uint8))
        check_offsets(offsets(emul, k, j, np.concatenate(parts)), k, f"k={k} j={j}")


@pytest.mark.parametrize("k", LUT_KS)
def test_packed_form_hashes_like_the_multiply_form_and_the_oracle(emul, k):
    lib = mo.lib()
    nb = chunk_bytes(k)
    for j in range(GROUP):
        rng = np.random.default_rng(6300 + 8 * k + j)
        windows = windows_for(rng, k)  # upper case; chunk_with puts every third in lower, every third in mixed case
        assert sum(1 for w in windows if w[:8] == revcomp(w)[:8]) >= 24, "windows whose first 8 bases tie between the strands"
        chunks = b"".join(chunk_with(rng, w, j, nb, i) for i, w in enumerate(windows))
        buf = np.frombuffer(chunks, np.uint8).copy()
        packed = np.zeros(len(windows), dtype=np.uint64)
        mul = np.zeros(len(windows), dtype=np.uint64)
        assert emul.emul_tail_digit_hashes(k, j, buf.ctypes.data, len(windows), packed.ctypes.data, mul.ctypes.data) == 0
        assert np.array_equal(packed, mul)
        for i, w in enumerate(windows):
            assert int(packed[i]) == lib.mo_kmer_hash(min(w, revcomp(w)), k, 42), f"k={k} j={j} window {w!r}"

"""canonical_words<K, J, ND> of the sketch kernel's hash loop on the CPU (tests/emul/canonical_words_emul.cpp): for every
K in 8..32 and every window J in 0..7 of a group, the words it hands to the hash must be the K bytes of
min(forward, reverse complement) of the upper-cased window, zero-padded, and murmur3_h1<K> of them the oracle's hash.
The function selects only the source dwords a strand's kept bytes come from, by a rule that depends on K and J, so no
(K, J) is left out; the bytes of the chunk around the window are arbitrary and must not show."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build

GROUP = 8
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("canonical_words_emul")
    L.emul_chunk_dwords.argtypes = [ctypes.c_int]
    L.emul_canonical_words.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def revcomp(w: bytes) -> bytes:
    return w.translate(COMP)[::-1]


def tie_window(rng, k: int, tied: int) -> bytes:
    """k bases whose first `tied` equal the first `tied` of the reverse complement (tied <= k; an odd k below 2 * tied
    has its middle base among them, which cannot equal its own complement: such a tie does not exist, None)."""
    w = bytearray(rng.choice(ACGT, size=k).tobytes())
    for i in range(tied):
        w[k - 1 - i] = bytes([w[i]]).translate(COMP)[0]
    w = bytes(w)
    if w[:tied] != revcomp(w)[:tied]:
        assert k % 2 == 1 and k < 2 * tied
        return None
    return w


def windows_for(rng, k: int):
    """Upper-case windows: random ones, ties of the first 8 bases between the strands (the kernel's fast strand test
    cannot decide those), longer ties, and windows that are their own reverse complement."""
    out = [bytes(rng.choice(ACGT, size=k)) for _ in range(160)]
    for tied in (8, min(k, 12), k // 2, k):
        for _ in range(24):
            w = tie_window(rng, k, tied)
            if w is not None:
                out.append(w)
    # a tie of exactly 8 bases, decided at the ninth, either way
    if k >= 18:
        for _ in range(24):
            w = bytearray(tie_window(rng, k, 8))
            w[8] = rng.choice(ACGT)
            out.append(bytes(w))
    out += [b"A" * k, b"T" * k, b"C" * k, b"G" * k, (b"AT" * k)[:k], (b"ACGT" * k)[:k], (b"TGCA" * k)[:k]]
    return out


def chunk_with(rng, window: bytes, j: int, nbytes: int, style: int) -> bytes:
    """The window at byte j of a chunk; what surrounds it: bases, or any bytes (newlines, N, quality characters)."""
    k = len(window)
    if style % 3 == 1:
        window = window.lower()
    elif style % 3 == 2:
        lower = rng.random(k) < 0.5
        window = bytes(b | 0x20 if lo else b for b, lo in zip(window, lower))
    around = rng.choice(ACGT, size=nbytes).tobytes() if style % 2 == 0 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes()
    return around[:j] + window + around[j + k:]


@pytest.mark.parametrize("j", range(GROUP))
@pytest.mark.parametrize("k", range(8, 33))
def test_words_and_hash_of_the_canonical_strand(emul, k, j):
    rng = np.random.default_rng(9000 + 8 * k + j)
    nd = emul.emul_chunk_dwords(k)
    assert nd == (GROUP + k - 1 + 3) // 4
    windows = windows_for(rng, k)
    ties = sum(1 for w in windows if w[:8] == revcomp(w)[:8])
    assert ties >= 24 or (k % 2 == 1 and k < 16), "the input must hold windows whose first 8 bases tie between the strands"
    chunks = b"".join(chunk_with(rng, w, j, 4 * nd, i) for i, w in enumerate(windows))
    buf = np.frombuffer(chunks, np.uint8).copy().view(np.uint32)
    words = np.full(8 * len(windows), 0xA5A5A5A5, dtype=np.uint32)
    hashes = np.zeros(len(windows), dtype=np.uint64)
    assert emul.emul_canonical_words(k, j, buf.ctypes.data, len(windows), words.ctypes.data, hashes.ctypes.data) == 0
    got = words.view(np.uint8).reshape(len(windows), 32)
    lib = mo.lib()
    for i, w in enumerate(windows):
        canon = min(w, revcomp(w))
        assert got[i].tobytes() == canon + bytes(32 - k), f"k={k} j={j} window {w!r}: words {got[i].tobytes()!r}"
        want = lib.mo_kmer_hash(canon, k, 42)
        have = int(hashes[i]) if k > 16 else int(hashes[i]) & 0xFFFFFFFF
        assert have == want, f"k={k} j={j} window {w!r}"

"""The strand decision of the sketch kernel's hash loop from the two views the hash reads, on the CPU
(tests/emul/strand_views_emul.cpp): strand_views<ND>(src, U, R), canonical_strand<K, J, ND>(U, R), canonical_words on them in
both forms, PairWords' route and the table routes of the tail block, for every K in 8..32 and every window 0..7 of a group.

  * On windows of A/C/G/T in either case -- those of tests/test_canonical_words.py, ties of the first 8 bases of the two
    strands that the 9th .. K-th base decides either way, ties of every length up to the middle, palindromes -- the strand is
    memcmp(forward, reverse complement) > 0, the words are the four-view overload's and the K bytes of the smaller strand,
    and every route's hash is the oracle's.
  * No byte of the chunk outside the window shows: every value 0..255 at every position outside it leaves every output as
    it was.
  * A window that holds a byte other than A/C/G/T may decide either way -- the kernel throws its hash away -- so only what
    the kernel relies on is asserted: the call returns, the table offsets stay inside the table, window_is_acgt is false."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests.test_canonical_words import ACGT, GROUP, chunk_with, revcomp, tie_window, windows_for

KS = range(8, 33)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("strand_views_emul")
    L.emul_chunk_dwords.argtypes = [ctypes.c_int]
    L.emul_strand_views.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def run(emul, k: int, j: int, chunks: np.ndarray):
    """chunks: (n, 4 * nd) bytes -> (n, out dwords), (n, 3) hashes"""
    nd, no = emul.emul_chunk_dwords(k), emul.emul_out_dwords()
    assert nd == (GROUP + k - 1 + 3) // 4 and chunks.shape[1] == 4 * nd
    buf = np.ascontiguousarray(chunks, dtype=np.uint8).view(np.uint32)
    out = np.full((len(chunks), no), 0xA5A5A5A5, dtype=np.uint32)
    hashes = np.zeros((len(chunks), 3), dtype=np.uint64)
    assert emul.emul_strand_views(k, j, buf.ctypes.data, len(chunks), out.ctypes.data, hashes.ctypes.data) == 0
    return out, hashes


def decided_behind_the_tie(rng, k: int):
    """Windows whose strands tie on their first t bases, t = 8 .. the last length at which base t and its mirror image
    are two bases, and whose base t decides: once for the forward strand, once for the reverse complement."""
    out = []
    for t in range(8, (k - 1) // 2 + (k - 1) % 2):
        for base in (b"A", b"T"):   # w[t] = w[k-1-t] = 'A': the reverse complement has 'T' there, forward is smaller; 'T': the other way
            for _ in range(4):
                w = bytearray(tie_window(rng, k, t))
                w[t] = w[k - 1 - t] = base[0]
                w = bytes(w)
                assert w[:t] == revcomp(w)[:t] and (revcomp(w) < w) == (base == b"T")
                out.append(w)
    return out


def palindromes(rng, k: int):
    """windows that are their own reverse complement (even k only: the middle base of an odd k cannot be)"""
    out = []
    for _ in range(8 if k % 2 == 0 else 0):
        half = rng.choice(ACGT, size=k // 2).tobytes()
        out.append(half + revcomp(half))
        assert out[-1] == revcomp(out[-1])
    return out


def all_windows(rng, k: int):
    return windows_for(rng, k) + decided_behind_the_tie(rng, k) + palindromes(rng, k)


def as_chunks(rng, windows, j: int, nd: int) -> np.ndarray:
    return np.frombuffer(b"".join(chunk_with(rng, w, j, 4 * nd, i) for i, w in enumerate(windows)), np.uint8).reshape(len(windows), 4 * nd).copy()


@pytest.mark.parametrize("j", range(GROUP))
@pytest.mark.parametrize("k", KS)
def test_strand_words_and_hash_from_two_views(emul, k, j):
    rng = np.random.default_rng(9000 + 8 * k + j)       # the seeds of tests/test_canonical_words.py: its windows first
    nd = emul.emul_chunk_dwords(k)
    windows = all_windows(rng, k)
    if k >= 18:
        tied = [w for w in windows if w[:8] == revcomp(w)[:8] and w != revcomp(w)]
        assert sum(w < revcomp(w) for w in tied) >= 8 and sum(w > revcomp(w) for w in tied) >= 8, "ties broken in either direction"
    out, hashes = run(emul, k, j, as_chunks(rng, windows, j, nd))
    w2, w4, b2, b4, wp, bp = (out[:, 8 * i:8 * i + 8] for i in range(6))
    assert np.array_equal(w2, w4), "the words of the four-view overload"
    assert np.array_equal(b2, b4), "body-only words of the four-view overload"
    for col in (49, 50, 51):
        assert np.array_equal(out[:, 48], out[:, col]), f"strand, column {col}"
    assert out[:, 52].all(), "window_is_acgt"
    nbw = 2 * (k // 8) if k > 16 and k % 8 else 0
    assert np.array_equal(b2[:, :nbw], w2[:, :nbw]) and not b2[:, nbw:].any()
    if k > 16:
        assert np.array_equal(wp, w2), "PairWords, all dwords"
        assert np.array_equal(bp, b2), "PairWords, body dwords"
    got = np.ascontiguousarray(w2).view(np.uint8).reshape(len(windows), 32)
    lib = mo.lib()
    mask = (1 << 64) - 1 if k > 16 else 0xFFFFFFFF
    for i, w in enumerate(windows):
        rc = revcomp(w)
        assert out[i, 48] == (rc < w), f"k={k} j={j} window {w!r}: strand"
        canon = min(w, rc)
        assert got[i].tobytes() == canon + bytes(32 - k), f"k={k} j={j} window {w!r}: words {got[i].tobytes()!r}"
        want = lib.mo_kmer_hash(canon, k, 42)
        assert [int(h) & mask for h in hashes[i]] == [want] * 3, f"k={k} j={j} window {w!r}"
    if out[0, 55]:      # a K with a table: both routes name the same entry
        assert np.array_equal(out[:, 53], out[:, 54])


@pytest.mark.parametrize("j", range(GROUP))
@pytest.mark.parametrize("k", KS)
def test_no_byte_outside_the_window_shows(emul, k, j):
    rng = np.random.default_rng(19000 + 8 * k + j)
    nd = emul.emul_chunk_dwords(k)
    pal = palindromes(rng, k)[:1]
    windows = [bytes(rng.choice(ACGT, size=k)), tie_window(rng, k, 8) or bytes(rng.choice(ACGT, size=k))] + decided_behind_the_tie(rng, k)[:2] + pal
    clean = as_chunks(rng, windows, j, nd)
    outside = [p for p in range(4 * nd) if not j <= p < j + k]
    assert (j == 0 or j - 1 in outside) and (j + k == 4 * nd or j + k in outside), "the positions next to the window"
    want_out, want_h = run(emul, k, j, clean)
    values = np.arange(256, dtype=np.uint8)
    for p in outside:
        chunks = np.repeat(clean, 256, axis=0)                    # window i, value v at row 256 i + v
        chunks[:, p] = np.tile(values, len(windows))
        out, hashes = run(emul, k, j, chunks)
        assert np.array_equal(out, np.repeat(want_out, 256, axis=0)), f"k={k} j={j}: byte {p} shows"
        assert np.array_equal(hashes, np.repeat(want_h, 256, axis=0)), f"k={k} j={j}: byte {p} shows in a hash"


NOT_A_BASE = np.array([v for v in range(256) if bytes([v]) not in b"ACGTacgt"], dtype=np.uint8)


@pytest.mark.parametrize("j", range(GROUP))
@pytest.mark.parametrize("k", KS)
def test_a_window_with_another_byte_is_harmless(emul, k, j):
    rng = np.random.default_rng(29000 + 8 * k + j)
    nd = emul.emul_chunk_dwords(k)
    windows = [bytes(rng.choice(ACGT, size=k)), tie_window(rng, k, 8) or bytes(rng.choice(ACGT, size=k))]
    clean = as_chunks(rng, windows, j, nd)
    for p in range(j, j + k):
        chunks = np.repeat(clean, len(NOT_A_BASE), axis=0)
        chunks[:, p] = np.tile(NOT_A_BASE, len(windows))
        out, _ = run(emul, k, j, chunks)                            # returns
        assert not out[:, 52].any(), f"k={k} j={j}: window_is_acgt with another byte at {p}"
        assert (out[:, 48] <= 1).all() and np.array_equal(out[:, 48], out[:, 49])
        table = int(out[0, 55])
        if table:
            for col in (53, 54):
                assert (out[:, col] < table).all() and (out[:, col] % 8 == 0).all(), f"k={k} j={j}: table offset, column {col}"

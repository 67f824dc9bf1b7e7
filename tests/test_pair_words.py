"""PairWords<K, J, ND> of the sketch kernel's hash loop on the CPU (tests/emul/pair_words_emul.cpp): the words of windows
J and J + 4 of a group from one funnel shift per strand.  For every K in 17..32 (the switch names a few of them; the
struct serves them all) and every window 0..7, on the inputs of tests/test_canonical_words.py -- upper-, lower- and
mixed-case chunks, arbitrary bytes around the window, strand ties on the first 8 bases broken either way -- the words
must be canonical_words<K, J, ND>'s, in both forms (all dwords; the full 8-byte words in front of the partial word),
the K bytes of min(forward, reverse complement), and their hash the oracle's.  And the switch must be the documented one."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests.test_canonical_words import GROUP, chunk_with, revcomp, windows_for

KS = range(17, 33)
# which kernel forms (FMT, QUEUE) of which K take the pair route
ALL_BUT_INLINE_REPAIR = {(0, 0), (0, 1), (2, 0), (2, 1), (1, 1)}   # every form but the inline ones of the look-back repair kernel
QUEUE_FORMS = {(0, 1), (1, 1), (2, 1)}
PAIR_FORMS = {17: ALL_BUT_INLINE_REPAIR, 18: ALL_BUT_INLINE_REPAIR, 19: ALL_BUT_INLINE_REPAIR, 21: ALL_BUT_INLINE_REPAIR,
              23: ALL_BUT_INLINE_REPAIR, 25: QUEUE_FORMS, 26: QUEUE_FORMS, 27: QUEUE_FORMS, 29: QUEUE_FORMS}


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("pair_words_emul")
    L.emul_chunk_dwords.argtypes = [ctypes.c_int]
    L.emul_pair_words.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_pair_words_form.argtypes = [ctypes.c_int] * 3
    return L


@pytest.mark.parametrize("j", range(GROUP))
@pytest.mark.parametrize("k", KS)
def test_pair_words_are_canonical_words(emul, k, j):
    rng = np.random.default_rng(9000 + 8 * k + j)       # the seeds of tests/test_canonical_words.py: the same windows
    nd = emul.emul_chunk_dwords(k)
    assert nd == (GROUP + k - 1 + 3) // 4
    windows = windows_for(rng, k)
    tied = [w for w in windows if w[:8] == revcomp(w)[:8] and w != revcomp(w)]
    assert sum(w < revcomp(w) for w in tied) >= 8 and sum(w > revcomp(w) for w in tied) >= 8, "ties broken in either direction"
    chunks = b"".join(chunk_with(rng, w, j, 4 * nd, i) for i, w in enumerate(windows))
    buf = np.frombuffer(chunks, np.uint8).copy().view(np.uint32)
    out = np.full(34 * len(windows), 0xA5A5A5A5, dtype=np.uint32)
    hashes = np.zeros(len(windows), dtype=np.uint64)
    assert emul.emul_pair_words(k, j, buf.ctypes.data, len(windows), out.ctypes.data, hashes.ctypes.data) == 0
    out = out.reshape(len(windows), 34)
    pair, canon_w, body, canon_body = (out[:, 8 * i:8 * i + 8] for i in range(4))
    assert np.array_equal(pair, canon_w), f"k={k} j={j}: all dwords"
    assert np.array_equal(body, canon_body), f"k={k} j={j}: body dwords"
    assert np.array_equal(out[:, 32], out[:, 33])
    nbw = 2 * (k // 8) if k % 8 else 0
    assert np.array_equal(body[:, :nbw], pair[:, :nbw]) and not body[:, nbw:].any()
    got = np.ascontiguousarray(pair).view(np.uint8).reshape(len(windows), 32)
    lib = mo.lib()
    for i, w in enumerate(windows):
        canon = min(w, revcomp(w))
        assert got[i].tobytes() == canon + bytes(32 - k), f"k={k} j={j} window {w!r}: words {got[i].tobytes()!r}"
        assert out[i, 32] == (revcomp(w) < w), f"k={k} j={j} window {w!r}: strand"
        assert int(hashes[i]) == lib.mo_kmer_hash(canon, k, 42), f"k={k} j={j} window {w!r}"


def test_the_switch_is_the_documented_one(emul):
    for k in range(1, 33):
        for fmt in (0, 1, 2):
            for queue in (0, 1):
                want = (fmt, queue) in PAIR_FORMS.get(k, ())
                assert emul.emul_pair_words_form(k, fmt, queue) == int(want), (k, fmt, queue)

"""Shapes for the segmented sketch (mhx_sketch_segments), shared by the CPU emulation test and the GPU test, and what the
oracle says about each: the definition-level sketch (oracle.mash_oracle.bruteforce_sketch) of every segment on its own.
A case is (stream bytes, ascending offsets); the expectation is computed once per (case, k) and truncated per s."""
import functools

import numpy as np

from oracle import mash_oracle as mo

KS = (3, 16, 17, 21, 27, 32)
SS = (1, 16, 1000)
CASES = ("edge_lengths", "touching", "many", "repeats", "dirty")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def dna(rng, n: int) -> bytes:
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def revcomp(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def join(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return b"".join(parts), off


@functools.lru_cache(maxsize=None)
def case(name: str, k: int, cut: int):
    """(stream, offsets).  Nothing stands between two segments: where the last bytes of one and the first of the next are
    A/C/G/T they would form windows, which belong to neither."""
    rng = np.random.default_rng([sum(name.encode()), k])
    if name == "edge_lengths":   # 0, k - 1, k, k + 1, around a wave, and cut - 1 / cut / cut + 1 windows (both routes and the seam)
        lengths = [0, k - 1, k, k + 1, 63, 64, 65, 0, cut + k - 2, cut + k - 1, cut + k, 1]
        return join([dna(rng, n) for n in lengths])
    if name == "touching":       # one sequence cut at odd places: every cut has valid windows across it
        seq = dna(rng, 3000)
        cuts = [0, 1, 2, 5, 5 + k, 100, 101, 777, 1500, 1501 + k, 2999, 3000]
        return seq, np.array(cuts, dtype=np.uint64)
    if name == "many":           # 5 000 segments of 30..300 bytes
        return join([dna(rng, int(n)) for n in rng.integers(30, 301, size=5000)])
    if name == "repeats":        # a tandem repeat (few distinct windows, each many times) and reverse palindromes (equal strands)
        unit = dna(rng, 7)
        half = dna(rng, 150)
        return join([unit * 120, half + revcomp(half), b"A" * 200, b"AT" * 100, (b"ACGT" * 64)[:k + 40], dna(rng, 90)])
    if name == "dirty":          # runs of N, lower case, a line break inside a segment
        a, b, c = dna(rng, 400), dna(rng, 300), dna(rng, 500)
        return join([a[:150] + b"N" * 40 + a[150:], b.lower(), c[:250] + b"\n" + c[250:], b"N" * 100, b"n" * (k + 3),
                     a[:60].lower() + b"NNN" + c[:80] + b"\r\n" + b[:70], dna(rng, k) + b"N", b"N" + dna(rng, k)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected_full(name: str, k: int, cut: int):
    """every distinct hash of every segment, ascending (the oracle's sketch with no size limit)"""
    data, off = case(name, k, cut)
    return [mo.bruteforce_sketch([data[int(off[i]):int(off[i + 1])]], k, 1 << 62)[0] for i in range(off.size - 1)]


def check_rows(rows, lens, name: str, k: int, s: int, cut: int, skip=()):
    """rows / lens against the oracle, exactly; skip: segment indices that the caller checks otherwise"""
    want = expected_full(name, k, cut)
    assert rows.shape[0] == lens.shape[0] == len(want)
    for i, full in enumerate(want):
        if i in skip:
            continue
        w = full[:s]
        assert int(lens[i]) == w.size, (name, k, s, i, int(lens[i]), w.size)
        assert np.array_equal(rows[i, :w.size], w), (name, k, s, i)

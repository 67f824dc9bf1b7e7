"""The two FASTQ good-map forms of the sketch kernel, compared on the CPU (tests/emul/tile_parse_emul.cpp): phase_good
with its per-newline loops is the reference, phase_events + phase_good_events is what the kernel runs on every tile whose
newlines fit the event list.  Per tile: every word of the good map, the bad-format flag, the number of long records.
Also: murmur3_h1<K> (seed folded into the first block's constant) against the oracle's hash for K = 1..32."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import synth
from oracle import mash_oracle as mo
from tests import emul_build

TILE = 16384
TILES, FALLBACK, GOOD_DIFF, BAD_DIFF, COUNT_DIFF, BAD_TILES, RECORDS, LINES = range(8)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("tile_parse_emul")
    L.emul_parse_compare.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    L.emul_mask_compare.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.emul_mask_compare.restype = ctypes.c_uint64
    L.emul_murmur3_h1.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return L


def compare(L, data: bytes, k=21, lead=0, cut=0, allow_fallback=False):
    """Both forms over the span [lead, lead + len(data) - cut) of a buffer that holds `lead` foreign bytes in front of
    the data and foreign bytes behind it.  Returns the emulator's counters after asserting that the forms agree -- and
    that the new form is what ran: a tile that takes the fallback is not compared at all (the emulator skips it), so
    unless the input is built to exceed the event list (allow_fallback) no tile may take it."""
    pad = 2 * TILE
    raw = np.zeros(lead + len(data) + pad + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    rng = np.random.default_rng(7)
    buf[:lead] = rng.choice(np.frombuffer(b"ACGT\n@+I", np.uint8), size=lead)
    buf[lead:lead + len(data)] = np.frombuffer(data, np.uint8)
    buf[lead + len(data):lead + len(data) + 48] = np.frombuffer(b"AC\nT" * 12, np.uint8)  # foreign tail, with newlines
    out = np.zeros(8, dtype=np.uint64)
    assert L.emul_parse_compare(buf.ctypes.data, lead, lead + len(data) - cut, k, out.ctypes.data) == 0
    out = [int(x) for x in out]
    assert out[GOOD_DIFF] == 0, f"good maps differ in {out[GOOD_DIFF]} of {out[TILES]} tiles"
    assert out[BAD_DIFF] == 0, f"bad-format flags differ in {out[BAD_DIFF]} of {out[TILES]} tiles"
    assert out[COUNT_DIFF] == 0, f"long-record counts differ in {out[COUNT_DIFF]} of {out[TILES]} tiles"
    if not allow_fallback:
        assert out[FALLBACK] == 0, f"{out[FALLBACK]} of {out[TILES]} tiles took the fallback: the new form was not compared there"
    return out


def random_reads(rng, n, lo, hi, p_n=0.2, p_lower=0.2):
    reads = []
    for _ in range(n):
        n_b = int(rng.integers(lo, hi + 1))
        r = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n_b)
        if n_b and rng.random() < p_n:
            for _ in range(int(rng.integers(1, 3))):
                r[int(rng.integers(0, n_b))] = ord("N")
        r = bytes(r)
        reads.append(r.lower() if rng.random() < p_lower else r)
    return reads


def fastq_bytes(rng, reads, header=lambda i: b"@r%d/1 x" % i, eol=b"\n", qual_first=None):
    alphabet = np.frombuffer(b"!#+@ACGTIJ5<?acgt", np.uint8)
    out = []
    for i, r in enumerate(reads):
        q = bytearray(rng.choice(alphabet, size=len(r)).tobytes())
        if q and qual_first is not None:
            q[0] = qual_first[i % len(qual_first)]
        out.append(header(i) + eol + r + eol + b"+" + eol + bytes(q) + eol)
    return b"".join(out)


def test_mask_by_bit_arithmetic_equals_the_loop(emul):
    rng = np.random.default_rng(1)
    dense = rng.integers(0, 2 ** 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    sparse = dense & rng.integers(0, 2 ** 32, size=100_000, dtype=np.uint64).astype(np.uint32) \
        & rng.integers(0, 2 ** 32, size=100_000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 1, 2, 3, 5, 0x80000000, 0xC0000000, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA, 0x00010001], np.uint32)
    words = np.ascontiguousarray(np.concatenate([dense, sparse, edge]))
    assert emul.emul_mask_compare(words.ctypes.data, len(words)) == 0


@pytest.mark.parametrize("k", [21, 27, 32])
def test_synthetic_reads(emul, k):
    genome = synth.make_genome(300_000, seed=42)
    fq = synth.make_fastq(genome, 2000, 150, seed=43, device="cpu").numpy().tobytes()
    out = compare(emul, fq, k)
    assert out[TILES] >= 38 and out[FALLBACK] == 0 and out[BAD_TILES] == 0
    assert out[LINES] == 4 * 2000 and out[RECORDS] == 2000


@pytest.mark.parametrize("k,lead", [(21, 0), (21, 37), (27, 5000), (16, 32768 + 11), (5, 1), (1, 16383)])
def test_ragged_reads_with_n_and_lower_case(emul, k, lead):
    rng = np.random.default_rng(200 + k + lead)
    reads = random_reads(rng, 900, 1, 400)
    out = compare(emul, fastq_bytes(rng, reads), k, lead=lead)
    assert out[FALLBACK] == 0 and out[BAD_TILES] == 0
    assert out[LINES] == 4 * len(reads)
    assert out[RECORDS] == sum(1 for r in reads if len(r) >= k)


@pytest.mark.parametrize("k", [21, 32])
def test_crlf(emul, k):
    rng = np.random.default_rng(300 + k)
    reads = random_reads(rng, 900, k - 3, k + 3, p_n=0.1)
    data = fastq_bytes(rng, reads, header=lambda i: b"@instrument:run:lane:tile:%d/1" % i, eol=b"\r\n")
    for cut in (0, 1):  # whole, and ending with a bare CR
        out = compare(emul, data, k, lead=5, cut=cut)
        assert out[FALLBACK] == 0 and out[BAD_TILES] == 0
        assert out[RECORDS] == sum(1 for r in reads if len(r) >= k)


def test_quality_lines_that_begin_with_at_and_plus(emul):
    rng = np.random.default_rng(4)
    reads = random_reads(rng, 1500, 1, 300)
    data = fastq_bytes(rng, reads, qual_first=b"@+@@+")
    out = compare(emul, data, 21, lead=77)
    assert out[FALLBACK] == 0 and out[BAD_TILES] == 0
    assert out[RECORDS] == sum(1 for r in reads if len(r) >= 21)


def test_headers_longer_than_a_word_and_longer_than_a_tile(emul):
    rng = np.random.default_rng(5)
    reads = random_reads(rng, 300, 30, 300)
    data = fastq_bytes(rng, reads, header=lambda i: b"@read%d " % i + b"x" * (40 + 13 * (i % 9)))
    out = compare(emul, data, 21)
    assert out[FALLBACK] == 0 and out[BAD_TILES] == 0 and out[RECORDS] == len(reads)
    reads = random_reads(rng, 12, 30, 300)
    data = fastq_bytes(rng, reads, header=lambda i: b"@h%d " % i + b"y" * (17000 + 4001 * (i % 3)))
    out = compare(emul, data, 21, lead=3)
    assert out[FALLBACK] == 0 and out[BAD_TILES] == 0 and out[RECORDS] == len(reads)


def test_reads_beyond_2700_bases(emul):
    """Lines too long for a tile to find its phase by itself (the look-back form of the kernel): the good map of a
    tile then hangs on the line count carried in from its predecessors alone."""
    rng = np.random.default_rng(6)
    reads = random_reads(rng, 40, 2800, 40000, p_n=0.5)
    for cut in (0, 1):
        out = compare(emul, fastq_bytes(rng, reads), 21, lead=3, cut=cut)
        assert out[FALLBACK] == 0 and out[BAD_TILES] == 0 and out[RECORDS] == len(reads)


@pytest.mark.parametrize("seed", range(12))
def test_damaged_records_flag_the_same_tiles(emul, seed):
    """Records cut short, '+' lines missing or overwritten, lines duplicated: both forms flag the same tiles (compare()
    asserts it) -- and a missing '+' is flagged at all."""
    rng = np.random.default_rng(4000 + seed)
    reads = random_reads(rng, 900, 20, 260)
    lines = fastq_bytes(rng, reads).split(b"\n")[:-1]
    for _ in range(int(rng.integers(1, 4))):
        i = int(rng.integers(0, len(lines)))
        what = int(rng.integers(0, 4))
        if what == 0:
            del lines[i]
        elif what == 1:
            lines.insert(i, lines[i])
        elif what == 2:
            lines[i] = lines[i][: len(lines[i]) // 2]
            del lines[i + 1: i + 1 + int(rng.integers(0, 3))]
        else:
            lines[i] = bytes(rng.choice(np.frombuffer(b"@+ACGT\n", np.uint8), size=max(1, len(lines[i]))))
    compare(emul, b"\n".join(lines) + b"\n", 21, lead=int(rng.integers(0, 20000)))
    good = fastq_bytes(rng, reads)
    out = compare(emul, good.replace(b"\n+\n", b"\n", 1), 21)
    assert out[BAD_TILES] > 0
    out = compare(emul, good.replace(b"\n+\n", b"\nX\n", 1), 21)
    assert out[BAD_TILES] > 0


@pytest.mark.parametrize("lead,length", [(5, 15), (16380, 20), (100, 21), (16383, 300), (7000, 3000), (16384 + 9, 16384),
                                         (31, 16353), (12345, 40000), (1, 2), (0, 1)])
def test_unaligned_and_short_spans(emul, lead, length):
    """Spans that begin and end anywhere inside a tile, some shorter than k: bytes outside the span are foreign (they
    hold newlines, '@' and '+') and must not show in the map, the flag or the count."""
    rng = np.random.default_rng(lead + length)
    reads = random_reads(rng, 400, 1, 200)
    data = fastq_bytes(rng, reads)[:length]
    out = compare(emul, data, 21, lead=lead)
    assert out[FALLBACK] == 0 and out[BAD_TILES] == 0


def test_three_base_reads_take_the_fallback(emul):
    """Records of 13 bytes: ~5000 newlines in a 16 KiB tile, five times what the event list holds, so phase_good itself is
    what the kernel runs there.  Every full tile takes it; the short last tile may fit the list."""
    rng = np.random.default_rng(13)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3)) for _ in range(20000)]
    data = b"".join(b"@r\n" + r + b"\n+\n" + b"III\n" for r in reads)
    out = compare(emul, data, 3, lead=5, allow_fallback=True)
    full_tiles = (5 + len(data)) // TILE
    print(f"fallback tiles: {out[FALLBACK]} of {out[TILES]}")
    assert full_tiles >= 15 and full_tiles <= out[FALLBACK] <= out[TILES]
    assert out[BAD_TILES] == 0 and out[RECORDS] == len(reads) and out[LINES] == 4 * len(reads)


def test_list_exactly_full_and_one_over(emul):
    """1024 newlines in a tile fit the list, 1025 do not: the choice is made per tile and either way the tile's
    result is phase_good's (records of 64 bytes: 256 of them, 1024 newlines, fill a tile)."""
    rec = b"@rr\n" + b"ACGT" * 7 + b"\n+\n" + b"I" * 28 + b"\n"
    assert len(rec) == 64
    data = rec * 300
    fits = compare(emul, data[:TILE], 3)
    assert fits[TILES] == 1 and fits[LINES] == 1024 and fits[FALLBACK] == 0
    over = compare(emul, b"@\n\n+\n\n" + data[: TILE - 6], 3, allow_fallback=True)
    assert over[TILES] == 1 and over[LINES] > 1024 and over[FALLBACK] == 1


@pytest.mark.parametrize("k", range(1, 33))
def test_hash_with_the_folded_seed_is_the_oracle_hash(emul, k):
    rng = np.random.default_rng(7000 + k)
    lib = mo.lib()
    for _ in range(200):
        window = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=k)) if rng.random() < 0.7 \
            else bytes(rng.integers(0, 256, size=k, dtype=np.uint8))
        w = np.zeros(8, dtype=np.uint32)
        w.view(np.uint8)[:k] = np.frombuffer(window, np.uint8)
        h = ctypes.c_uint64()
        assert emul.emul_murmur3_h1(k, w.ctypes.data, ctypes.byref(h)) == 0
        want = lib.mo_kmer_hash(window, k, 42)
        got = h.value if k > 16 else h.value & 0xFFFFFFFF
        assert got == want

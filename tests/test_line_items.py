"""The two ways the sketch kernel makes a FASTQ tile's work list, compared on the CPU (tests/emul/line_items_emul.cpp): the
map path (good map, run_starts, scan, compaction) is the reference; the line-item form (phase_line_span + phase_line_items,
mhx_tile.h) is what the kernel runs on interior tiles of ordinary reads.  Per tile: the set of listed groups, the start mask
of every listed group, the k-mer count, the long-record count, the bad-format flag -- and WHICH form the kernel's conditions
choose, which the cases below pin.  The inputs are crafted tiles: tile 0 of each buffer is interior (the span goes on for
more than a tile and its halo behind it) and begins in the line the case names."""
import ctypes

import numpy as np
import pytest

from tests import emul_build

TILE, HALO = 16384, 64
KS = [8, 16, 21, 27, 32]
TILES, BY_LINES, TOO_LONG, LIST_DIFF, MASK_DIFF, KMER_DIFF, CHECK_DIFF, KMERS, ITEMS, RECORDS = range(10)
MAPS, LINES, LATE = 0, 1, 2      # a tile's form: the maps, line items, line items tried and a line found too long


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("line_items_emul")
    L.emul_line_items_compare.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p]
    L.emul_line_items_bounds.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def bounds(emul):
    b = np.zeros(3, np.uint32)
    emul.emul_line_items_bounds(b.ctypes.data)
    max_lines, max_groups, min_newlines = (int(x) for x in b)
    assert (max_lines, max_groups, min_newlines) == (64, 40, 48)
    return max_lines, max_groups, min_newlines


def rule(data: bytes, k: int, first_line: int):
    """k-mers and long records of the whole span, line by line: a CR in front of the newline is a line byte for the k-mer
    starts and no base for the record's length; a record counts where its sequence line starts"""
    kmers = records = 0
    for i, line in enumerate(data.split(b"\n")):
        if (first_line + i) % 4 == 1:
            kmers += max(0, len(line) - k + 1)
            if i > 0:
                records += len(line[:-1] if line.endswith(b"\r") else line) >= k
    return kmers, records


def compare(L, data: bytes, k: int, first_line: int = 0):
    """both forms over the whole buffer; asserts that they agree wherever the line-item form runs; returns the counters and
    the form of every tile"""
    raw = np.zeros(len(data) + 2 * TILE + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    buf[len(data):len(data) + 48] = np.frombuffer(b"AC\nT" * 12, np.uint8)  # foreign tail, with newlines
    ntiles = (len(data) + TILE - 1) // TILE
    out, form = np.zeros(10, dtype=np.uint64), np.full(ntiles, 9, dtype=np.uint8)
    assert L.emul_line_items_compare(buf.ctypes.data, 0, len(data), first_line, k, out.ctypes.data, form.ctypes.data) == 0
    out = [int(x) for x in out]
    assert out[TILES] == ntiles
    for what in (LIST_DIFF, MASK_DIFF, KMER_DIFF, CHECK_DIFF):
        assert out[what] == 0, (what, out)
    assert (out[KMERS], out[RECORDS]) == rule(data, k, first_line)   # the checks' own yardstick: both sides of CHECK_DIFF run phase_event_checks
    assert form[-1] == MAPS                     # the last tile of a span is not interior
    return out, [int(f) for f in form]


GENOME = np.random.default_rng(5).choice(np.frombuffer(b"ACGT", np.uint8), size=6000)


def bases(rng, n):
    """n bases from a small genome (tests/test_gpu_line_items.py wants k-mers that occur more than once)"""
    if n > len(GENOME) // 2:
        return bytes(np.resize(GENOME, n))
    at = int(rng.integers(0, len(GENOME) - n + 1))
    return bytes(GENOME[at:at + n])


def record(rng, i, seq_len, hdr_len=11, eol=b"\n"):
    hdr = (b"@r%d " % i).ljust(hdr_len, b"x")[:max(hdr_len, 1)]
    return hdr + eol + bases(rng, seq_len) + eol + b"+" + eol + b"I" * seq_len + eol


def head_of(rng, first_line, seq_len=150):
    """the rest of the record a span begins in the middle of: its first line has index first_line"""
    r = record(rng, 0, seq_len).split(b"\n")
    return b"\n".join(r[first_line:])           # (ends with the newline of the quality line)


def fill(rng, data, upto, seq_len=150):
    i = 1000
    while len(data) < upto:
        data += record(rng, i, seq_len)
        i += 1
    return data


def tile_with_line(rng, k, first_line, start, nl_pos, total=2 * TILE + 3000):
    """ordinary 150-base records, among them one whose sequence line begins at byte `start` and ends with the newline at
    byte nl_pos"""
    data = head_of(rng, first_line) if first_line else b""
    i = 1
    while len(data) + 330 + 400 < start:
        data += record(rng, i, 150)
        i += 1
    hdr_len = start - len(data) - 1
    assert hdr_len >= 2
    seq_len = nl_pos - start
    data += b"@" + b"h" * (hdr_len - 1) + b"\n" + bases(rng, seq_len) + b"\n+\n" + b"I" * seq_len + b"\n"
    assert data[start - 1:start] == b"\n" and data[nl_pos:nl_pos + 1] == b"\n" and b"\n" not in data[start:nl_pos]
    return fill(rng, data, total)


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_ordinary_reads_take_the_line_items(emul, k, first_line):
    rng = np.random.default_rng(10 * k + first_line)
    data = fill(rng, head_of(rng, first_line) if first_line else b"", 3 * TILE + 500)
    out, form = compare(emul, data, k, first_line)
    assert form == [LINES, LINES, LINES, MAPS] and out[TOO_LONG] == 0


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_a_sequence_line_that_starts_in_the_last_bytes_of_a_tile(emul, k, first_line):
    rng = np.random.default_rng(100 * k + first_line)
    for start in (TILE - (k - 1), TILE - 1, TILE - k, TILE - k - 1, TILE):
        out, form = compare(emul, tile_with_line(rng, k, first_line, start, start + 150), k, first_line)
        assert form[0] == LINES, (start, form)


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_the_terminating_newline_around_the_tile_border_and_the_halo(emul, k, first_line):
    rng = np.random.default_rng(200 * k + first_line)
    start = TILE - k - 5
    for nl_pos in (TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 31, TILE + 32, TILE + HALO - 1, TILE + HALO, TILE + 200):
        out, form = compare(emul, tile_with_line(rng, k, first_line, start, nl_pos), k, first_line)
        assert form[0] == LINES, (nl_pos, form)
    # ... and with the line's start well inside the tile, so that the tile's last start is what the halo decides
    for nl_pos in (TILE + k - 2, TILE + k - 1, TILE + k):
        out, form = compare(emul, tile_with_line(rng, k, first_line, TILE - 100, nl_pos), k, first_line)
        assert form[0] == LINES, (nl_pos, form)


@pytest.mark.parametrize("k", KS)
def test_first_line_is_a_sequence_line_continued_from_the_tile_before(emul, k):
    rng = np.random.default_rng(300 + k)
    for rest in (0, 1, k - 1, k, k + 1, 150):      # what is left of that line in this tile
        data = fill(rng, bases(rng, rest) + b"\n+\n" + b"I" * 150 + b"\n", 2 * TILE + 3000)
        out, form = compare(emul, data, k, 1)
        assert form[0] == LINES


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_crlf(emul, k, first_line):
    rng = np.random.default_rng(400 * k + first_line)
    data = head_of(rng, first_line).replace(b"\n", b"\r\n") if first_line else b""
    i = 0
    while len(data) < 2 * TILE + 3000:
        data += record(rng, i, (k - 1, k, k + 1, 150)[i % 4], hdr_len=200, eol=b"\r\n")
        i += 1
    out, form = compare(emul, data, k, first_line)
    assert form[0] == LINES
    assert out[RECORDS] == rule(data, k, first_line)[1]


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_sequence_lines_of_length_0_and_around_k(emul, k, first_line):
    rng = np.random.default_rng(500 * k + first_line)
    data = head_of(rng, first_line) if first_line else b""
    i = 0
    while len(data) < 2 * TILE + 3000:
        data += record(rng, i, (0, k - 1, k, k + 1, 3 * k)[i % 5], hdr_len=260)     # long headers: under 64 records in a tile
        i += 1
    out, form = compare(emul, data, k, first_line)
    assert form[0] == LINES and form[1] == LINES
    assert out[RECORDS] == rule(data, k, first_line)[1]


@pytest.mark.parametrize("k", KS)
def test_64_65_and_257_sequence_lines_in_a_tile(emul, k, bounds):
    rng = np.random.default_rng(600 + k)

    def recs(size, n):
        seq = (size - 11 - 6) // 2
        data = b"".join(record(rng, i, seq, hdr_len=size - 2 * seq - 5) for i in range(n))
        assert len(data) == n * size
        return data

    out, form = compare(emul, recs(256, 64 * 2 + 20), k)     # 64 records fill a tile exactly
    assert form[:2] == [LINES, LINES]
    out, form = compare(emul, recs(252, 65 * 2 + 20), k)     # 65 sequence lines in tile 0
    assert form[0] == MAPS
    out, form = compare(emul, recs(63, 261 * 2 + 40), k)     # 260 records, 1040 newlines: beyond the event list as well
    assert form[0] == MAPS and form[1] == MAPS
    out, form = compare(emul, recs(64, 256 * 2 + 40), k)     # 256 records, 1024 newlines: the list holds them, the lanes do not
    assert form[0] == MAPS


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_one_line_above_the_bound_next_to_ordinary_ones(emul, k, first_line, bounds):
    rng = np.random.default_rng(700 * k + first_line)
    groups = bounds[1]
    # an aligned start and 8 * groups valid starts: exactly `groups` groups; one start more is one group more
    out, form = compare(emul, tile_with_line(rng, k, first_line, 8000, 8000 + 8 * groups + k - 1), k, first_line)
    assert form[0] == LINES and out[TOO_LONG] == 0
    out, form = compare(emul, tile_with_line(rng, k, first_line, 8000, 8000 + 8 * groups + k), k, first_line)
    assert form[0] == LATE and form[1] == LINES and out[TOO_LONG] == 1
    # the same number of starts off the grid takes a group more
    out, form = compare(emul, tile_with_line(rng, k, first_line, 8003, 8003 + 8 * groups + k - 1), k, first_line)
    assert form[0] == LATE
    # a line of 3000 bases, and one that runs through the whole next tile
    out, form = compare(emul, tile_with_line(rng, k, first_line, 5000, 8000), k, first_line)
    assert form[0] == LATE
    out, form = compare(emul, tile_with_line(rng, k, first_line, TILE - 400, 2 * TILE + 700, total=3 * TILE + 3000), k, first_line)
    assert form[0] == LATE and form[1] == MAPS      # tile 1 holds no newline at all


@pytest.mark.parametrize("k", KS)
def test_a_tile_without_any_newline_and_tiles_of_long_reads_keep_the_maps(emul, k, bounds):
    rng = np.random.default_rng(800 + k)
    data = b""
    i = 0
    while len(data) < 4 * TILE:
        data += record(rng, i, 10_000)
        i += 1
    out, form = compare(emul, data, k)
    assert set(form) == {MAPS} and out[TOO_LONG] == 0        # under 48 newlines: not even tried
    # 48 newlines in the tile try the lines, 47 keep the maps: 12 records of 1300 bytes and a header that runs on into the
    # next tile; without the first header line the span begins in a sequence line and the tile holds a newline less
    assert bounds[2] == 48
    data = b"".join(record(rng, i, 100, hdr_len=1095) for i in range(12)) + b"@" + b"h" * 2500
    data = fill(rng, data + b"\n" + bases(rng, 50) + b"\n+\n" + b"I" * 50 + b"\n", 2 * TILE + 3000)
    assert data[:TILE].count(b"\n") == 48 and data[1096:][:TILE].count(b"\n") == 47
    out, form = compare(emul, data, k)
    assert form[0] == LINES
    out, form = compare(emul, data[1096:], k, 1)
    assert form[0] == MAPS


def test_the_kernel_forms_that_have_the_path(emul):
    """line_items_form: the self-synchronising FASTQ kernels (FMT 2) of K >= 8, but for the queue forms of K = 29 (scratch);
    the sequence-stream kernels (FMT 0) and the look-back kernels (FMT 1) stay as they were"""
    for k in range(1, 33):
        for fmt in (0, 1, 2):
            for queue in (0, 1):
                want = fmt == 2 and k >= 8 and not (k == 29 and queue)
                assert emul.emul_line_items_form(k, fmt, queue) == int(want), (k, fmt, queue)


def test_below_k_8_every_tile_keeps_the_maps(emul):
    rng = np.random.default_rng(9)
    out, form = compare(emul, fill(rng, b"", 3 * TILE + 500), 7)
    assert set(form) == {MAPS}


@pytest.mark.parametrize("k", [21, 32])
def test_damaged_records_are_flagged_alike(emul, k):
    """compare() asserts that flag and long-record count agree; the damage must not move a tile off the line items"""
    rng = np.random.default_rng(1000 + k)
    good = fill(rng, b"", 2 * TILE + 3000)
    for bad in (good.replace(b"\n+\n", b"\nX\n", 3), good.replace(b"\n@r", b"\n#r", 2)):
        out, form = compare(emul, bad, k)
        assert form[0] == LINES

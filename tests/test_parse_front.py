"""The long-record count of the line path of the sketch kernel on the CPU (tests/emul/parse_front_emul.cpp).

On the line path the long records are counted from the ends of the sequence lines (phase_line_span, line_span_long_record,
mhx_tile.h) and no longer by seqline_is_long in phase_event_checks; the emulator runs both on the same crafted tiles and
compares the counts tile by tile.  The reference is seqline_is_long, summed over the newlines of the tile that start a
sequence line; the total is also held against the rule of tests/test_line_items.py."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import test_line_items as cpu

TILE, HALO = cpu.TILE, cpu.HALO
KS = [8, 21, 32]
TILES, BY_LINES, TOO_LONG, COUNT_DIFF, CHECK_DIFF, RECORDS, SPAN_RECORDS, LINE0 = range(8)


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("parse_front_emul")
    L.emul_parse_front_records.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    return L


# ---- the record rule ---------------------------------------------------------------------------------------------------------

def records(L, data: bytes, k: int, first_line: int = 0, begin: int = 0):
    """the span [begin, begin + len(data)) of a buffer; asserts that the span count, the checks and the rule agree"""
    raw = np.zeros(begin + len(data) + 2 * TILE + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:begin] = np.frombuffer((b"GT\n@" * (begin // 4 + 1))[:begin], np.uint8)         # foreign bytes in front, with newlines
    buf[begin:begin + len(data)] = np.frombuffer(data, np.uint8)
    buf[begin + len(data):begin + len(data) + 48] = np.frombuffer(b"AC\nT" * 12, np.uint8)  # ... and behind
    out = np.zeros(8, dtype=np.uint64)
    assert L.emul_parse_front_records(buf.ctypes.data, begin, begin + len(data), first_line, k, out.ctypes.data) == 0
    out = [int(x) for x in out]
    assert out[TILES] == (begin + len(data) + TILE - 1) // TILE - begin // TILE
    assert out[COUNT_DIFF] == 0 and out[CHECK_DIFF] == 0, out
    assert out[RECORDS] == cpu.rule(data, k, first_line)[1], out
    assert out[SPAN_RECORDS] <= out[RECORDS]
    return out


def cycle(rng, lens, hdr_len, eol=b"\n", upto=2 * TILE + 3000, first_line=0):
    data = (cpu.head_of(rng, first_line).replace(b"\n", eol) if first_line else b"")
    i = 0
    while len(data) < upto:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len, eol=eol)
        i += 1
    return data


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_sequence_lines_of_k_minus_1_k_and_k_plus_1_bytes(emul, k, first_line):
    rng = np.random.default_rng(11 * k + first_line)
    out = records(emul, cycle(rng, (k - 1, k, k + 1), 260, first_line=first_line), k, first_line)
    assert out[BY_LINES] == 2 and out[TOO_LONG] == 0 and out[SPAN_RECORDS] > 20


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_k_bases_and_k_minus_1_bases_in_front_of_a_cr(emul, k, first_line):
    rng = np.random.default_rng(13 * k + first_line)
    data = cycle(rng, (k, k - 1, k + 1, k - 2), 260, eol=b"\r\n", first_line=first_line)
    out = records(emul, data, k, first_line)
    assert out[BY_LINES] == 2 and out[SPAN_RECORDS] > 10
    # a line of k bytes whose last one is a CR does not count, one of k + 1 bytes does: half of the records
    n = sum(1 for i, ln in enumerate(data.split(b"\n")) if (first_line + i) % 4 == 1 and i > 0)
    assert abs(2 * out[RECORDS] - n) <= 2


@pytest.mark.parametrize("k", KS)
def test_a_line_that_starts_in_the_last_k_bytes_of_the_tile_and_ends_in_the_halo(emul, k):
    rng = np.random.default_rng(17 * k)
    for start in (TILE - k, TILE - (k - 1), TILE - 3, TILE - 1, TILE):
        for length in (k - 1, k, k + 1, 40):
            if start + length < TILE or start + length >= TILE + HALO:
                continue
            out = records(emul, cpu.tile_with_line(rng, k, 0, start, start + length), k)
            assert out[BY_LINES] == 2, (start, length, out)
        # K bases and a CR, and K - 1 bases and a CR, across the border
        for bases in (k - 1, k):
            data = bytearray(cpu.tile_with_line(rng, k, 0, start, start + bases + 1))
            data[start + bases] = 13
            out = records(emul, bytes(data), k)
            assert out[BY_LINES] == 2, (start, bases, out)


@pytest.mark.parametrize("k", KS)
def test_a_line_that_runs_beyond_the_halo(emul, k):
    rng = np.random.default_rng(19 * k)
    for start in (TILE - 100, TILE - k, TILE - 1, TILE):
        for nl_pos in (TILE + HALO - 1, TILE + HALO, TILE + HALO + 1, TILE + 200):
            out = records(emul, cpu.tile_with_line(rng, k, 0, start, nl_pos, total=3 * TILE + 3000), k)
            assert out[BY_LINES] == 3 and out[LINE0] >= 1, (start, nl_pos, out)   # tile 1 begins inside that line, or right behind it


@pytest.mark.parametrize("k", KS)
def test_line_0_continues_from_the_tile_in_front(emul, k):
    rng = np.random.default_rng(23 * k)
    # what is left of the line in the tile: nothing, less than K, K and more -- it was counted where it began, or not at all
    for rest in (0, 1, k - 1, k, k + 1, 150):
        data = cpu.tile_with_line(rng, k, 0, TILE - (150 - rest), TILE + rest, total=3 * TILE + 3000)
        out = records(emul, data, k)
        assert out[BY_LINES] == 3 and out[LINE0] >= 1, (rest, out)    # tile 1; tile 2 may begin in a sequence line as well
    # ... and a span that itself begins inside a sequence line
    for rest in (0, k - 1, k, 150):
        data = cpu.fill(rng, cpu.bases(rng, rest) + b"\n+\n" + b"I" * 150 + b"\n", 2 * TILE + 3000)
        out = records(emul, data, k, 1)
        assert out[BY_LINES] == 2 and out[LINE0] >= 1, (rest, out)


@pytest.mark.parametrize("k", KS)
def test_the_first_tile_of_a_span(emul, k):
    rng = np.random.default_rng(29 * k)
    data = cpu.fill(rng, b"", 2 * TILE + 3000)
    out = records(emul, data, k)                 # the span begins with the buffer
    assert out[BY_LINES] == 2 and out[LINE0] == 0
    out = records(emul, data, k, begin=TILE)     # ... at a tile border inside it: that tile is interior and begins a record
    assert out[BY_LINES] == 2 and out[TILES] == 3
    out = records(emul, data, k, begin=TILE + 16)  # ... inside a tile: not interior, the maps; the tile behind it takes the lines
    assert out[BY_LINES] == 1 and out[TILES] == 3
    # the first sequence line right behind a one-byte header: the earliest a counted line can start
    out = records(emul, b"@\n" + cpu.bases(rng, k) + b"\n+\n" + b"I" * k + b"\n" + data, k)
    assert out[BY_LINES] == 2


@pytest.mark.parametrize("first_line", range(4))
@pytest.mark.parametrize("k", KS)
def test_a_tile_that_falls_back_to_the_maps_has_its_records_counted_once(emul, k, first_line):
    rng = np.random.default_rng(31 * k + first_line)
    out = records(emul, cpu.tile_with_line(rng, k, first_line, 8000, 8000 + 8 * 40 + k - 1), k, first_line)
    assert out[TOO_LONG] == 0 and out[BY_LINES] == 2
    for start, nl_pos in ((8000, 8000 + 8 * 40 + k), (5000, 8000), (TILE - 400, TILE + 64)):
        out = records(emul, cpu.tile_with_line(rng, k, first_line, start, nl_pos), k, first_line)
        assert out[TOO_LONG] == 1 and out[BY_LINES] == 2, out
        # records() has compared the count of that tile, taken in front of the barrier, with the checks': nothing is added behind it

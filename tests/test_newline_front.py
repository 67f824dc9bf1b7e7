"""The two front pieces of the sketch kernel that work on fewer instructions, on the CPU (tests/emul/newline_front_emul.cpp).

newline_mask (mhx_tile.h) tests eight bytes at a time with one 64-bit add and gathers their flags with two chained 64-bit
multiply-adds; the reference is a byte loop.  The phase search reads the first six newline positions from the list
phase_events has written: four lanes test the four triples side by side where the first wave holds six newlines
(selfsync_triple, selfsync_phase; the emulator lets only that wave list its newlines in front of it, as the kernel does
without a barrier), thread 0 walks the complete list and the halo words otherwise (phase_selfsync_list).  The reference is
phase_selfsync on the same staged bytes."""
import ctypes

import numpy as np
import pytest

from tests import emul_build
from tests import test_line_items as cpu

TILE, HALO = cpu.TILE, cpu.HALO
MAP, TAKEN, LIST, WAVE0, TOTAL, ANY_LIST, WHOLE_LIST = range(7)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("newline_front_emul")
    L.emul_newline_mask.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.emul_pair_flags.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.emul_pair_flags.restype = ctypes.c_uint64
    L.emul_pair_gather.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.emul_pair_gather.restype = ctypes.c_uint32
    L.emul_selfsync.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return L


# ---- newline_mask ------------------------------------------------------------------------------------------------------------

def check_word(L, word: bytes) -> None:
    assert len(word) == 32
    buf = np.frombuffer(word, np.uint8).copy().view(np.uint32)
    out = np.zeros(3, np.uint32)
    L.emul_newline_mask(buf.ctypes.data, out.ctypes.data)
    want = sum(1 << i for i, c in enumerate(word) if c == 10)
    assert [int(x) for x in out] == [want] * 3, (word, [hex(int(x)) for x in out], hex(want))


@pytest.mark.parametrize("newline_share", [0.0, 0.3])
def test_every_byte_value_at_every_position(emul, newline_share):
    rng = np.random.default_rng(int(100 * newline_share))
    for pos in range(32):
        for value in range(256):
            word = rng.integers(0, 256, 32, dtype=np.uint8)
            word[rng.random(32) < newline_share] = 10
            word[pos] = value
            check_word(emul, bytes(word))


def test_all_256_flag_combinations_of_a_dword_pair(emul):
    rng = np.random.default_rng(1)
    others = np.frombuffer(bytes([0x00, 0x0B, 0x08, 0x1A, 0x4A, 0x7F, 0x80, 0x8A, 0x8B, 0xFF, 0x0D, 0x2B, 0x40]), np.uint8)
    for combo in range(256):
        pair = rng.choice(others, 8)
        for j in range(8):
            if (combo >> j) & 1:
                pair[j] = 10
        lo, hi = (int(x) for x in pair.view(np.uint32))
        flags = emul.emul_pair_flags(lo, hi)
        assert flags == sum(0x80 << (8 * j) for j in range(8) if (combo >> j) & 1), (combo, hex(flags))
        assert emul.emul_pair_gather(flags & 0xFFFFFFFF, flags >> 32) & 0xFF == combo
        for at in range(4):                                   # ... and as each of the four pairs of a word
            word = rng.choice(others, 32)
            word[8 * at:8 * at + 8] = pair
            check_word(emul, bytes(word))
    # the pure gather, on flag words that hold nothing but flags
    for combo in range(256):
        f = sum(0x80 << (8 * j) for j in range(8) if (combo >> j) & 1)
        assert emul.emul_pair_gather(f & 0xFFFFFFFF, f >> 32) & 0xFF == combo


def test_words_of_newlines_of_crlf_runs_and_of_bytes_above_0x7f(emul):
    check_word(emul, b"\n" * 32)
    check_word(emul, b"\r\n" * 16)
    check_word(emul, b"\n\r" * 16)
    check_word(emul, b"AC\r\n" * 8)
    check_word(emul, b"\r" * 32)
    for value in (0x80, 0x8A, 0x8B, 0x8D, 0xFF):
        check_word(emul, bytes([value]) * 32)
        check_word(emul, (bytes([value]) + b"\n") * 16)
        check_word(emul, (b"\n" + bytes([value])) * 16)
    rng = np.random.default_rng(2)
    for _ in range(200):
        check_word(emul, bytes(rng.choice(np.frombuffer(b"\n\x8a\x0b\xff", np.uint8), 32)))


# ---- the phase search from the newline list ----------------------------------------------------------------------------------

def selfsync(L, data: bytes, tile: int, begin: int = 0, end=None, limit: int = NONE):
    end = len(data) if end is None else end
    raw = np.zeros(len(data) + 2 * TILE + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    buf[len(data):len(data) + 48] = np.frombuffer(b"AC\nT" * 12, np.uint8)   # foreign tail, with newlines
    out = np.zeros(7, np.uint32)
    assert L.emul_selfsync(buf.ctypes.data, begin, end, tile, limit, out.ctypes.data) == 0
    out = [int(x) for x in out]
    if out[TAKEN]:
        assert out[LIST] == out[MAP], out           # the route the kernel takes gives the search's answer
    if out[ANY_LIST] != 9 and tile != begin // TILE:
        assert out[ANY_LIST] == out[MAP], out       # ... and so it would wherever the first wave lists six newlines
    if out[WHOLE_LIST] != 9 and tile != begin // TILE:
        assert out[WHOLE_LIST] == out[MAP], out     # thread 0's walk of the whole list (and the halo words): the same again
    return out


def true_phase(data: bytes, tile: int, first_line: int = 0) -> int:
    return (first_line + data[:tile * TILE].count(b"\n")) % 4


def pad_to(rng, data: bytes, target: int) -> bytes:
    """whole records up to byte `target` exactly"""
    data = cpu.fill(rng, data, target - 1000)
    hdr = target - len(data) - 305
    data += b"@" + b"p" * (hdr - 1) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    assert len(data) == target
    return data


@pytest.mark.parametrize("first_line", range(4))
def test_ordinary_reads_take_the_list(emul, first_line):
    rng = np.random.default_rng(first_line)
    data = cpu.fill(rng, cpu.head_of(rng, first_line) if first_line else b"", 3 * TILE + 500)
    for tile in (1, 2):
        out = selfsync(emul, data, tile)
        assert out[TAKEN] == 1 and out[LIST] == true_phase(data, tile, first_line) and out[WAVE0] >= 6


@pytest.mark.parametrize("quality_start", [b"@", b"+", b"@+", b"+@", b"@@"])
def test_quality_lines_that_start_with_at_or_plus(emul, quality_start):
    rng = np.random.default_rng(sum(quality_start))
    for shift in range(0, 340, 17):                 # the tile border falls into every line of a record
        data = b"@" + b"s" * shift + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + quality_start + b"I" * (150 - len(quality_start)) + b"\n"
        i = 0
        while len(data) < 2 * TILE + 3000:
            r = cpu.record(rng, i, 150).split(b"\n")
            r[3] = quality_start + r[3][len(quality_start):]
            data += b"\n".join(r)
            i += 1
        out = selfsync(emul, data, 1)
        assert out[TAKEN] == 1 and out[LIST] == true_phase(data, 1), (shift, out)
    # sequence lines that start like a quality line cannot exist, but a header of a single '@' and an empty sequence line can
    data = cpu.fill(rng, b"", TILE - 200) + b"@\n\n+\n\n" * 100
    data = cpu.fill(rng, data, 2 * TILE + 3000)
    selfsync(emul, data, 1)


def test_fewer_than_six_newlines(emul):
    rng = np.random.default_rng(7)
    data = cpu.fill(rng, b"", 3 * TILE + 500, seq_len=3000)
    for tile in (1, 2):
        out = selfsync(emul, data, tile)
        assert out[TAKEN] == 0 and out[WAVE0] < 6 and out[LIST] == 9 and out[WHOLE_LIST] == out[MAP]
    # six in the tile, but not in the first wave's 4 KiB: the search of the map finds them, the list is not asked
    data = pad_to(rng, b"", TILE) + b"@" + b"h" * 5000 + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    data = cpu.fill(rng, data, 2 * TILE + 3000)
    out = selfsync(emul, data, 1)
    assert out[TAKEN] == 0 and out[WAVE0] == 0 and out[TOTAL] >= 6 and out[MAP] == 0


@pytest.mark.parametrize("sixth_at", [4094, 4095, 4096, 4097])
def test_the_sixth_newline_at_the_end_of_the_first_wave(emul, sixth_at):
    rng = np.random.default_rng(sixth_at)
    data = pad_to(rng, b"", TILE) + cpu.record(rng, 1, 150)                # newlines 1..4
    hdr = sixth_at - 316 - 151
    data += b"@" + b"h" * (hdr - 1) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    data = cpu.fill(rng, data, 2 * TILE + 3000)
    where = [i - TILE for i in range(TILE, 2 * TILE) if data[i] == 10]
    assert where[5] == sixth_at
    out = selfsync(emul, data, 1)
    assert out[WAVE0] == (6 if sixth_at < 4096 else 5) and out[TAKEN] == (1 if sixth_at < 4096 else 0), out
    assert out[MAP] == 0                                                   # either route: the tile begins a record


@pytest.mark.parametrize("first_line", range(4))
def test_check_limit_cuts_each_of_the_three_positions(emul, first_line):
    rng = np.random.default_rng(40 + first_line)
    data = cpu.fill(rng, cpu.head_of(rng, first_line) if first_line else b"", 2 * TILE + 3000)
    where = [i - TILE for i in range(TILE, 2 * TILE) if data[i] == 10][:6]
    answers = set()
    for n in where:
        for d in (0, 1, 2, 3):
            # the search cut at an arbitrary place ...
            out = selfsync(emul, data, 1, limit=n + d)
            assert out[ANY_LIST] != 9
            answers.add(out[ANY_LIST])
            # ... and by the end of the span, which takes the newlines behind it out of the list as well
            out = selfsync(emul, data, 1, end=TILE + n + d)
            assert out[TAKEN] == (1 if out[WAVE0] >= 6 else 0)
    for limit in (0, 1, TILE + HALO):
        answers.add(selfsync(emul, data, 1, limit=limit)[ANY_LIST])
    assert answers == {4, true_phase(data, 1, first_line)}                 # cut in front of the '+': no answer; behind it: the phase


def test_a_tile_that_is_the_first_of_its_span(emul):
    rng = np.random.default_rng(9)
    data = cpu.fill(rng, b"", 3 * TILE + 500)
    for begin in (0, TILE, TILE + 16):
        out = selfsync(emul, data, begin // TILE, begin=begin)
        assert out[TAKEN] == 0 and out[MAP] == 0 and out[WAVE0] >= 6, out
        out = selfsync(emul, data, begin // TILE + 1, begin=begin)
        assert out[TAKEN] == 1


def test_random_lines_and_limits(emul):
    """lines of random lengths that start with '@', '+' or a base, in no order: whatever the first six newlines look like,
    the list gives the search's answer"""
    rng = np.random.default_rng(11)
    starts = np.frombuffer(b"@@@+++AC", np.uint8)
    taken = answers = 0
    for _ in range(300):
        lines = []
        while sum(map(len, lines)) < 2 * TILE + 200:
            n = int(rng.integers(0, 4)) if rng.random() < 0.3 else int(rng.integers(0, 900))
            lines.append(bytes(rng.choice(starts, 1)) * min(n, 1) + b"G" * max(n - 1, 0) + (b"\r\n" if rng.random() < 0.1 else b"\n"))
        data = b"".join(lines)
        limit = NONE if rng.random() < 0.5 else int(rng.integers(0, 4200))
        out = selfsync(emul, data, 1, limit=limit)
        taken += out[TAKEN]
        answers += out[ANY_LIST] in (0, 1, 2, 3)
    assert taken > 100 and answers > 10


def test_under_six_newlines_in_the_tile_and_the_rest_in_the_halo(emul):
    """a header that fills tile 0 and all but the end of tile 1, then short records, moved byte by byte across the border:
    of the first six newlines none to six lie in the tile, the rest in the two halo words"""
    rng = np.random.default_rng(60)
    in_tile = set()
    for shift in range(40):
        end_of_header = 2 * TILE - 25 + shift
        data = b"@" + b"h" * (end_of_header - 1) + b"\nACGT\n+\nIIII\n@b\nAC\n+\nII\n" + cpu.fill(rng, b"", 3000, seq_len=500)
        six = [i for i, c in enumerate(data) if c == 10][:6]
        assert six[0] == end_of_header and six[5] == end_of_header + 18 < 2 * TILE + HALO
        out = selfsync(emul, data, 1)
        assert out[TAKEN] == 0 and out[WAVE0] == 0 and out[WHOLE_LIST] == 0      # the fourth triple: the tile begins in a header
        in_tile.add(sum(i < 2 * TILE for i in six))
        for limit in (six[5] - TILE, six[5] - TILE + 1, six[5] - TILE + 2, six[3] - TILE + 1, TILE, TILE + HALO):
            out = selfsync(emul, data, 1, limit=limit)
            assert out[WHOLE_LIST] == (0 if limit > six[5] - TILE + 1 else 4), (shift, limit, out)
    assert in_tile == set(range(7))

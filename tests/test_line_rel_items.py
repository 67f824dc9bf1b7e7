"""The line-relative items of the sketch kernel on the CPU (tests/emul/line_rel_items_emul.cpp; phase_line_rel_items,
process_line_rel_item, the TAIL form of process_group_regs: mhx_tile.h).  A sequence line with n valid starts from byte a on
gives n >> 3 full items at a, a + 8, .. and, if n & 7 is not 0, one tail item behind them; all full items of a tile stand in
front of all its tails.  The map path (good map, run_starts, scan, compaction) is the reference of the windows; the aligned
items (phase_line_items + process_group) and the C oracle are the references of the hashes, with a threshold that admits every
hash.  The inputs are crafted tiles in the way of tests/test_line_items.py, whose builders they use."""
import ctypes

import numpy as np
import pytest

from oracle import mash_oracle as mo
from tests import emul_build
from tests import test_line_items as cpu

TILE = cpu.TILE
KS = [8, 16, 21, 27, 32]
(TILES, REL, TOO_LONG, WINDOW_DIFF, KMER_DIFF, ORDER_DIFF, BOUNDS_DIFF, FULL, TAILS, ALIGNED, MORE_ITEMS, HOT_TRIPS,
 TAIL_TRIPS, CHOSEN, OFFSET_DIFF) = range(15)
MAPS, LINES, LATE = 0, 1, 2      # a tile's form: the maps, line-relative items, the line path tried and a line found too long


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("line_rel_items_emul")
    L.emul_line_rel_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    L.emul_line_rel_form.argtypes = [ctypes.c_int] * 3
    return L


def run(L, data: bytes, k: int, first_line: int = 0, hashes: bool = False, queue: bool = False):
    """the writer next to the map path over the whole buffer, every property asserted; with hashes=True the whole path too:
    returns the counters, the form of every tile and the two hash lists (new items, aligned items)"""
    raw = np.zeros(len(data) + 2 * TILE + 64, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    buf[len(data):len(data) + 48] = np.frombuffer(b"AC\nT" * 12, np.uint8)  # foreign tail, with newlines
    ntiles = (len(data) + TILE - 1) // TILE
    out, form = np.zeros(15, dtype=np.uint64), np.full(ntiles, 9, dtype=np.uint8)
    cap = len(data) if hashes else 0
    h_new, h_ref, n2 = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(2, np.uint64)
    rc = L.emul_line_rel_run(buf.ctypes.data, 0, len(data), first_line, k, int(queue), out.ctypes.data, form.ctypes.data,
                             h_new.ctypes.data if hashes else None, h_ref.ctypes.data if hashes else None, cap, n2.ctypes.data)
    assert rc == 0
    out = [int(x) for x in out]
    assert out[TILES] == ntiles
    for what in (WINDOW_DIFF, KMER_DIFF, ORDER_DIFF, BOUNDS_DIFF, MORE_ITEMS, OFFSET_DIFF):
        assert out[what] == 0, (what, out)
    assert form[-1] == MAPS                     # the last tile of a span is not interior
    return out, [int(f) for f in form], h_new[:int(n2[0])], h_ref[:int(n2[1])]


def records(rng, lens, hdr_len, eol=b"\n", upto=2 * TILE + 3000):
    data, i = b"", 0
    while len(data) < upto:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len, eol=eol)
        i += 1
    return data


def sized(rng, size, n, hdr_len):
    """n records of `size` bytes each"""
    seq = (size - hdr_len - 5) // 2
    data = b"".join(cpu.record(rng, i, seq, hdr_len=size - 2 * seq - 5) for i in range(n))
    assert len(data) == n * size
    return data


def border(o_start, o_end):
    """a sequence line that begins o_start bytes behind a multiple of 8 in front of the border between tiles 0 and 1 and ends
    o_end bytes behind one beyond it: the last line of tile 0 and the first of tile 1, both interior"""
    return lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 104 + o_start, TILE + 64 + k + o_end, total=3 * TILE + 3000)


# name -> (builder(rng, k), the forms of the tiles in front of the last one; None: not pinned)
CASES = {
    # n & 7 = 0 .. 7: the lengths K + 127 .. K + 134 (K = 21: 148 .. 155)
    **{"n_mod_8_is_%d" % c: ((lambda c: lambda rng, k: records(rng, (k + 127 + c,), 11))(c), [LINES, LINES]) for c in range(8)},
    "one_window_lines": (lambda rng, k: records(rng, (k,), 300), [LINES, LINES]),                       # tails alone
    "lines_shorter_than_k": (lambda rng, k: records(rng, (k - 1, 0, 150, 3), 220), [LINES, LINES]),
    "crlf": (lambda rng, k: records(rng, (k - 1, k, k + 1, 150), 200, eol=b"\r\n"), [LINES, LINES]),
    **{"border_%d" % o: (border(o, 7 - o), [LINES, LINES, LINES]) for o in range(8)},
    "lines_64": (lambda rng, k: sized(rng, 256, 64 * 2 + 20, 11), [LINES, LINES]),
    "mixed_lengths": (lambda rng, k: records(rng, (150, 148, k, 101, 76, 250, k + 6, 151), 40), [LINES, LINES]),
    "above_the_length_bound": (lambda rng, k: cpu.tile_with_line(rng, k, 0, 8000, 8000 + 8 * 40 + k), [LATE, LINES]),
}


def case(name, k):
    build, forms = CASES[name]
    return build(np.random.default_rng(sum(name.encode()) + k), k), forms


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_items_are_the_valid_starts_each_once(emul, name, k):
    data, forms = case(name, k)
    out, form, _, _ = run(emul, data, k)
    assert form[:-1] == forms, (form, out)
    lines = [ln for ln in data[:(len(form) - 1) * TILE].split(b"\n")[1::4]]
    if name.startswith("n_mod_8_is_"):   # every whole line of the tiles on the path: n >> 3 full items, a tail iff n & 7
        c = int(name[-1])
        assert out[TAILS] > 0 if c else out[TAILS] <= 2 * out[REL], out       # (only the lines the tile border cuts)
        assert out[FULL] >= 16 * (len(lines) - 2 * len(form))
    if name == "one_window_lines":
        assert out[FULL] == 0 and out[TAILS] > 40, out
    assert out[FULL] + out[TAILS] <= out[ALIGNED]


@pytest.mark.parametrize("queue", [False, True], ids=["inline", "queue"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["n_mod_8_is_2", "n_mod_8_is_0", "one_window_lines", "crlf", "border_3", "lines_64", "mixed_lengths",
                                  "above_the_length_bound"])
def test_hashes_are_the_aligned_items_and_the_oracles(emul, name, k, queue):
    data, _ = case(name, k)
    out, form, h_new, h_ref = run(emul, data, k, hashes=True, queue=queue)
    assert LINES in form and out[HOT_TRIPS] + out[TAIL_TRIPS] > 0
    if name == "one_window_lines":
        assert out[TAIL_TRIPS] > 0 and out[HOT_TRIPS] == 0, out   # trips that begin among the tails: the TAIL body alone
    else:
        assert out[HOT_TRIPS] > 0, out   # (whether a tile's tails fill the rest of its last hot trip or need one of their own is arithmetic)
    if name in ("n_mod_8_is_2", "mixed_lengths", "crlf"):
        assert out[TAILS] > 0, out
    got, got_n = np.unique(h_new, return_counts=True)
    ref, ref_n = np.unique(h_ref, return_counts=True)
    assert np.array_equal(got, ref) and np.array_equal(got_n, ref_n)
    seqs = [ln[:-1] if ln.endswith(b"\r") else ln for ln in data.split(b"\n")[1::4]]
    want, want_n = mo.bruteforce_sketch(seqs, k, 1 << 62, 1)
    assert len(want) > 0 and np.array_equal(got, want) and np.array_equal(got_n, want_n)


def test_which_kernel_forms_take_the_items(emul):
    """line_rel_form: the forms that have the line path (line_items_form: FMT 2, K >= 8, not the queue forms of K = 29) but for
    those that took scratch with the two further loop bodies: the inline forms of K = 18, 23, 28, 30, 31, 32, the queue forms of K = 26"""
    for k in range(1, 33):
        for fmt in (0, 1, 2):
            for queue in (False, True):
                want = fmt == 2 and k >= 8 and not (k == 29 and queue) and not (k == 26 if queue else k in (18, 23, 28, 30, 31, 32))
                assert emul.emul_line_rel_form(k, fmt, queue) == int(want), (k, fmt, queue)


def test_the_choice_per_tile(emul):
    """line_rel_choose: the new items only where the full items alone fill fewer trips of 64 than the aligned groups"""
    emul.emul_line_rel_choose.argtypes = [ctypes.c_uint32] * 3
    for full, tails, extra, want in [(832, 52, 6, 1),     # 150-base reads at K = 21: 13 trips and a short one against 14
                                     (843, 0, 47, 0),     # 148-base reads: 14 trips either way, the aligned items stay
                                     (833, 52, 5, 0), (0, 60, 0, 1), (64, 0, 0, 0), (64, 0, 1, 1), (0, 0, 0, 0),
                                     (2048, 0, 0, 0), (1984, 64, 0, 1), (1900, 64, 64, 1)]:
        assert emul.emul_line_rel_choose(full, tails, extra) == want, (full, tails, extra)

"""The first launch of a fresh sketcher may run several workgroups per tile (HashArgs::split, sketch_tile_kernel<.., SPLIT>):
every one of them parses the tile, each hashes one slice of its work list, slice 0 speaks for the tile.  Whatever the
split, the sketch must be the oracle's and the counters -- k-mers, inserts, lines, records, flags, launches -- those of the
same input at MHX_FIRST_SPLIT=1; the device counts are exact multiplicities, so they equal the unsplit run's and are
never below the oracle's (mash's heap forgets the occurrences of a hash it has evicted in between)."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo

pytestmark = pytest.mark.gpu

TILE = 16384
RB = synth.record_bytes(150)
KSM = [(21, 1000, 1), (27, 1000, 3), (16, 1000, 1), (32, 64, 1)]
TILES = [1, 3, 33, 40]     # one tile; fewer tiles than slices; both sides of the 32-tile first chunk
COUNTERS = ("kmers", "inserts", "lines", "flags", "launches")


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


@lru_cache(maxsize=None)
def fastq(tiles: int) -> bytes:
    """150 bp reads that end inside tile number `tiles`, at ~12x coverage so that m = 3 has solid k-mers"""
    n_reads = (tiles * TILE - 100) // RB
    genome = synth.make_genome(max(400, n_reads * 150 // 12), seed=100 + tiles)
    return synth.make_fastq(genome, n_reads, 150, seed=200 + tiles, device="cpu").numpy().tobytes()


@lru_cache(maxsize=None)
def oracle_fastq(data: bytes, k, s, m):
    ref = mo.Sketcher(k, s, m)
    ref.add_fastx(data)
    return ref.finish()


def to_device(data: bytes, lead: int = 0):
    dev = torch.zeros(lead + len(data) + 64, dtype=torch.uint8, device="cuda")
    dev[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return dev


def sketch(dev, lead, spans, fmt, k, s, m, split):
    """Outcome of pushing dev[lead + a : lead + b] for (a, b) in spans with MHX_FIRST_SPLIT=split:
    (error code or 0, hashes, counts, counters + records)."""
    old = os.environ.get("MHX_FIRST_SPLIT")
    os.environ["MHX_FIRST_SPLIT"] = str(split)
    try:
        sk = engine.Sketcher(k, s, m, expected_bytes=0)
        for a, b in spans:
            sk.push_device(dev.data_ptr() + lead + a, b - a, fmt)
        sk.sync()
        st = sk.stats()
        counters = tuple(st[c] for c in COUNTERS) + (sk.record_count(),)
        try:
            h, c = sk.finish()
            out = (0, h.tobytes(), c.tobytes(), counters)
        except engine.EngineError as e:
            out = (e.code, b"", b"", counters)
        sk.close()
        return out
    finally:
        if old is None:
            del os.environ["MHX_FIRST_SPLIT"]
        else:
            os.environ["MHX_FIRST_SPLIT"] = old


_unsplit = {}


def unsplit(key, *args):
    """the MHX_FIRST_SPLIT=1 outcome of a case, computed once"""
    if key not in _unsplit:
        _unsplit[key] = sketch(*args, 1)
    return _unsplit[key]


def check(key, data, dev, lead, spans, fmt, k, s, m, split, want=None, accepted=True):
    got = sketch(dev, lead, spans, fmt, k, s, m, split)
    assert got == unsplit(key, dev, lead, spans, fmt, k, s, m), (key, split)
    if accepted:
        assert got[0] == 0, (key, got[0])
    if got[0] == 0 and want is not False:
        want_h, want_c = want if want is not None else oracle_fastq(data, k, s, m)
        assert np.array_equal(np.frombuffer(got[1], np.uint64), want_h), key
        assert np.all(np.frombuffer(got[2], np.uint32) >= want_c), key
    return got


@pytest.mark.parametrize("k,s,m", KSM)
@pytest.mark.parametrize("split", [2, 4, 8])
@pytest.mark.parametrize("tiles", TILES)
def test_split_first_launch_equals_oracle_and_unsplit_run(tiles, split, k, s, m):
    data = fastq(tiles)
    assert (len(data) + TILE - 1) // TILE == tiles
    dev = to_device(data)
    got = check(("fq", tiles, k, s, m), data, dev, 0, [(0, len(data))], engine.FMT_FASTQ4, k, s, m, split)
    assert got[3][2] == 4 * (len(data) // RB) and got[3][3] == 0             # lines, flags
    assert got[3][4] == (2 if tiles > 32 and m == 1 else 1)                  # launches: the first chunk is 32 tiles (m > 1: the first MiB)


def test_sequence_stream_every_group_a_work_item():
    data = fastq(33)
    k, s, m = 21, 1000, 1
    ref = mo.Sketcher(k, s, m)
    for line in data.split(b"\n"):
        ref.add_seq(line)
    got = check(("seq", 33), data, to_device(data), 0, [(0, len(data))], engine.FMT_SEQ, k, s, m, 8, want=ref.finish())
    assert got[3][3] == 0


def test_span_off_the_16_byte_grid_that_ends_mid_tile():
    data = fastq(33)[: 70 * RB]     # 22 050 bytes: the second tile is cut short
    dev = to_device(data, lead=7)
    for k, s, m in KSM[:2]:
        check(("lead", k, s, m), data, dev, 7, [(0, len(data))], engine.FMT_FASTQ4, k, s, m, 8)


def test_five_small_pushes_only_the_first_launch_splits():
    data = fastq(33)
    n = len(data) // RB
    cuts = [0, 60 * RB, 61 * RB, (n // 2) * RB, (n - 3) * RB, len(data)]    # the first push is two tiles
    spans = list(zip(cuts[:-1], cuts[1:]))
    dev = to_device(data)
    for k, s, m in KSM[:2]:
        got = check(("five", k, s, m), data, dev, 0, spans, engine.FMT_FASTQ4, k, s, m, 8)
        assert got[3][4] >= 5


def test_long_reads_take_the_repair_pass_which_never_splits():
    genome = synth.make_genome(30_000, seed=77)
    data = synth.make_fastq(genome, 55, 3000, seed=78, device="cpu").numpy().tobytes()      # ~20 tiles of 3 kb reads
    got = check(("long",), data, to_device(data), 0, [(0, len(data))], engine.FMT_FASTQ4, 21, 1000, 1, 8)
    assert got[3][4] >= 2 and got[3][3] == 0     # the repair pass ran: launches of its own


def test_record_cut_short_in_front_of_a_tile_border_is_flagged_alike():
    data = fastq(3)
    last = (TILE // RB) - 1                      # the last record that ends inside the first tile
    cut = data[: last * RB + 11 + 150 + 1] + data[(last + 1) * RB:]     # ... loses its '+' and quality lines
    dev = to_device(cut)
    got = check(("cut",), cut, dev, 0, [(0, len(cut))], engine.FMT_FASTQ4, 21, 1000, 1, 8, accepted=False)
    assert got[0] == engine.MHX_E_FORMAT and got[3][3] & 2


def test_work_list_shorter_than_one_slice():
    two = fastq(1)[: 2 * RB]                     # two reads: ~33 groups of eight windows, one slice holds 256
    check(("two",), two, to_device(two), 0, [(0, len(two))], engine.FMT_FASTQ4, 21, 1000, 1, 8)
    # a few reads, then nothing but newlines up to the third tile: whatever the parser makes of them, the split makes the same
    padded = fastq(1)[: 3 * RB] + b"\n" * (2 * TILE + 500)
    check(("padded",), padded, to_device(padded), 0, [(0, len(padded))], engine.FMT_FASTQ4, 21, 1000, 1, 8, want=False, accepted=False)

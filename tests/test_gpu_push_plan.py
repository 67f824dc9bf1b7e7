"""The launches of a push on the device against the schedule (auriclass_amd/csrc/mhx_push_plan.h): for pushes that end one
tile past a stage of the schedule -- 33 tiles, one past the 32-tile first chunk of m = 1; 65 tiles, one past the MiB that
m > 1 admits whole --, whole and in two parts, `launches` of the sketcher's statistics equals what the CPU emulator plans
for the same pushes and a literal taken from the library before the schedule moved into its header; the sketch is the
oracle's.  k = 21, s = 1000, 150 bp reads (no repair pass: every launch is the schedule's)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo
from tests import push_rule as pr
from tests.test_push_plan import emul, planned  # noqa: F401  (the emulator fixture and its row reader)

pytestmark = pytest.mark.gpu

TILE = pr.TILE
RB = synth.record_bytes(150)
K, S = 21, 1000
#        name           m  tiles  first part (tiles; None: whole)  format             launches
CASES = [("m1_whole",   1, 33,    None,                            engine.FMT_FASTQ4, 2),
         ("m1_20_13",   1, 33,    20,                              engine.FMT_FASTQ4, 2),
         ("m3_whole",   3, 65,    None,                            engine.FMT_FASTQ4, 2),
         ("m3_40_25",   3, 65,    40,                              engine.FMT_FASTQ4, 2),
         ("m1_seq",     1, 33,    None,                            engine.FMT_SEQ,    2)]


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


@lru_cache(maxsize=None)
def fastq(tiles: int) -> bytes:
    """150 bp reads that end inside tile number `tiles`, at ~12x coverage so that m = 3 has solid k-mers"""
    n_reads = (tiles * TILE - 100) // RB
    genome = synth.make_genome(max(400, n_reads * 150 // 12), seed=300 + tiles)
    return synth.make_fastq(genome, n_reads, 150, seed=400 + tiles, device="cpu").numpy().tobytes()


@lru_cache(maxsize=None)
def dense(tiles: int) -> bytes:
    """a sequence stream that ends inside tile number `tiles`: records of bases only, a newline behind each"""
    g = synth.make_genome(tiles * TILE - 100, seed=500 + tiles).tobytes()
    cuts = [0, 5000, 5021, 200_000, len(g) - 1]
    return b"".join(g[a:b - 1] + b"\n" for a, b in zip(cuts[:-1], cuts[1:]))


def oracle(data: bytes, m: int, fmt: int):
    ref = mo.Sketcher(K, S, m)
    if fmt == engine.FMT_FASTQ4:
        ref.add_fastx(data)
    else:
        for line in data.split(b"\n"):
            ref.add_seq(line)
    return ref.finish()


def exact_counts(data: bytes, fmt: int, hashes):
    """the multiplicity of every hash of a sketch in the whole input: the oracle with room for every distinct k-mer forgets nothing"""
    ref = mo.Sketcher(K, 1 << 20, 1)
    if fmt == engine.FMT_FASTQ4:
        ref.add_fastx(data)
    else:
        for line in data.split(b"\n"):
            ref.add_seq(line)
    all_h, all_c = ref.finish()
    at = np.searchsorted(all_h, hashes)
    assert np.array_equal(all_h[at], hashes)
    return all_c[at]


@pytest.mark.parametrize("name,m,tiles,first,fmt,literal", CASES, ids=[c[0] for c in CASES])
def test_launches_are_the_planned_ones(emul, name, m, tiles, first, fmt, literal):  # noqa: F811
    data = fastq(tiles) if fmt == engine.FMT_FASTQ4 else dense(tiles)
    assert pr.tiles_of(0, len(data)) == tiles
    cuts = [0, len(data)]
    if first is not None:
        cuts.insert(1, (first * TILE - 50) // RB * RB)         # a record start inside tile number `first`
    spans = list(zip(cuts[:-1], cuts[1:]))
    dev = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    dev[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    if first is not None:
        assert [pr.tiles_of(a % 16, b - a) for a, b in spans] == [first, tiles - first]
    sk = engine.Sketcher(K, S, m, expected_bytes=0)
    for a, b in spans:
        sk.push_device(dev.data_ptr() + a, b - a, fmt)
    sk.sync()
    launches = sk.stats()["launches"]
    got_h, got_c = sk.finish()
    sk.close()
    # the table of s = 1000 without a size hint.  The library does not report it; a different table would show here, though:
    # the first chunk of m = 1 is nslots / 4 bytes = 32 tiles, which is what makes the 33-tile cases two launches and not one
    nslots = 1 << 21
    rows = planned(emul, (S, m, nslots, 2 ** 64 - 1, 1), [(2 if fmt == engine.FMT_FASTQ4 else 0, 0, a % 16, b - a) for a, b in spans],
                   torch.cuda.get_device_properties(0).multi_processor_count)
    print(f"{name}: launches {launches}, planned {len(rows)}, literal {literal}")
    assert launches == len(rows)
    assert launches == literal
    want_h, want_c = oracle(data, m, fmt)
    assert np.array_equal(got_h, want_h)
    assert np.all(got_c >= want_c)      # exact multiplicities: never below the oracle's (its heap forgets evicted hashes' earlier occurrences)
    assert np.array_equal(got_c, exact_counts(data, fmt, got_h))

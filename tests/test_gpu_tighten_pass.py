"""The tighten pass (table_tighten_kernel) in its one-workgroup-per-CU form: the threshold it leaves is the rule's
(the edge of the first of 2048 bins below which s qualifying entries lie), computed here from the table's
own contents; the pass behind the last launch of a FASTQ push also checks the push's phase chain (the work of
phase_verify_kernel); and the words it clears for the next pass -- histogram, accumulators, ticket -- are clear however
often a sketcher is used."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo

pytestmark = pytest.mark.gpu

TILE = 16384
RB = synth.record_bytes(150)
U64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


@lru_cache(maxsize=None)
def fastq(tiles: int, seed: int = 0) -> bytes:
    n_reads = (tiles * TILE - 100) // RB
    genome = synth.make_genome(max(400, n_reads * 150 // 12), seed=300 + tiles + seed)
    return synth.make_fastq(genome, n_reads, 150, seed=400 + tiles + seed, device="cpu").numpy().tobytes()


def oracle(data: bytes, k, s, m):
    ref = mo.Sketcher(k, s, m)
    ref.add_fastx(data)
    return ref.finish()[0]


def rule(keys, cnts, T, s, m):
    """the threshold one exact pass leaves behind a table (keys, cnts) whose threshold is T"""
    lz = 64 - T.bit_length() if T else 63
    q = keys[(keys <= np.uint64(T)) & (cnts >= m)]
    bins = ((q << np.uint64(lz)) >> np.uint64(53)).astype(np.int64)
    cum = np.cumsum(np.bincount(bins, minlength=2048))
    at = int(np.searchsorted(cum, s))          # first bin at which the cumulative count reaches s
    if at >= 2048 or lz > 52:
        return T
    return min(T, ((at + 1) << (53 - lz)) - 1)


@pytest.mark.parametrize("k,s,m", [(21, 1000, 1), (21, 16, 1), (27, 1000, 3), (16, 1000, 1), (21, 1, 1), (21, 8191, 1), (21, 8192, 3)])
def test_threshold_is_the_rules(k, s, m):
    data = fastq(20)                           # one launch that admits everything, one pass behind it
    sk = engine.Sketcher(k, s, m, expected_bytes=0)
    sk.push_host(data, engine.FMT_FASTQ4)
    keys, cnts = sk.export(U64)
    t0 = U64 if k > 16 else (1 << 32) - 1
    t1 = rule(keys, cnts, t0, s, m)
    assert t1 < t0 or (cnts >= m).sum() < s
    assert sk.threshold() == rule(keys, cnts, t1, s, m)       # threshold(): one more pass, from t1
    got, _ = sk.finish()
    sk.close()
    assert np.array_equal(got, oracle(data, k, s, m))


def test_fewer_than_s_distinct_kmers_leave_the_threshold_alone():
    data = fastq(1)[: 4 * RB]
    for m in (1, 3):
        sk = engine.Sketcher(21, 1000, m, expected_bytes=0)
        sk.push_host(data, engine.FMT_FASTQ4)
        assert sk.threshold() == U64
        got, _ = sk.finish()
        sk.close()
        assert len(got) < 1000 and np.array_equal(got, oracle(data, 21, 1000, m))


def cut_record(data: bytes, tile: int) -> bytes:
    """Damage that no tile can see by itself: the record that crosses the border behind `tile` gets a longer name, so that
    its sequence line ends exactly at the border, and loses its '+' and quality lines.  Both tiles parse cleanly -- one ends
    after line 2 of a record, the next begins with line 1 of one -- and only the chain of their phases is broken."""
    border = (tile + 1) * TILE
    r = border // RB
    pad = border - (r * RB + 11 + 150 + 1)
    if pad < 0:
        r, pad = r - 1, pad + RB
    rec = data[r * RB:(r + 1) * RB]
    return data[: r * RB] + rec[:10] + b"x" * pad + rec[10:11 + 150 + 1] + data[(r + 1) * RB:]


@pytest.mark.parametrize("tile", [0, 31, 35])      # inside the first launch, at its border, inside the second
def test_phase_chain_is_checked_by_the_last_pass_of_a_push(tile):
    clean = fastq(40)
    for data, refused in ((clean, False), (cut_record(clean, tile), True)):
        sk = engine.Sketcher(21, 1000, 1, expected_bytes=0)
        sk.push_host(data, engine.FMT_FASTQ4)
        sk.sync()
        assert bool(sk.stats()["flags"] & 2) == refused
        if refused:
            with pytest.raises(engine.EngineError) as e:
                sk.finish()
            assert e.value.code == engine.MHX_E_FORMAT
        else:
            assert np.array_equal(sk.finish()[0], oracle(data, 21, 1000, 1))
        sk.close()


def test_every_push_checks_its_own_chain():
    clean = fastq(40)
    n = len(clean) // RB
    cuts = [0, 30 * RB, 31 * RB, (n // 2) * RB, (n - 40) * RB, len(clean)]     # pushes of one tile (no chain) and of many
    for bad in (None, 2, 3):
        sk = engine.Sketcher(21, 1000, 1, expected_bytes=0)
        dev = []
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            part = clean[a:b]
            if i == bad:
                part = cut_record(part, 0)
            t = torch.frombuffer(bytearray(part), dtype=torch.uint8).cuda()
            dev.append(t)
            sk.push_device(t.data_ptr(), len(part), engine.FMT_FASTQ4)
        sk.sync()
        assert bool(sk.stats()["flags"] & 2) == (bad is not None), bad
        if bad is None:
            assert np.array_equal(sk.finish()[0], oracle(clean, 21, 1000, 1))
        sk.close()


@pytest.mark.parametrize("s,m", [(1, 1), (16, 3), (1000, 1), (1000, 3), (8191, 1), (8192, 1)])
def test_one_sketcher_used_again_and_again(s, m):
    a, b = fastq(40), fastq(33, seed=7)
    want_a, want_ab = oracle(a, 21, s, m), oracle(a + b, 21, s, m)
    sk = engine.Sketcher(21, s, m, expected_bytes=0)
    for _ in range(3):                          # reset -> push -> finish: histogram, accumulators and ticket are clear each time
        sk.reset()
        sk.push_host(a, engine.FMT_FASTQ4)
        assert np.array_equal(sk.finish()[0], want_a)
    assert np.array_equal(sk.finish()[0], want_a)             # finish() twice in a row
    sk.push_host(b, engine.FMT_FASTQ4)                        # push -> finish -> push -> finish without a reset
    assert np.array_equal(sk.finish()[0], want_ab)
    sk.close()

"""The parse front of the sketch kernel on the device: the DPP workgroup scan (block_scan_excl, mhx_block.h), the bound tests
around the ends of a span, and the long-record count the line path takes from the ends of its sequence lines
(line_span_long_record, mhx_tile.h).

The shapes of tests/test_parse_front.py as FASTQ files of two to three tiles, pushed as device buffers at pointer alignments
0, 1 and 15, with lengths that end the span at a tile border +-1 and at tile + halo +-1.  The sketch size is above the number
of distinct k-mers, so the threshold stays at its maximum and every valid start's hash lands in the result with its
multiplicity; hashes and multiplicities are the C oracle's, k-mers, lines and records of stats() follow from the file by the
rule of tests/test_line_items.py.  A wrong prefix of the scan moves an event, a wrong bound masks a byte or counts a record
that ends the span: either changes `records`, `kmers` or the sketch.

The kernel forms: whatever the engine chooses (in this process) and, in child processes, the inline form plain and as the
split first launch, the queue form and the look-back format, forced the way tests/test_gpu_line_items.py forces them."""
import os
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import test_line_items as cpu

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE, HALO, S = cpu.TILE, cpu.HALO, 32768
KS = [21, 32]
LEADS = (0, 1, 15)
LENGTHS = (2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * TILE + HALO - 1, 2 * TILE + HALO, 2 * TILE + HALO + 1)


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def cycle(rng, lens, hdr_len, eol=b"\n", upto=2 * TILE + 3000):
    data, i = b"", 0
    while len(data) < upto:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len, eol=eol)
        i += 1
    return data


def cr_across_the_border(rng, k, bases):
    """`bases` bases and a CR in a sequence line that starts three bytes in front of the tile border (its quality line ends
    with a CR as well)"""
    start, n = TILE - 3, bases + 1
    data = bytearray(cpu.tile_with_line(rng, k, 0, start, start + n))
    assert data[start + n:start + n + 3] == b"\n+\n" and data[start + 2 * n + 3] == 10
    data[start + n - 1] = data[start + 2 * n + 2] = 13
    return bytes(data)


SHAPES = {
    "lengths_k_minus_1_k_k_plus_1": lambda rng, k: cycle(rng, (k - 1, k, k + 1), 260),
    "k_and_k_minus_1_bases_and_cr": lambda rng, k: cycle(rng, (k, k - 1, k + 1, k - 2), 260, eol=b"\r\n"),
    "starts_in_last_k_ends_in_halo": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - (k - 1), TILE + 9),
    "k_bytes_from_the_last_tile_byte": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 1, TILE - 1 + k),
    "k_minus_1_bytes_from_the_border": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE, TILE + k - 1),
    "k_bases_and_cr_across_the_border": lambda rng, k: cr_across_the_border(rng, k, k),
    "k_minus_1_bases_and_cr_across_the_border": lambda rng, k: cr_across_the_border(rng, k, k - 1),
    "runs_beyond_the_halo": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 100, TILE + 200),
    "line_0_continues_with_less_than_k": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 140, TILE + 10),
    "first_tile_of_a_span": lambda rng, k: b"@\n" + cpu.bases(rng, k) + b"\n+\n" + b"I" * k + b"\n" + cpu.fill(rng, b"", 2 * TILE + 3000),
    "falls_back_to_the_maps": lambda rng, k: cpu.tile_with_line(rng, k, 0, 8000, 8000 + 8 * 40 + k),
}


def fit(data: bytes, length: int) -> bytes:
    """whole records of `data` and a last one whose header makes the file `length` bytes long"""
    ends = [i + 1 for i, c in enumerate(data) if c == 10][3::4]       # the byte behind every record
    keep = max(e for e in ends if 330 <= length - e)
    assert keep > TILE + 400                                           # what the shape crafted around the first border is kept
    hdr = length - keep - (2 * 150 + 5)
    out = data[:keep] + b"@" + b"z" * (hdr - 1) + b"\n" + bytes(cpu.GENOME[:150]) + b"\n+\n" + b"I" * 150 + b"\n"
    assert len(out) == length
    return out


def expectation(data: bytes, k: int):
    lines = data.split(b"\n")
    seqs = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines[1::4]]
    vals, cnts = mo.bruteforce_sketch(seqs, k, 1 << 62, 1)
    assert 0 < len(vals) < S
    kmers, records = cpu.rule(data, k, 0)
    assert records == sum(len(s) >= k for s in seqs)
    return vals, cnts, (kmers, data.count(b"\n"), records)


@lru_cache(maxsize=None)
def shape(name: str, k: int, length: int):
    data = SHAPES[name](np.random.default_rng(sum(name.encode()) + k), k)
    if length:
        data = fit(data, length)
    assert 2 * TILE - 1 <= len(data) <= 3 * TILE and data.endswith(b"\n")
    return (data, *expectation(data, k))


def check(what, data, vals, cnts, want, k, lead=0) -> None:
    dev = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    dev[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    dev[lead + len(data):] = 10                                         # newlines right behind the span, which are not its own
    torch.cuda.synchronize()
    sk = engine.Sketcher(k, S, 1, expected_bytes=len(data))
    sk.push_device(dev.data_ptr() + lead, len(data), engine.FMT_FASTQ4, keep=dev)
    got, cnt = sk.finish()
    st = sk.stats()
    records = sk.record_count()
    sk.close()
    assert st["flags"] & 0xFF == 0, (what, st)
    assert (st["kmers"], st["lines"], records) == want, (what, st, records, want)
    assert np.array_equal(got, vals), f"{what}: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts), what


def check_shape(name, k, every_pair: bool) -> None:
    pairs = [(lead, n) for lead in LEADS for n in LENGTHS] if every_pair else list(zip(LEADS * 2, LENGTHS))
    for lead, n in [(lead, 0) for lead in LEADS] + pairs:              # 0: the file as the shape makes it
        check((name, k, lead, n), *shape(name, k, n), k, lead)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_at_every_alignment_and_span_end(name, k):
    check_shape(name, k, True)


# ---- the scan ------------------------------------------------------------------------------------------------------------------

def all_line_lengths_1_to_200(rng):
    """header, sequence and quality lines of 1 .. 200 bytes, record by record, the short ones first in one tile and last in
    the next: the 64 bytes of a thread hold between none and more than a dozen newlines, and the sums of the four waves of
    a tile differ"""
    data, i = b"", 0
    while len(data) < 2 * TILE + 3000:
        n = 1 + (i if i < 100 else 140 - i if i <= 140 else 199 - 7 * (i - 141)) % 200   # 1 .. 100, 41 down to 1, 200 down in sevens
        data += cpu.record(rng, i, n, hdr_len=n)
        i += 1
    for tile in (0, 1):
        per_thread = [data[t:t + 64].count(b"\n") for t in range(tile * TILE, (tile + 1) * TILE, 64)]
        assert min(per_thread) == 0 and max(per_thread) >= 12, (tile, max(per_thread))
        assert len({sum(per_thread[w:w + 64]) for w in range(0, 256, 64)}) == 4
    return data


def newlines_in_one_thread_only(rng):
    """tile 1 holds four newlines, all in the 64 bytes of thread 191 (lane 63 of wave 2): every prefix in front of it is 0,
    every prefix behind it the tile's total (this tile takes the look-back pass: under six newlines)"""
    first = TILE + 191 * 64 + 1                                         # the newline that ends the header
    data = cpu.fill(rng, b"", TILE - 700)
    data += b"@" + b"h" * (first - len(data) - 1) + b"\n" + cpu.bases(rng, 25) + b"\n+\n" + b"I" * 25 + b"\n"
    data += b"@" + b"h" * (TILE + 900) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    data = cpu.fill(rng, data, 3 * TILE + 1500)
    where = [i for i in range(TILE, 2 * TILE) if data[i] == 10]
    assert len(where) == 4 and all((i - TILE) // 64 == 191 for i in where)
    return data


def more_than_1024_newlines(rng):
    # seven records of 47 bytes and one of 87 (the one whose sequence line holds K bases), on and on
    data = b"".join(cpu.record(rng, i, 40 if i % 8 == 7 else 20, hdr_len=2) for i in range(2 * 320 + 40))
    assert data[:TILE].count(b"\n") > 1024
    return data


SCANS = {"line_lengths_1_to_200": all_line_lengths_1_to_200, "newlines_in_one_thread_only": newlines_in_one_thread_only,
         "more_than_1024_newlines": more_than_1024_newlines}


@lru_cache(maxsize=None)
def scan_case(name: str, k: int):
    data = SCANS[name](np.random.default_rng(sum(name.encode())))
    return (data, *expectation(data, k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SCANS))
def test_scan_on_the_device(name, k):
    for lead in LEADS:
        check((name, k, lead), *scan_case(name, k), k, lead)


def test_scan_in_the_fasta_parser():
    """a multi-record FASTA through the kernels of mhx_fasta.hip, which scan four times per tile: the dense stream and the
    separator positions against the rule, byte for byte"""
    from tests.fasta_rule import rule

    rng = np.random.default_rng(77)
    recs = []
    while sum(map(len, recs)) < 150_000:
        i, width = len(recs), int(rng.integers(1, 90))
        seq = cpu.bases(rng, int(rng.integers(0, 2500)))
        body = b"".join(seq[j:j + width] + b"\n" for j in range(0, len(seq), width))
        recs.append(b">r%d %s\n" % (i, b"d" * int(rng.integers(0, 300))) + body)
    data = b"".join(recs)
    got = engine.fasta_stream(data)
    assert got is not None
    want_stream, want_seps = rule(data)
    assert got[0] == want_stream
    assert np.array_equal(got[1], np.array(want_seps, dtype=np.uint64))


# ---- the kernel forms ------------------------------------------------------------------------------------------------------------

def run_form(form: str) -> None:
    """every shape and scan case in one kernel form, forced for this process by the caller"""
    engine.init(0)
    splits = ("1", "8") if form == "inline" else ("1",)   # with 8 the whole file is the split first launch
    for split in splits:
        os.environ["MHX_FIRST_SPLIT"] = split
        for k in KS:
            for name in SHAPES:
                check_shape(name, k, False)
            for name in SCANS:
                check((name, k), *scan_case(name, k), k, 1)
    print("ok")


FORMS = {"inline": {"MHX_QUEUE_CANDIDATES": "0"}, "queue": {"MHX_QUEUE_CANDIDATES": "1"}, "lookback": {"MHX_NO_SELFSYNC": "1"}}


@pytest.mark.parametrize("form", list(FORMS), ids=["inline_and_split", "queue", "lookback_format"])
def test_forced_kernel_form(form):
    env = dict(os.environ, PYTHONPATH=str(ROOT), **FORMS[form])
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_parse_front import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

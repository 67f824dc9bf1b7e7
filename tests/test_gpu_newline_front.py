"""The newline map and the phase search of the sketch kernel on the device, in the forms that work on fewer instructions:
newline_mask with one 64-bit add and two chained multiply-adds per dword pair, and the line phase from the first six entries
of the newline list, tested by four lanes of the first wave (selfsync_triple, mhx_tile.h).

Files of three tiles each.  The sketch size is above the number of distinct k-mers, so the threshold stays at its maximum and
every valid start's hash lands in the result with its multiplicity: hashes and multiplicities are the C oracle's; k-mers, lines
and records of stats() follow from the file by the rule of tests/test_line_items.py.  A newline missed or invented moves a
line, a wrong phase takes quality lines for sequence lines: either changes `records`, `kmers` or the sketch.

The kernel forms: whatever the engine chooses (in this process) and, in child processes, the inline form plain and as the
split first launch, the queue form and the look-back format, forced the way tests/test_gpu_parse_front.py forces them."""
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
TILE, HALO, S, K = cpu.TILE, cpu.HALO, 32768, 21
UPTO = 2 * TILE + 3000


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def cycle(rng, lens, hdr_len, eol=b"\n"):
    data, i = b"", 0
    while len(data) < UPTO:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len, eol=eol)
        i += 1
    return data


def more_than_1024_newlines(rng):
    # seven records of 47 bytes and one of 87 (the one whose sequence line holds K bases), on and on: phase_events does not fit
    data, i = b"", 0
    while len(data) < UPTO:
        data += cpu.record(rng, i, 40 if i % 8 == 7 else 20, hdr_len=2)
        i += 1
    assert all(data[t * TILE:(t + 1) * TILE].count(b"\n") > 1024 for t in (0, 1))
    return data


def sixth_newline_at(rng, at):
    """tile 1 begins a record; its sixth newline is byte `at` of the tile: 4095 is the first wave's, 4096 is not"""
    data = cpu.fill(rng, b"", TILE - 1000)
    data += b"@" + b"p" * (TILE - len(data) - 306) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    assert len(data) == TILE
    data += cpu.record(rng, 1, 150)
    data += b"@" + b"h" * (at - 468) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    data = cpu.fill(rng, data, UPTO)
    assert [i - TILE for i in range(TILE, 2 * TILE) if data[i] == 10][5] == at
    return data


def at_and_plus_quality_lines(rng):
    data, i = b"", 0
    while len(data) < UPTO:
        r = cpu.record(rng, i, 150, hdr_len=11 + i % 7).split(b"\n")
        r[3] = (b"@", b"+", b"@+", b"+@")[i % 4] + r[3][2:] + b"I" * (i % 4 < 2)
        data += b"\n".join(r)
        i += 1
    return data


FASTQ = {f"header_of_{h}_bytes": (lambda rng, h=h: cycle(rng, (150,), h)) for h in range(1, 33)}
FASTQ.update({
    "crlf": lambda rng: cycle(rng, (150, 141, K, K - 1), 40, eol=b"\r\n"),
    "more_than_1024_newlines": more_than_1024_newlines,
    "sixth_newline_at_4095": lambda rng: sixth_newline_at(rng, 4095),
    "sixth_newline_at_4096": lambda rng: sixth_newline_at(rng, 4096),
    "quality_lines_with_at_and_plus": at_and_plus_quality_lines,
    # tile 1 begins in a header; of its first six newlines three are its own and three lie in the halo
    "first_six_newlines_across_the_border": lambda rng: cpu.fill(
        rng, b"@" + b"h" * (2 * TILE - 12) + b"\nACGT\n+\nIIII\n@b\nAC\n+\nII\n", UPTO),
    "reads_of_3_kb": lambda rng: cpu.fill(rng, b"", UPTO, seq_len=3000),     # six newlines in a tile, not in its first 4 KiB
    "reads_of_6_kb": lambda rng: cpu.fill(rng, b"", UPTO, seq_len=6000),     # tiles of under six newlines: the look-back pass
})


@lru_cache(maxsize=None)
def fastq_case(name: str):
    data = FASTQ[name](np.random.default_rng(sum(name.encode())))
    assert UPTO <= len(data) <= 3 * TILE and data.endswith(b"\n"), (name, len(data))
    lines = data.split(b"\n")
    seqs = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines[1::4]]
    vals, cnts = mo.bruteforce_sketch(seqs, K, 1 << 62, 1)
    assert 0 < len(vals) < S
    kmers, records = cpu.rule(data, K, 0)
    assert records == sum(len(s) >= K for s in seqs)
    return data, vals, cnts, (kmers, data.count(b"\n"), records)


@lru_cache(maxsize=None)
def fasta_case():
    """a sequence stream: lines of 1 .. 96 bases, so that the separators fall on every byte of a 32-byte word"""
    rng = np.random.default_rng(3)
    seqs = []
    while sum(len(s) + 1 for s in seqs) < UPTO:
        seqs.append(cpu.bases(rng, 1 + (7 * len(seqs)) % 96))
    data = b"\n".join(seqs) + b"\n"
    assert {i % 32 for i, c in enumerate(data) if c == 10} == set(range(32)) and len(data) <= 3 * TILE
    vals, cnts = mo.bruteforce_sketch(seqs, K, 1 << 62, 1)
    assert 0 < len(vals) < S
    return data, vals, cnts, sum(max(0, len(s) - K + 1) for s in seqs)


def sketch(data: bytes, fmt: int, lead: int):
    dev = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    dev[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    dev[lead + len(data):] = 10                                         # newlines right behind the span, which are not its own
    torch.cuda.synchronize()
    sk = engine.Sketcher(K, S, 1, expected_bytes=len(data))
    sk.push_device(dev.data_ptr() + lead, len(data), fmt, keep=dev)
    got, cnt = sk.finish()
    st = sk.stats()
    records = sk.record_count()
    sk.close()
    return got, cnt, st, records


def check_fastq(name: str, lead: int = 0) -> None:
    data, vals, cnts, want = fastq_case(name)
    got, cnt, st, records = sketch(data, engine.FMT_FASTQ4, lead)
    assert st["flags"] & 0xFF == 0, (name, st)
    assert (st["kmers"], st["lines"], records) == want, (name, st, records, want)
    assert np.array_equal(got, vals), f"{name}: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts), name


def check_fasta(lead: int = 0) -> None:
    data, vals, cnts, kmers = fasta_case()
    got, cnt, st, _ = sketch(data, engine.FMT_SEQ, lead)
    assert st["flags"] & 0xFF == 0 and st["kmers"] == kmers, (st, kmers)
    assert np.array_equal(got, vals), f"sequence stream: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts)


@pytest.mark.parametrize("name", list(FASTQ))
def test_fastq(name):
    for lead in (0, 1 + sum(name.encode()) % 15):     # the tile grid is the buffer's, the words are the pointer's: both alignments
        check_fastq(name, lead)


def test_sequence_stream():
    for lead in (0, 1, 15):
        check_fasta(lead)


# ---- the kernel forms ------------------------------------------------------------------------------------------------------------

def run_form(form: str) -> None:
    """every case in one kernel form, forced for this process by the caller"""
    engine.init(0)
    splits = ("1", "8") if form == "inline" else ("1",)   # with 8 the whole file is the split first launch
    for split in splits:
        os.environ["MHX_FIRST_SPLIT"] = split
        for name in FASTQ:
            check_fastq(name, 1)
        check_fasta(1)
    print("ok")


FORMS = {"inline": {"MHX_QUEUE_CANDIDATES": "0"}, "queue": {"MHX_QUEUE_CANDIDATES": "1"}, "lookback": {"MHX_NO_SELFSYNC": "1"}}


@pytest.mark.parametrize("form", list(FORMS), ids=["inline_and_split", "queue", "lookback_format"])
def test_forced_kernel_form(form):
    env = dict(os.environ, PYTHONPATH=str(ROOT), **FORMS[form])
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_newline_front import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

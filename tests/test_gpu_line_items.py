"""The FASTQ work list made from the line list (phase_line_span + phase_line_items, mhx_tile.h) on the device: the crafted
tiles of tests/test_line_items.py as FASTQ files of two to three tiles, at K = 21 and 27.  The sketch size is above the
number of distinct k-mers, so the threshold stays at its maximum and every valid start's hash lands in the result with its
multiplicity: a start the list loses or a mask bit too many shows as a missing hash or a wrong count.  Hashes and
multiplicities are the C oracle's (every window of every sequence line); k-mers, lines and records of stats() are computed
from the file by the rule: a sequence line of n bytes (a CR included) has n - K + 1 starts, and its record counts if it holds
K bases.

Tile 0 of every file is interior and, where the case says so, takes the line items; the last tile never does, so every file
runs both forms side by side.  The kernel forms: whatever the engine chooses (in this process), and in child processes --
MHX_QUEUE_CANDIDATES and MHX_NO_SELFSYNC are read once -- the inline form plain and as the split first launch, the queue form,
and the look-back format, whose kernels keep the maps on every tile (line_items_form) and must give the same for the same
files.

Nothing here shows that a tile TOOK the line path (kernel text is not inspected): which tile takes which form is pinned on the
CPU by tests/test_line_items.py, and on the device by the instruction counter of profiles/line_items_ab.txt, section 2.  With
the path switched off by mistake these tests would pass on the maps."""
import os
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import test_line_items as cpu

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TILE, S = cpu.TILE, 32768
KS = [21, 27]


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def recs(rng, size, n, hdr_len):
    seq = (size - hdr_len - 5) // 2
    data = b"".join(cpu.record(rng, i, seq, hdr_len=size - 2 * seq - 5) for i in range(n))
    assert len(data) == n * size
    return data


def cycle(rng, lens, hdr_len, eol=b"\n", upto=2 * TILE + 3000):
    data, i = b"", 0
    while len(data) < upto:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len, eol=eol)
        i += 1
    return data


CASES = {
    "ordinary": lambda rng, k: cpu.fill(rng, b"", 2 * TILE + 3000),
    "starts_in_last_k_minus_1": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - (k - 1), TILE + 140),
    "starts_in_last_byte": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 1, TILE + 149),
    "newline_at_16382": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - k - 5, TILE - 2),
    "newline_at_16383": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - k - 5, TILE - 1),
    "newline_at_16384": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - k - 5, TILE),
    "newline_in_halo": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 100, TILE + k - 1),
    "newline_in_second_halo_word": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 100, TILE + 40),
    "newline_beyond_halo": lambda rng, k: cpu.tile_with_line(rng, k, 0, TILE - 100, TILE + 64),   # ... and tile 1 begins inside a sequence line
    "crlf": lambda rng, k: cycle(rng, (k - 1, k, k + 1, 150), 200, eol=b"\r\n"),
    "lengths_around_k": lambda rng, k: cycle(rng, (0, k - 1, k, k + 1, 3 * k), 260),
    "lines_64": lambda rng, k: recs(rng, 256, 64 * 2 + 20, 11),
    "lines_65": lambda rng, k: recs(rng, 252, 65 * 2 + 20, 11),
    "lines_260": lambda rng, k: recs(rng, 63, 260 * 2 + 40, 4),
    "at_the_group_bound": lambda rng, k: cpu.tile_with_line(rng, k, 0, 8000, 8000 + 8 * 40 + k - 1),
    "above_the_group_bound": lambda rng, k: cpu.tile_with_line(rng, k, 0, 8000, 8000 + 8 * 40 + k),
    "line_of_3000": lambda rng, k: cpu.tile_with_line(rng, k, 0, 5000, 8000),
    "tile_without_newline": lambda rng, k: through_header(rng),
}


def through_header(rng):
    """ordinary records, one of them with a header line that runs through the whole of tile 1"""
    data = cpu.fill(rng, b"", TILE - 700)
    assert len(data) < TILE - 300
    data += b"@" + b"h" * (TILE + 800) + b"\n" + cpu.bases(rng, 150) + b"\n+\n" + b"I" * 150 + b"\n"
    assert b"\n" not in data[TILE:2 * TILE]
    return cpu.fill(rng, data, 2 * TILE + 1500)


@lru_cache(maxsize=None)
def case(name: str, k: int):
    """the file, the oracle's hashes and multiplicities, and (k-mers, lines, records) by the rule"""
    data = CASES[name](np.random.default_rng(sum(name.encode()) + k), k)
    assert 2 * TILE < len(data) <= 3 * TILE and data.endswith(b"\n")
    lines = data.split(b"\n")
    seqs = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines[1::4]]
    vals, cnts = mo.bruteforce_sketch(seqs, k, 1 << 62, 1)
    assert 0 < len(vals) < S
    kmers, records = cpu.rule(data, k, 0)
    assert records == sum(len(s) >= k for s in seqs)
    return data, vals, cnts, (kmers, data.count(b"\n"), records)


def check(name: str, k: int) -> None:
    data, vals, cnts, want = case(name, k)
    sk = engine.Sketcher(k, S, 1, expected_bytes=len(data))
    sk.push_host(data, engine.FMT_FASTQ4)
    got, cnt = sk.finish()
    st = sk.stats()
    records = sk.record_count()
    sk.close()
    assert st["flags"] & 0xFF == 0, (name, k, st)
    assert (st["kmers"], st["lines"], records) == want, (name, k, st, records, want)
    assert np.array_equal(got, vals), f"{name} k={k}: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts), (name, k)


def test_the_files_have_k_mers_that_repeat():
    assert case("ordinary", 21)[2].max() > 1


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_crafted_tiles_against_the_oracle(name, k):
    check(name, k)


def run_form(form: str) -> None:
    """every case in one kernel form, forced for this process by the caller"""
    engine.init(0)
    splits = ("1", "8") if form == "inline" else ("1",)   # three tiles: with 8 the whole file is the split first launch
    for split in splits:
        os.environ["MHX_FIRST_SPLIT"] = split
        for k in KS:
            for name in CASES:
                check(name, k)
    print("ok")


FORMS = {"inline": {"MHX_QUEUE_CANDIDATES": "0"}, "queue": {"MHX_QUEUE_CANDIDATES": "1"}, "lookback": {"MHX_NO_SELFSYNC": "1"}}


@pytest.mark.parametrize("form", list(FORMS), ids=["inline_and_split", "queue", "lookback_format"])
def test_forced_kernel_form(form):
    env = dict(os.environ, PYTHONPATH=str(ROOT), **FORMS[form])
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_line_items import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

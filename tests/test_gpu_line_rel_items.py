"""The line-relative items of the sketch kernel (phase_line_rel_items, process_line_rel_item: mhx_tile.h) on the device: FASTQ
files of three tiles and a few bytes -- read lengths 148 .. 155, so that the starts of a line leave every remainder 0 .. 7 at
K = 21, and one file of mixed lengths -- pushed from device memory at two pointer alignments.  The sketch size is above the
number of distinct k-mers, so the threshold stays at its maximum and every valid start's hash lands in the result with its
multiplicity: a window the items lose, list twice or read from the wrong byte shows as a missing hash or a wrong count.
Hashes and multiplicities are the C oracle's, bit for bit, and the same at both alignments.

At the first alignment the span begins on a 16-byte boundary and tiles 0 .. 2 are interior; at the second it begins 5 bytes
behind one, every line stands 5 bytes further into its tile and tile 0, which holds the start of the span, keeps the maps.

The kernel forms are forced in child processes (MHX_QUEUE_CANDIDATES is read once): the inline form at K = 21 (plain and as
the split first launch), 16 (32-bit hashes), 29 and 32, and the queue form at K = 27.  The inline form of K = 32 is one that
line_rel_form leaves on the aligned items (registers): its case pins that form on the same files; K = 29 is the largest K whose
inline form takes the new items.  As in tests/test_gpu_line_items.py nothing here shows that a tile TOOK the path:
tests/test_line_rel_items.py pins that, and the switch, on the CPU."""
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
TILE, S = cpu.TILE, 32768
OFFSETS = (0, 5)         # bytes behind a 16-byte boundary at which the pushed span begins
# name -> (read lengths in turn, header length: 48 newlines at least and 64 sequence lines at most in a tile)
FILES = {**{"len_%d" % n: ((n,), 11) for n in range(148, 156)}, "mixed": ((150, 148, 21, 101, 76, 250, 27, 151, 16, 33), 120)}
# form -> (environment, [(K, MHX_FIRST_SPLIT)])
FORMS = {"inline": ({"MHX_QUEUE_CANDIDATES": "0"}, [(21, "1"), (21, "8"), (16, "1"), (29, "1"), (32, "1")]),
         "queue": ({"MHX_QUEUE_CANDIDATES": "1"}, [(27, "1")])}


@lru_cache(maxsize=None)
def fastq(name: str) -> bytes:
    rng, (lens, hdr_len) = np.random.default_rng(sum(name.encode())), FILES[name]
    data, i = b"", 0
    while len(data) < 3 * TILE + 70:
        data += cpu.record(rng, i, lens[i % len(lens)], hdr_len=hdr_len)
        i += 1
    assert 3 * TILE + 64 <= len(data) < 3 * TILE + 700
    return data


@lru_cache(maxsize=None)
def oracle(name: str, k: int):
    seqs = fastq(name).split(b"\n")[1::4]
    vals, cnts = mo.bruteforce_sketch(seqs, k, 1 << 62, 1)
    assert 0 < len(vals) < S and cnts.max() > 1
    return vals, cnts, sum(max(0, len(s) - k + 1) for s in seqs)


def check(name: str, k: int) -> None:
    data = fastq(name)
    vals, cnts, kmers = oracle(name, k)
    results = []
    for off in OFFSETS:
        dev = torch.zeros(len(data) + 256, dtype=torch.uint8, device="cuda")
        at = (-dev.data_ptr()) % 16 + 16 + off
        dev[at:at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        sk = engine.Sketcher(k, S, 1, expected_bytes=len(data))
        sk.push_device(dev.data_ptr() + at, len(data), engine.FMT_FASTQ4, keep=dev)
        got, cnt = sk.finish()
        st = sk.stats()
        sk.close()
        assert st["flags"] & 0xFF == 0 and st["kmers"] == kmers, (name, k, off, st, kmers)
        assert np.array_equal(got, vals), f"{name} k={k} offset {off}: {len(got)} hashes, {len(vals)} expected"
        assert np.array_equal(cnt, cnts), (name, k, off)
        results.append((got, cnt))
    assert all(np.array_equal(a, b) for a, b in zip(results[0], results[1]))


def run_form(form: str) -> None:
    """every file in the kernel forms of FORMS[form], forced for this process by the caller"""
    engine.init(0)
    for k, split in FORMS[form][1]:
        os.environ["MHX_FIRST_SPLIT"] = split
        for name in FILES:
            check(name, k)
    print("ok")


@pytest.mark.parametrize("form", list(FORMS))
def test_forced_kernel_form(form):
    env = dict(os.environ, PYTHONPATH=str(ROOT), **FORMS[form][0])
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_line_rel_items import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

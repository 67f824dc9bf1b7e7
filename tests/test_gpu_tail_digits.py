"""The hash loop with the tail table's offset taken from digits packed once per group (TailDigits, mhx_tile.h) on the
device: EVERY window hash of a small input against the C oracle, hashes and multiplicities, at every K that has a table
(17..21, 25..29; the hot loop packs at those tail_digits_apply names and keeps the per-window index at the others).

Input: 130 reads of 150 bp from a 5 kb genome (~40 KB: windows cross two tile borders and the halo), lower-case reads
and stretches and a few N among them, as 4-line FASTQ and, at K = 21 and 27, the same reads as a sequence stream.  The
sketch size, 32768, is above the number of distinct k-mers, so the threshold stays at its maximum, every window is a
candidate, and every window's hash lands in the result: a single wrong table offset shows as a wrong or missing hash.

Kernel forms, each forced in a child process (MHX_QUEUE_CANDIDATES, as tests/test_gpu_tail_lut.py forces them): the
inline form finishes each candidate from the loop's own partial hash, so the small input pins the loop window by
window; the queue form only ADMITS by the loop's hash (process_deferred hashes again), and with the threshold at its
maximum it admits everything, so it also runs the 13 000 reads of tests/test_gpu_admission_bound.py at K = 21 with
s = 8192, where launches run behind a lowered threshold and a hash the loop gets wrong is a hash the sketch loses."""
import os
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo
from tests import test_gpu_admission_bound as big

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N_READS, READ_LEN, S = 130, 150, 32768
RB = synth.record_bytes(READ_LEN)
LUT_KS = [17, 18, 19, 20, 21, 25, 26, 27, 28, 29]


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


@lru_cache(maxsize=None)
def fastq() -> bytes:
    genome = synth.make_genome(5_000, seed=811)
    fq = synth.make_fastq(genome, N_READS, READ_LEN, seed=812, device="cpu").numpy().copy()
    bases = fq.reshape(N_READS, RB)[:, 11:11 + READ_LEN]
    rng = np.random.default_rng(813)
    bases[rng.random(N_READS) < 0.15] |= 0x20                      # whole reads in lower case
    for r, c in zip(rng.integers(0, N_READS, size=30), rng.integers(0, READ_LEN - 30, size=30)):
        bases[r, c:c + 30] |= 0x20                                  # lower-case stretches
    bases[rng.random(bases.shape) < 0.03] |= 0x20                  # single lower-case bases
    for r, c in zip(rng.integers(0, N_READS, size=10), rng.integers(0, READ_LEN, size=10)):
        bases[r, c] = ord("N") if r % 2 else ord("n")
    return fq.tobytes()


@lru_cache(maxsize=None)
def reads():
    rec = np.frombuffer(fastq(), np.uint8).reshape(N_READS, RB)
    return [r[11:11 + READ_LEN].tobytes() for r in rec]


@lru_cache(maxsize=None)
def definition(k: int):
    """every window hash of the input, ascending, with its multiplicity"""
    vals, cnts = mo.bruteforce_sketch(reads(), k, 1 << 62, 1)
    assert 1000 < len(vals) < S and cnts.max() > 1
    return vals, cnts


def check(data: bytes, fmt: int, k: int) -> None:
    sk = engine.Sketcher(k, S, 1, expected_bytes=len(data))
    sk.push_host(data, fmt)
    got, cnt = sk.finish()
    st = sk.stats()
    sk.close()
    vals, cnts = definition(k)
    assert np.array_equal(got, vals), f"k={k}: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts)
    # the statistic counts the candidate starts (k bytes inside one sequence line), never a window hashed over anything else
    assert st["kmers"] == N_READS * (READ_LEN - k + 1), st


@pytest.mark.parametrize("k", LUT_KS)
def test_every_window_hash_of_a_fastq(k):
    data = fastq()
    assert 2 * 16384 < len(data) <= 3 * 16384
    check(data, engine.FMT_FASTQ4, k)


@pytest.mark.parametrize("k", [21, 27], ids=["k1_table", "k2_table"])
def test_every_window_hash_of_a_sequence_stream(k):
    check(b"\n".join(reads()), engine.FMT_SEQ, k)


def run_form(form: str) -> None:
    """one kernel form, forced for this process by the caller"""
    assert os.environ["MHX_QUEUE_CANDIDATES"] == form
    engine.init(0)
    for k in LUT_KS:
        check(fastq(), engine.FMT_FASTQ4, k)
    check(b"\n".join(reads()), engine.FMT_SEQ, 21)
    if form == "1":
        for s, m in big.SM_QUEUE:
            big.check("fastq", big.fastq(), engine.FMT_FASTQ4, 21, s, m)
    print("ok")


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline", "queue"])
def test_forced_kernel_form(form):
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    code = "from tests.test_gpu_tail_digits import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

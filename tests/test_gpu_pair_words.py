"""The hash loop with the words of windows J and J + 4 from one funnel shift per strand (PairWords, mhx_tile.h) on the
device: EVERY window hash of a small input against the C oracle, hashes and multiplicities, at every K that takes the
route and at one that keeps the per-window extraction.

Input: that of tests/test_gpu_tail_digits.py -- 130 reads of 150 bp from a 5 kb genome (~40 KB: windows cross two tile
borders and the halo, where a wrong dword index shows), lower case and N mixed in, the sketch size above the number of
distinct k-mers, so every window's hash and multiplicity lands in the result -- as 4-line FASTQ and as a sequence stream.

Kernel forms, each forced in a child process (MHX_QUEUE_CANDIDATES, as that test forces them).  The inline child runs
the input once more with the first launch split eight ways (MHX_FIRST_SPLIT, tests/test_gpu_first_launch_split.py): the
SPLIT form of the kernel.  The queue form only ADMITS by the loop's hash, and with the threshold at its maximum it admits
everything, so the queue child also runs the 13 000 reads of tests/test_gpu_admission_bound.py with s = 8192, where
launches run behind a lowered threshold and a hash the loop gets wrong is a hash the sketch loses."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from auriclass_amd import engine
from tests import test_gpu_admission_bound as big
from tests import test_gpu_tail_digits as small

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PAIR_KS = [17, 18, 19, 21, 23, 25, 26, 27, 29]      # pair_words_apply (tests/test_pair_words.py pins the switch)
KS = PAIR_KS + [22]  # ... and a K whose kernels keep canonical_words per window


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def seq_stream() -> bytes:
    return b"\n".join(small.reads())


@pytest.mark.parametrize("k", KS)
def test_every_window_hash_of_a_fastq(k):
    data = small.fastq()
    assert 2 * 16384 < len(data) <= 3 * 16384
    small.check(data, engine.FMT_FASTQ4, k)


@pytest.mark.parametrize("k", KS)
def test_every_window_hash_of_a_sequence_stream(k):
    small.check(seq_stream(), engine.FMT_SEQ, k)


def run_form(form: str) -> None:
    """one kernel form, forced for this process by the caller"""
    assert os.environ["MHX_QUEUE_CANDIDATES"] == form
    engine.init(0)
    if form == "0":
        os.environ["MHX_FIRST_SPLIT"] = "1"     # left to itself a first launch of three tiles splits: the plain form first
    for k in KS:
        small.check(small.fastq(), engine.FMT_FASTQ4, k)
        small.check(seq_stream(), engine.FMT_SEQ, k)
    if form == "0":
        os.environ["MHX_FIRST_SPLIT"] = "8"     # three tiles: the whole input is the first launch
        for k in KS:
            small.check(small.fastq(), engine.FMT_FASTQ4, k)
            small.check(seq_stream(), engine.FMT_SEQ, k)
    else:
        for k in PAIR_KS:
            for s, m in big.SM_QUEUE:
                big.check("fastq", big.fastq(), engine.FMT_FASTQ4, k, s, m)
    print("ok")


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline_and_split", "queue"])
def test_forced_kernel_form(form):
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_pair_words import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

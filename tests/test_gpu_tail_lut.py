"""The hash loop with the tail block's partial word taken from a table (mhx_tail_lut.h, murmur3_core<K, true>) on the
device: hashes and counts against the C oracle, exactly, at every tail layout that has a table -- K = 17, 19, 21 (partial
k1 of 1, 3, 5 bases), 25, 27, 29 (partial k2 behind a full k1) -- and at K = 22, which has none, as the control.

Small input (~190 KB, 12 tiles): 600 reads of 150 bp from a 20 kb genome with lower-case stretches and a few N, as
4-line FASTQ and, at K = 21 and 27 (one K of either table form), as a sequence stream whose last read ends with the last byte of the span (no newline
behind it), so that the last group's register chunk reaches into the halo.  The hot loop hashes every window of every
tile, the ones over header, '+' and quality lines, newlines and N included: their index must stay inside the table
and none of them may show in a hash, a count or the k-mer statistic.

Larger input: the 13 000 reads of tests/test_gpu_admission_bound.py at K = 21 and 27, so that launches run behind a
lowered threshold, each kernel form forced as that file forces it (MHX_QUEUE_CANDIDATES, a child process per form): the
inline form at (s, m) = (1000, 1) and (1000, 3), the queue form at s = 8192 (its candidates are finished by
process_deferred, which keeps the multiply form).  One containment screen at K = 21: the PROBE kernels share the loop."""
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
N_READS, READ_LEN = 600, 150
RB = synth.record_bytes(READ_LEN)
SMALL_KS = [17, 19, 21, 25, 27, 29, 22]
BIG_KS = [21, 27]


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


@lru_cache(maxsize=None)
def small_fastq() -> bytes:
    genome = synth.make_genome(20_000, seed=711)
    fq = synth.make_fastq(genome, N_READS, READ_LEN, seed=712, device="cpu").numpy().copy()
    bases = fq.reshape(N_READS, RB)[:, 11:11 + READ_LEN]
    rng = np.random.default_rng(713)
    bases[rng.random(N_READS) < 0.1] |= 0x20                       # whole reads in lower case
    for r, c in zip(rng.integers(0, N_READS, size=60), rng.integers(0, READ_LEN - 30, size=60)):
        bases[r, c:c + 30] |= 0x20                                  # lower-case stretches
    for r, c in zip(rng.integers(0, N_READS, size=12), rng.integers(0, READ_LEN, size=12)):
        bases[r, c] = ord("N") if r % 2 else ord("n")
    bases[N_READS - 1, READ_LEN - 40:] |= 0x20                     # the very last windows of the span in lower case
    return fq.tobytes()


@lru_cache(maxsize=None)
def small_reads():
    rec = np.frombuffer(small_fastq(), np.uint8).reshape(N_READS, RB)
    return [r[11:11 + READ_LEN].tobytes() for r in rec]


@lru_cache(maxsize=None)
def small_definition(k: int):
    """every window hash of the small input, ascending, with its multiplicity"""
    return mo.bruteforce_sketch(small_reads(), k, 1 << 62, 1)


def check_small(data: bytes, fmt: int, k: int, s: int = 1000, m: int = 1) -> None:
    sk = engine.Sketcher(k, s, m, expected_bytes=len(data))
    sk.push_host(data, fmt)
    got, cnt = sk.finish()
    st = sk.stats()
    sk.close()
    ref = mo.Sketcher(k, s, m)
    for seq in small_reads():
        ref.add_seq(seq)
    want, want_cnt = ref.finish()
    assert np.array_equal(got, want)
    assert np.all(cnt >= want_cnt)              # mash's heap forgets the occurrences of a hash it evicted in between
    vals, cnts = small_definition(k)
    assert len(vals) >= s
    assert np.array_equal(got, vals[:s]) and np.array_equal(cnt, cnts[:s])
    # the statistic counts the candidate starts (k bytes inside one sequence line), never a window hashed over anything else
    assert st["kmers"] == N_READS * (READ_LEN - k + 1), st


@pytest.mark.parametrize("k", SMALL_KS)
def test_small_fastq_at_every_tail_layout(k):
    data = small_fastq()
    assert 11 * 16384 < len(data) <= 12 * 16384
    check_small(data, engine.FMT_FASTQ4, k)


@pytest.mark.parametrize("k", [21, 27], ids=["k1_table", "k2_table"])
def test_small_sequence_stream_ending_with_the_last_read(k):
    stream = b"\n".join(small_reads())
    assert stream[-1:] not in (b"\n", b"\r")
    check_small(stream, engine.FMT_SEQ, k)


def run_form(form: str) -> None:
    """every case of one kernel form on the larger input; the caller has forced the form for this process.
    These are the K = 21 and 27 cases of tests/test_gpu_admission_bound.py's own forced runs (the same input, SM_INLINE,
    SM_QUEUE, check() and child-process mechanism), run here once more so that what pins the table stands in one file:
    they add no coverage while that file keeps 21 and 27 among its KS, and keep the table pinned if it ever drops them."""
    assert os.environ["MHX_QUEUE_CANDIDATES"] == form
    engine.init(0)
    for k in BIG_KS:
        for s, m in (big.SM_QUEUE if form == "1" else big.SM_INLINE):
            big.check("fastq", big.fastq(), engine.FMT_FASTQ4, k, s, m)
    print("ok")


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline", "queue"])
def test_forced_kernel_form_with_a_lowered_threshold(form):
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    code = "from tests.test_gpu_tail_lut import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_containment_screen_shares_the_loop():
    from tests import screen_rule as rule
    from tests.test_gpu_screen import check_result, pack, sketch_of

    k, s = 21, 1000
    genome = synth.make_genome(100_000, seed=611)          # the genome the larger input's reads come from
    refs = [sketch_of(genome, k, s), sketch_of(synth.mutate(genome, 0.01, 8), k, s), sketch_of(synth.make_genome(100_000, seed=202), k, s)]
    rows, lens = pack(refs)
    data = big.fastq()
    osk = mo.Sketcher(k, s, 1)
    osk.add_fastx(data)
    want = rule.tally(refs, rule.window_hashes(big.fastq_reads(), k))
    assert want[0][1] > 0.9 * len(refs[0]) and want[2][1] <= 2
    sc = engine.Screener(k, rows, lens, s)
    try:
        sc.push_host(data, engine.FMT_FASTQ4)
        check_result(refs, k, sc.finish(with_counts=True), want, osk.set_size)
    finally:
        sc.close()

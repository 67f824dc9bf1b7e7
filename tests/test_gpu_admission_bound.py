"""The admission test of the hash loop on the device (Murmur3Tail::high_bound against admission_limit(T), mhx_tile.h): a
necessary condition of h <= T that must not lose a single hash.  It only decides anything once the threshold has come
down -- the first chunk of a sketch is admitted whole -- so the input is ~4 MB: 13 000 reads of 150 bp from a 100 kb genome,
some in lower case, a few N, at k-mer sizes on both sides of the 32-bit / 64-bit hash border and with every tail layout
of the hash.

Which kernel form a launch takes is the engine's choice (push_span): on an input of this size every FASTQ launch
behind the first chunk is the QUEUE form whatever s is, and the inline launches are the first ones, which admit
everything.  So each form is forced (MHX_QUEUE_CANDIDATES, read once per process: a child process per form): the
inline form (finish() behind the candidate branch; the low word reused for 32-bit hashes) with s = 1000 at m = 1 and 3
and on a sequence stream, the queue form (process_deferred) with s = 8192.  Every case asserts that launches ran behind
the first and that they admitted only a part of their windows.  The engine's own schedule runs in this process as well.

Hashes against mash's own sketch (the C oracle fed the same bytes), hashes and counts against the definition (every
window hash of the C oracle, sorted and counted: the device's counts are exact multiplicities)."""
import os
import subprocess
import sys
from pathlib import Path
from functools import lru_cache

import numpy as np
import pytest

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

N_READS, READ_LEN = 13_000, 150
RB = synth.record_bytes(READ_LEN)
KS = [16, 17, 21, 27, 32]
SM_INLINE = [(1000, 1), (1000, 3)]          # the inline form, without and with the multiplicity filter
SM_QUEUE = [(8192, 1)]                      # the queue form


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def spoil(bases: np.ndarray, rng) -> None:
    """some stretches in lower case, some single bases, and a few N (in place; bases: rows of sequence bytes)"""
    rows = bases.shape[0]
    whole = rng.random(rows) < 0.1
    bases[whole] |= 0x20
    some = rng.random(bases.shape) < 0.02
    bases[some] |= 0x20
    for r, c in zip(rng.integers(0, rows, size=40), rng.integers(0, bases.shape[1], size=40)):
        bases[r, c] = ord("N") if r % 2 else ord("n")


@lru_cache(maxsize=None)
def fastq() -> bytes:
    genome = synth.make_genome(100_000, seed=611)
    fq = synth.make_fastq(genome, N_READS, READ_LEN, seed=612, device="cpu").numpy().copy()
    spoil(fq.reshape(N_READS, RB)[:, 11:11 + READ_LEN], np.random.default_rng(613))
    return fq.tobytes()


@lru_cache(maxsize=None)
def fastq_reads():
    rec = np.frombuffer(fastq(), np.uint8).reshape(N_READS, RB)
    return [r[11:11 + READ_LEN].tobytes() for r in rec]


@lru_cache(maxsize=None)
def contigs():
    """a sequence stream's records: 24 contigs of a 3 Mb genome, spoilt like the reads"""
    genome = synth.make_genome(3_000_000, seed=621).copy().reshape(24, -1)
    spoil(genome, np.random.default_rng(622))
    return [row.tobytes() for row in genome]


@lru_cache(maxsize=None)
def window_hashes(source: str, k: int):
    """every window hash of the input, ascending, with its multiplicity (the definition; once per input and k)"""
    seqs = fastq_reads() if source == "fastq" else contigs()
    return mo.bruteforce_sketch(seqs, k, 1 << 62, 1)


def definition(source: str, k: int, s: int, m: int):
    vals, cnts = window_hashes(source, k)
    keep = cnts >= m
    return vals[keep][:s], cnts[keep][:s]


def check(source: str, data: bytes, fmt: int, k: int, s: int, m: int) -> None:
    sk = engine.Sketcher(k, s, m, expected_bytes=len(data))
    sk.push_host(data, fmt)
    got, cnt = sk.finish()
    st = sk.stats()
    sk.close()
    # with the threshold at its initial value every window without an N is admitted: inserts == k-mers but for ~0.1 %
    assert st["launches"] >= 2 and st["inserts"] < 0.9 * st["kmers"], ("no launch ran with a lowered threshold", st)
    ref = mo.Sketcher(k, s, m)
    if fmt == engine.FMT_FASTQ4:
        ref.add_fastx(data)
    else:
        for seq in data.split(b"\n"):
            if seq:
                ref.add_seq(seq)
    want, want_cnt = ref.finish()
    assert np.array_equal(got, want)
    assert np.all(cnt >= want_cnt)          # mash's heap forgets the occurrences of a hash it evicted in between
    def_h, def_c = definition(source, k, s, m)
    assert len(def_h) == s
    assert np.array_equal(got, def_h) and np.array_equal(cnt, def_c)


def seq_stream() -> bytes:
    return b"\n".join(contigs()) + b"\n"


def run_form(form: str) -> None:
    """every case of one kernel form; the caller has forced the form for this process"""
    assert os.environ["MHX_QUEUE_CANDIDATES"] == form
    engine.init(0)
    for k in KS:
        for s, m in (SM_QUEUE if form == "1" else SM_INLINE):
            check("fastq", fastq(), engine.FMT_FASTQ4, k, s, m)
    if form == "0":
        check("seq", seq_stream(), engine.FMT_SEQ, 21, 1000, 1)
    print("ok")


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline", "queue"])
def test_forced_kernel_form_with_a_lowered_threshold(form):
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    code = "from tests.test_gpu_admission_bound import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("s,m", SM_INLINE + SM_QUEUE)
@pytest.mark.parametrize("k", KS)
def test_fastq_sketch_with_the_engines_own_schedule(k, s, m):
    check("fastq", fastq(), engine.FMT_FASTQ4, k, s, m)


def test_sequence_stream_with_the_engines_own_schedule():
    check("seq", seq_stream(), engine.FMT_SEQ, 21, 1000, 1)

"""The hash loop with the strand decision taken from the two views the hash reads (canonical_strand on U and R,
mhx_tile.h) on the device: EVERY window hash of a small input against the C oracle, hashes and multiplicities.

Input: 200 reads of 60..150 bp from a 5 kb genome, one read of 7 bases (shorter than every K) and one of 20: whole reads,
stretches and single bases in lower case, N and n, and reads built around an inverted repeat -- eight bases, a spacer of
K - 16, their reverse complement -- whose window of K bases ties between the strands on its first eight bases, so that the
decision takes its exact path; for every K >= 16 of the list one such window starts at every byte position modulo 8 (every
window J of a group), in the FASTQ and in the sequence stream alike.  The reads as 4-line FASTQ with CR LF line ends, as a
sequence stream, and as a wrapped FASTA through the device's FASTA parser.  The sketch size is above the number of
distinct k-mers: every window's hash and multiplicity lands in the result.

Kernel forms: the engine's own choice in this process; the inline form, the inline form with the first launch split eight
ways (SPLIT) and the queue form each forced in a child process (MHX_QUEUE_CANDIDATES, MHX_FIRST_SPLIT).  The queue form
only ADMITS by the loop's hash, and with the threshold at its maximum it admits everything, so that child also runs the
13 000 reads of tests/test_gpu_admission_bound.py at K = 21 with s = 8192, where launches run behind a lowered threshold
and a hash the loop gets wrong is a hash the sketch loses.  The segmented sketch and the containment screen run once each
at K = 21."""
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
from tests.test_canonical_words import revcomp

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KS = [8, 15, 16, 17, 21, 22, 27, 31, 32]
TIE_KS = [k for k in KS if k >= 16]         # a tie of the first eight bases needs 16 (an odd K below has none)
N_PLAIN, S = 144, 32768
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def _header(i: int, pad: int) -> bytes:
    return b"@r%d" % i + b"x" * pad


@lru_cache(maxsize=None)
def layout():
    """(reads, header paddings, ties): ties[k] = the set of (position in the sequence stream) % 8 at which a window of k
    bases with tied first eight bases starts.  The FASTQ headers are padded so that every read starts at the same position
    modulo 8 in the FASTQ as in the sequence stream."""
    rng = np.random.default_rng(4100)
    genome = synth.make_genome(5_000, seed=4101)
    reads = []
    for _ in range(N_PLAIN):
        n = int(rng.integers(60, 151))
        at = int(rng.integers(0, len(genome) - n + 1))
        r = genome[at:at + n].copy()
        if rng.random() < 0.15:
            r |= 0x20                                                # a whole read in lower case
        if rng.random() < 0.25:
            c = int(rng.integers(0, n - 20))
            r[c:c + 20] |= 0x20                                      # a lower-case stretch
        r[rng.random(n) < 0.03] |= 0x20                              # single lower-case bases
        if rng.random() < 0.08:
            r[int(rng.integers(0, n))] = ord("N") if rng.random() < 0.5 else ord("n")
        reads.append(r.tobytes())
    reads.insert(40, b"ACGTACG")                                     # shorter than every K
    reads.insert(90, genome[100:120].tobytes())                      # shorter than K = 21 and above
    ties = {k: set() for k in TIE_KS}
    at_seq, out = 0, []
    plain = iter(reads)
    for i in range(len(reads) + 8 * len(TIE_KS)):
        tie = i % 3 == 2 and (i // 3) < 8 * len(TIE_KS)
        if tie:
            k, j = TIE_KS[(i // 3) // 8], (i // 3) % 8
            lead = 8 + (j - at_seq - 8) % 8                          # the window starts at stream position = j (mod 8)
            arm = rng.choice(ACGT, size=8).tobytes()
            w = arm + rng.choice(ACGT, size=k - 16).tobytes() + revcomp(arm)
            assert len(w) == k and w[:8] == revcomp(w)[:8]
            r = rng.choice(ACGT, size=lead).tobytes() + w + rng.choice(ACGT, size=int(rng.integers(40, 80))).tobytes()
            if j % 2:
                r = r.lower()
            ties[k].add((at_seq + lead) % 8)
        else:
            r = next(plain)
        out.append(r)
        at_seq += len(r) + 1
    assert next(plain, None) is None and all(t == set(range(8)) for t in ties.values()), ties
    assert all(60 <= len(r) <= 150 for r in out if len(r) > 20) and len(out) == N_PLAIN + 2 + 8 * len(TIE_KS)
    pads, at_seq, at_fq = [], 0, 0
    for i, r in enumerate(out):
        pad = (at_seq - (at_fq + len(_header(i, 0)) + 2)) % 8
        pads.append(pad)
        at_fq += len(_header(i, pad)) + 2
        assert at_fq % 8 == at_seq % 8
        at_fq += 2 * (len(r) + 2) + 3
        at_seq += len(r) + 1
    return out, pads


def reads():
    return layout()[0]


@lru_cache(maxsize=None)
def fastq() -> bytes:
    out, pads = layout()
    return b"".join(_header(i, p) + b"\r\n" + r + b"\r\n+\r\n" + b"I" * len(r) + b"\r\n" for i, (r, p) in enumerate(zip(out, pads)))


@lru_cache(maxsize=None)
def seq_stream() -> bytes:
    return b"\n".join(reads()) + b"\n"


@lru_cache(maxsize=None)
def fasta() -> bytes:
    return b"".join(b">r%d\n" % i + b"".join(r[c:c + 61] + b"\n" for c in range(0, len(r), 61)) for i, r in enumerate(reads()))


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
    sk.close()
    vals, cnts = definition(k)
    assert np.array_equal(got, vals), f"k={k}: {len(got)} hashes, {len(vals)} expected"
    assert np.array_equal(cnt, cnts)


@pytest.mark.parametrize("k", KS)
def test_every_window_hash_of_a_fastq(k):
    data = fastq()
    assert 2 * 16384 < len(data) <= 4 * 16384       # windows cross tile borders and the halo
    check(data, engine.FMT_FASTQ4, k)


@pytest.mark.parametrize("k", KS)
def test_every_window_hash_of_a_sequence_stream(k):
    check(seq_stream(), engine.FMT_SEQ, k)


def test_every_window_hash_of_a_fasta():
    parsed = engine.fasta_stream(fasta())
    assert parsed is not None and len(parsed[1]) >= len(reads()) - 1
    for k in (21, 27):
        check(parsed[0], engine.FMT_SEQ, k)


def run_form(form: str) -> None:
    """one kernel form, forced for this process by the caller"""
    assert os.environ["MHX_QUEUE_CANDIDATES"] == form
    engine.init(0)
    for split in (["1", "8"] if form == "0" else [None]):   # inline: the plain form, then the whole input as one split first launch
        if split is not None:
            os.environ["MHX_FIRST_SPLIT"] = split
        for k in KS:
            check(fastq(), engine.FMT_FASTQ4, k)
            check(seq_stream(), engine.FMT_SEQ, k)
    if form == "1":
        for s, m in big.SM_QUEUE:
            big.check("fastq", big.fastq(), engine.FMT_FASTQ4, 21, s, m)
    print("ok")


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline_and_split", "queue"])
def test_forced_kernel_form(form):
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    env.pop("MHX_FIRST_SPLIT", None)
    code = "from tests.test_gpu_strand_views import run_form; run_form(%r)" % form
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


def test_segmented_sketch_of_every_read():
    k, s = 21, 1000
    genome = synth.make_genome(5_000, seed=4101).tobytes()      # one segment above the cut: the sketcher's route
    segs = reads() + [genome]
    assert len(genome) - k + 1 > engine.sketch_segments_cut()
    data = b"".join(r + b"\n" for r in segs)
    off = np.concatenate([[0], np.cumsum([len(r) + 1 for r in segs])]).astype(np.uint64)
    rows, lens = engine.sketch_segments(data, off, k, s)
    for i, r in enumerate(segs):
        want = mo.bruteforce_sketch([r], k, s, 1)[0]
        assert lens[i] == len(want) and np.array_equal(rows[i, :lens[i]], want), f"segment {i}"


def test_containment_screen_of_the_reads():
    from tests import screen_rule as rule
    from tests.test_gpu_screen import pack

    k, s = 21, 1000
    refs = [mo.bruteforce_sketch([synth.make_genome(5_000, seed=4101).tobytes()], k, s)[0],
            mo.bruteforce_sketch([synth.make_genome(5_000, seed=4102).tobytes()], k, s)[0]]
    rows, lens = pack(refs)
    want = rule.tally(refs, rule.window_hashes([r.upper() for r in reads()], k))
    assert want[0][1] > 0.5 * len(refs[0]) and want[1][1] <= 2
    sc = engine.Screener(k, rows, lens, s, with_set_size=False)
    try:
        sc.push_host(fastq(), engine.FMT_FASTQ4)
        shared, median, _, counts = sc.finish(with_counts=True)
    finally:
        sc.close()
    for i, (c, sh, med) in enumerate(want):
        assert np.array_equal(counts[i, :len(refs[i])], c), f"reference {i}: multiplicities differ"
        assert (int(shared[i]), int(median[i])) == (sh, med), i

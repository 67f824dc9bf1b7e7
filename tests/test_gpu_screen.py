"""The containment screen (`mash screen`) on the GPU against the plain statement of its rule (tests/screen_rule.py): per-entry
multiplicities, shared, median and set size exactly, the identity column as text, the p column to the resolution of %g.
Buffer level on synthetic genomes (a clade, an unrelated genome, a small genome whose sketch is not full), file level on
the reference's fixtures and on every ingest route, and the `mash screen` command of the shim."""
import ctypes
import gzip
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from auriclass_amd import engine, mash_shim, synth
from oracle import mash_oracle as mo
from tests import screen_rule as rule
from tests.conftest import REFDATA

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------- inputs
def sketch_of(genome: np.ndarray, k: int, s: int) -> np.ndarray:
    return mo.bruteforce_sketch([genome.tobytes()], k, s)[0]


def pack(refs):
    stride = max(1, max(len(r) for r in refs))
    rows = np.zeros((len(refs), stride), dtype=np.uint64)
    for i, r in enumerate(refs):
        rows[i, :len(r)] = r
    return rows, np.array([len(r) for r in refs], dtype=np.uint32)


_CACHE = {}


def scenario(k: int, s: int, with_small: bool = True, genome_len: int = 100_000, coverage: int = 20):
    """references: a genome, two mutated copies (a clade), an unrelated genome, (a 5 kb genome: sketch not full for
    s = 50 000, T_screen high in either case); reads: ~20x of the first genome with errors, as many of the unrelated"""
    key = (k, s, with_small, genome_len, coverage)
    if key not in _CACHE:
        a = synth.make_genome(genome_len, seed=101)
        b = synth.make_genome(genome_len, seed=202)
        genomes = [a, synth.mutate(a, 0.002, 7), synth.mutate(a, 0.01, 8), b]
        if with_small:
            genomes.append(synth.make_genome(5_000, seed=303))
        n_reads = genome_len * coverage // 150
        own = synth.make_fastq(a, n_reads, 150, seed=11, sub_rate=0.01).numpy().tobytes()
        foreign = synth.make_fastq(b, n_reads, 150, seed=12, sub_rate=0.01, first_index=n_reads).numpy().tobytes()
        _CACHE.clear()   # one scenario in memory at a time
        _CACHE[key] = ([sketch_of(g, k, s) for g in genomes], own, foreign)
    return _CACHE[key]


def expectation(refs, k, s_ref, records, set_size_sketcher=None):
    h = rule.window_hashes(records, k)
    if set_size_sketcher is None:
        set_size_sketcher = mo.Sketcher(k, s_ref, 1)
        set_size_sketcher.add_fastx(as_fastq(records))
    return rule.tally(refs, h), set_size_sketcher.set_size


def check_result(refs, k, got, want, set_size_want):
    shared, median, set_size, counts = got
    assert set_size == set_size_want, (set_size, set_size_want)
    for i, (c, sh, med) in enumerate(want):
        assert np.array_equal(counts[i, :len(refs[i])], c), f"reference {i}: multiplicities differ"
        assert not counts[i, len(refs[i]):].any()
        assert (int(shared[i]), int(median[i])) == (sh, med), i
        n = len(refs[i])
        assert mo.fmt_g(engine.screen_identity(sh, n, k)) == mo.fmt_g(rule.identity(sh, n, k))
        assert rule.same_to_the_sixth_digit(engine.screen_p_value(sh, n, set_size, k), rule.p_value(sh, n, set_size_want, k))


def seq_stream(records):
    return b"\n".join(records) + b"\n"


# ---------------------------------------------------------------------------------------------- buffer level
@pytest.mark.parametrize("s", [1000, 50_000])
@pytest.mark.parametrize("k", [5, 16, 17, 21, 27, 32])
def test_buffer_level_mixture_both_formats(k, s):
    refs, own, foreign = scenario(k, s)
    rows, lens = pack(refs)
    fastq = own + foreign
    records = rule.fastq4_records(fastq)
    osk = mo.Sketcher(k, s, 1)
    osk.add_fastx(fastq)
    want, size = expectation(refs, k, s, records, osk)
    assert want[0][1] > 0.9 * len(refs[0]) or k == 5
    sc = engine.Screener(k, rows, lens, s)
    try:
        # one push of host bytes, 4-line FASTQ
        sc.push_host(fastq, engine.FMT_FASTQ4)
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        # reset and reuse: the same bytes as a sequence stream from device memory, in three pushes cut at record ends
        sc.reset()
        stream = seq_stream(records)
        cuts = [0, stream.index(b"\n", len(stream) // 3) + 1, stream.index(b"\n", 2 * len(stream) // 3) + 1, len(stream)]
        dev = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
        for lo, hi in zip(cuts, cuts[1:]):
            sc.push_device(dev.data_ptr() + lo, hi - lo, engine.FMT_SEQ, keep=dev)
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        # a second finish() after more pushes: everything counted twice, the set size unchanged
        sc.push_host(fastq, engine.FMT_FASTQ4)
        shared, median, size2, counts = sc.finish(with_counts=True)
        assert size2 == size
        for i, (c, sh, med) in enumerate(want):
            assert np.array_equal(counts[i, :len(refs[i])], 2 * c) and int(shared[i]) == sh
    finally:
        sc.close()


@pytest.mark.parametrize("k,s,genome_len", [(21, 1000, 4_000_000), (27, 50_000, 1_000_000), (16, 1000, 300_000)])
def test_low_candidate_rate_regimes(k, s, genome_len):
    """full sketches of large genomes only: T_screen / 2^64 = s / genome -- 2.5e-4 (inline form by the rule), 0.05 (queue
    form, large sketch), 3e-3 (queue form, small sketch); many device pushes of FASTQ from one buffer"""
    a = synth.make_genome(genome_len, seed=5)
    refs = [sketch_of(a, k, s), sketch_of(synth.mutate(a, 0.005, 6), k, s), sketch_of(synth.make_genome(genome_len, seed=9), k, s)]
    rows, lens = pack(refs)
    n_reads = 60_000
    fastq = synth.make_fastq(a, n_reads, 150, seed=21, sub_rate=0.005).numpy().tobytes()
    records = rule.fastq4_records(fastq)
    osk = mo.Sketcher(k, s, 1)
    osk.add_fastx(fastq)
    want, size = expectation(refs, k, s, records, osk)
    assert want[0][1] > 0 and want[2][1] <= 2
    rb = synth.record_bytes(150)
    dev = torch.frombuffer(bytearray(fastq), dtype=torch.uint8).cuda()
    sc = engine.Screener(k, rows, lens, s)
    try:
        cuts = [0, 1, 7, 1000, 1001, 30_000, n_reads]   # records: spans of one record up to tens of thousands
        for lo, hi in zip(cuts, cuts[1:]):
            sc.push_device(dev.data_ptr() + lo * rb, (hi - lo) * rb, engine.FMT_FASTQ4, keep=dev)
        sc.sync()
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        # without the set-size sketch: same tallies, set size reported as 0
        bare = engine.Screener(k, rows, lens, s, with_set_size=False)
        bare.push_device(dev.data_ptr(), len(fastq), engine.FMT_FASTQ4, keep=dev)
        shared, median, size0, _ = bare.finish()
        bare.close()
        assert size0 == 0.0
        assert [int(x) for x in shared] == [w[1] for w in want] and [int(x) for x in median] == [w[2] for w in want]
    finally:
        sc.close()


def messy_records(genome: np.ndarray, seed: int):
    """reads shorter than k, ordinary ones, N / IUPAC / lower case, long reads (> 2.7 kb: the repair pass) and lines longer
    than a tile (16 KiB)"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(400):
        kind = i % 8
        length = {0: 150, 1: int(rng.integers(1, 40)), 2: 150, 3: 3000 + int(rng.integers(0, 500)), 4: 250, 5: 20_000, 6: 150, 7: 75}[kind]
        if kind == 5 and i > 120:
            length = 150
        start = int(rng.integers(0, len(genome) - length))
        seq = bytearray(genome[start:start + length].tobytes())
        if kind == 2:
            for p in rng.integers(0, length, size=3):
                seq[p] = ord("N")
        if kind == 4:
            seq = bytearray(bytes(seq).lower())
            seq[100] = ord("R")
        if kind == 6:
            seq[10:60] = bytes(seq[10:60]).lower()
            seq[120] = ord("y")
        recs.append(bytes(seq))
    return recs


def as_fastq(recs, eol=b"\n"):
    return b"".join(b"@m%d" % i + eol + r + eol + b"+" + eol + b"I" * len(r) + eol for i, r in enumerate(recs))


@pytest.mark.parametrize("k,s", [(16, 1000), (21, 1000), (32, 50_000)])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_messy_reads_long_lines_and_push_patterns(k, s, eol):
    refs, _, _ = scenario(k, s)
    rows, lens = pack(refs)
    a = synth.make_genome(100_000, seed=101)
    recs = messy_records(a, seed=k)
    want, size = expectation(refs, k, s, recs)
    assert want[0][1] > 50
    sc = engine.Screener(k, rows, lens, s)
    try:
        fq = as_fastq(recs, eol)
        sc.push_host(fq, engine.FMT_FASTQ4)                    # one push
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        sc.reset()
        parts = [as_fastq(recs[i:i + 37], eol) for i in range(0, len(recs), 37)]
        dev = [torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() for p in parts]
        for i, (p, d) in enumerate(zip(parts, dev)):            # many pushes, host and device pointers in turn
            if i % 2:
                sc.push_host(p, engine.FMT_FASTQ4)
            else:
                sc.push_device(d.data_ptr(), len(p), engine.FMT_FASTQ4, keep=d)
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        sc.reset()
        sc.push_host(seq_stream(recs), engine.FMT_SEQ)          # the same records as a sequence stream
        check_result(refs, k, sc.finish(with_counts=True), want, size)
    finally:
        sc.close()


def test_empty_input_and_reads_without_a_kmer():
    k, s = 21, 1000
    refs, _, _ = scenario(k, s)
    rows, lens = pack(refs)
    sc = engine.Screener(k, rows, lens, s)
    try:
        for feed in (None, as_fastq([b"ACGTACGTAC", b"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN", b""])):
            sc.reset()
            if feed:
                sc.push_host(feed, engine.FMT_FASTQ4)
            shared, median, size, counts = sc.finish(with_counts=True)
            assert size == 0.0 and not shared.any() and not median.any() and not counts.any()
            for n in lens:
                assert mo.fmt_g(engine.screen_identity(0, int(n), k)) == "0" and engine.screen_p_value(0, int(n), size, k) == 1.0
    finally:
        sc.close()


def test_reference_set_edge_shapes():
    """an empty reference, a one-entry reference, duplicates across references, 32-bit hashes"""
    k, s = 16, 1000
    refs, own, _ = scenario(k, s)
    refs = [refs[0], np.zeros(0, np.uint64), refs[0][5:6], refs[1], refs[0][::2]]
    rows, lens = pack(refs)
    records = rule.fastq4_records(own)
    want, size = expectation(refs, k, s, records)
    sc = engine.Screener(k, rows, lens, s)
    try:
        sc.push_host(own, engine.FMT_FASTQ4)
        check_result(refs, k, sc.finish(with_counts=True), want, size)
        assert want[1][1] == 0 and want[2][1] <= 1
    finally:
        sc.close()


@pytest.mark.parametrize("k", [5, 16, 21, 27])
def test_contaminating_reads_do_not_lower_containment_but_raise_the_mash_distance(k):
    """the point of the feature: reads of another organism leave `shared` of the true reference where it was (never
    lower; for k >= 21, where a chance hit of the foreign genome on one of s reference hashes does not happen for these
    seeds -- the plain statement below says so --, exactly where it was), while the Mash distance of the read set's
    bottom-s sketch to that reference rises"""
    s = 1000
    refs, own, foreign = scenario(k, s)
    rows, lens = pack(refs)
    pure_want, _ = expectation(refs, k, s, rule.fastq4_records(own))
    mix_want, _ = expectation(refs, k, s, rule.fastq4_records(own + foreign))
    if k >= 21:
        assert pure_want[0][1] == mix_want[0][1]            # the statement itself: no chance hits for these seeds
    sc = engine.Screener(k, rows, lens, s)
    try:
        sc.push_host(own, engine.FMT_FASTQ4)
        pure = sc.finish()[0].copy()
        sc.reset()
        sc.push_host(own + foreign, engine.FMT_FASTQ4)
        mixed = sc.finish()[0].copy()
    finally:
        sc.close()
    assert [int(x) for x in pure] == [w[1] for w in pure_want] and [int(x) for x in mixed] == [w[1] for w in mix_want]
    assert int(mixed[0]) >= int(pure[0])
    if k < 21:
        return
    assert int(mixed[0]) == int(pure[0])
    dist = []
    for data in (own, own + foreign):
        sk = engine.Sketcher(k, s, 1, expected_bytes=len(data))
        sk.push_host(data, engine.FMT_FASTQ4)
        h, _ = sk.finish()
        sk.close()
        q = np.zeros((1, rows.shape[1]), dtype=np.uint64)
        q[0, :len(h)] = h
        dist.append(engine.dist_batch(q, np.array([len(h)], np.uint32), rows[:1], lens[:1], k, s)[2][0, 0])
    assert dist[1] > dist[0], dist


FORMS_CHILD = r"""
import sys
import numpy as np
from auriclass_amd import engine
from tests import screen_rule as rule
from tests.test_gpu_screen import scenario, pack, expectation, check_result, messy_records, as_fastq, seq_stream
from auriclass_amd import synth
for k, s, glen in ((16, 1000, 100_000), (27, 50_000, 2_000_000)):
    # (16, 1000) with the 5 kb reference: every fifth window a candidate; (27, 50 000) on 2 Mb genomes: one in forty
    refs, own, foreign = scenario(k, s, with_small=(k == 16), genome_len=glen, coverage=2)
    rows, lens = pack(refs)
    recs = rule.fastq4_records(own) + messy_records(synth.make_genome(100_000, seed=101), seed=3)
    want, size = expectation(refs, k, s, recs)
    sc = engine.Screener(k, rows, lens, s)
    sc.push_host(as_fastq(recs), engine.FMT_FASTQ4)
    check_result(refs, k, sc.finish(with_counts=True), want, size)
    sc.reset()
    sc.push_host(seq_stream(recs), engine.FMT_SEQ)
    check_result(refs, k, sc.finish(with_counts=True), want, size)
    sc.close()
print("ok")
"""


@pytest.mark.parametrize("form", ["0", "1"], ids=["inline", "queue"])
def test_both_kernel_forms(form):
    """MHX_QUEUE_CANDIDATES forces the form of every launch (read once per process: a child process each); the queue form
    with the small reference among the references overflows its queue and takes the generic routine"""
    env = dict(os.environ, MHX_QUEUE_CANDIDATES=form, PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-c", FORMS_CHILD], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- file level
REF = REFDATA / "ref_sketch.msh"


def file_expectation(paths, ref=None):
    ref = ref or mo.read_msh(REF)
    k, s = ref.kmer_size, ref.sketch_size
    data = [mo.read_maybe_gz(p) for p in paths]
    osk = mo.Sketcher(k, s, 1)
    for d in data:
        osk.add_fastx(d)
    records = sum((rule.fastx_records(d) for d in data), [])
    return ref, rule.tally([r.hashes for r in ref.references], rule.window_hashes(records, k)), osk.set_size


def check_text(text, size, ref, want, size_want):
    assert size == size_want
    rows = rule.rows_of_text(text)
    assert len(rows) == len(ref.references)
    k = ref.kmer_size
    for (ident, sh, n, med, p, name, comment), r, (c, sh_w, med_w) in zip(rows, ref.references, want):
        assert (sh, n, med, name, comment) == (sh_w, len(r.hashes), med_w, r.name, r.comment)
        assert ident == mo.fmt_g(rule.identity(sh_w, n, k))
        assert rule.same_to_the_sixth_digit(p, float(mo.fmt_g(rule.p_value(sh_w, n, size_want, k))))


PAIR = [REFDATA / "NC_001416.1_1.fq.gz", REFDATA / "NC_001416.1_2.fq.gz"]


def test_fixture_pair_against_the_reference_sketch(tmp_path):
    """lambda reads against {lambda, T7} at k = 27, s = 50 000: both sketches are short of s, every window probes"""
    ref, want, size_want = file_expectation(PAIR)
    assert (want[0][1], want[0][2], want[1][1]) == (48466, 39, 0) and size_want == 154153.32037587647
    text, size = engine.screen_files(REF, PAIR)
    check_text(text, size, ref, want, size_want)
    assert text.splitlines()[0].startswith("0.999992\t48466/48476\t39\t0\t") and text.splitlines()[1].startswith("0\t0/39770\t0\t1\t")
    assert engine.last_fastq_route() == "device-streamed"
    # the set size is the estimated genome size of a reads-mode sketch with m = 1, bit for bit
    _, est = engine.sketch_files(PAIR, ref.kmer_size, ref.sketch_size, tmp_path / "m.msh", reads=True, min_mult=1)
    assert size == est
    # the shim prints the same rows; flags it does not serve are refused
    assert shim_stdout(["screen", str(REF)] + [str(p) for p in PAIR]) == (0, text)
    assert shim_stdout(["screen", "-p", "8", str(REF)] + [str(p) for p in PAIR]) == (0, text)
    for flag in ("-w", "-i", "-v", "-a"):
        extra = [flag] if flag in ("-w", "-a") else [flag, "0.5"]
        assert shim_stdout(["screen"] + extra + [str(REF), str(PAIR[0])])[0] == 1
    assert shim_stdout(["screen", str(REF)])[0] == 1
    assert shim_stdout(["screen", str(tmp_path / "none.msh"), str(PAIR[0])])[0] == 1
    assert "screen" in mash_shim.USAGE


def shim_stdout(argv):
    import contextlib
    import io

    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = mash_shim.main(argv)
    return rc, out.getvalue()


def test_plain_gz_bgzf_single_and_whole_file_routes(tmp_path, monkeypatch):
    from tests.test_lib_cpu import _bgzf

    raw = [mo.read_maybe_gz(p) for p in PAIR]
    plain = [tmp_path / "r1.fq", tmp_path / "r2.fq"]
    for p, d in zip(plain, raw):
        p.write_bytes(d)
    bg = tmp_path / "r1.bgzf.fq.gz"
    bg.write_bytes(_bgzf(raw[0], 6))
    gz = tmp_path / "r2.fq.gz"
    gz.write_bytes(gzip.compress(raw[1], 1))
    for paths in ([plain[0]], plain, [bg], [bg, gz], [plain[0], gz]):
        ref, want, size_want = file_expectation(paths)
        text, size = engine.screen_files(REF, paths)
        check_text(text, size, ref, want, size_want)
        assert engine.last_fastq_route() == "device-streamed"
    monkeypatch.setenv("MHX_NO_STREAMING", "1")
    ref, want, size_want = file_expectation(plain)
    text, size = engine.screen_files(REF, plain)
    check_text(text, size, ref, want, size_want)
    assert engine.last_fastq_route() == "device-whole"


def test_fasta_assembly_as_the_read_set():
    paths = [REFDATA / "NC_001416.1.fasta.gz"]
    ref, want, size_want = file_expectation(paths)
    assert want[0][1] == len(ref.references[0].hashes) and want[0][2] == 1
    text, size = engine.screen_files(REF, paths)
    check_text(text, size, ref, want, size_want)
    assert text.startswith("1\t48476/48476\t1\t0\t")
    assert engine.last_fastq_route() == "record-parser"
    both = [REFDATA / "NC_001416.1.fasta.gz", REFDATA / "NC_001604.1.fasta.gz"]
    ref, want, size_want = file_expectation(both)
    text, size = engine.screen_files(REF, both)
    check_text(text, size, ref, want, size_want)
    assert [r[1] == r[2] for r in rule.rows_of_text(text)] == [True, True]


def test_damaged_fastq_goes_to_the_record_parser_and_ends_as_the_sketch_call(tmp_path):
    raw = mo.read_maybe_gz(PAIR[0])
    lines = raw.split(b"\n")
    mid = (len(lines) // 8) * 4 + 3                      # a quality line in the middle, one byte short
    lines[mid] = lines[mid][:-1]
    bad = tmp_path / "short_quality.fq"
    bad.write_bytes(b"\n".join(lines))

    def outcome(call):
        try:
            return ("ok", call()[1])
        except engine.EngineError as e:
            return (e.code, e.message)

    sketch_end = outcome(lambda: engine.sketch_files([bad], 27, 50_000, tmp_path / "x.msh", reads=True, min_mult=1))
    sketch_route = engine.last_fastq_route()
    screen_end = outcome(lambda: engine.screen_files(REF, [bad]))
    assert screen_end == sketch_end                      # the record parser's verdict (mash: truncated quality string), or its set size
    assert engine.last_fastq_route() == sketch_route == "record-parser"
    osk = mo.Sketcher(27, 50_000, 1)
    try:
        osk.add_fastx(bad.read_bytes())
        assert sketch_end == ("ok", osk.set_size)
    except ValueError:
        assert sketch_end[0] == engine.MHX_E_FORMAT


def test_errors_and_the_two_call_text_pattern(tmp_path):
    ref = mo.read_msh(REF)
    other_seed = tmp_path / "seed7.msh"
    mo.write_msh(other_seed, mo.SketchFile(kmer_size=27, sketch_size=50_000, references=ref.references, hash_seed=7))
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(other_seed, PAIR)
    assert e.value.code == engine.MHX_E_MISMATCH
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(tmp_path / "missing.msh", PAIR)
    assert e.value.code == engine.MHX_E_IO
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(REF, [PAIR[0], tmp_path / "missing.fq.gz"])
    assert e.value.code == engine.MHX_E_IO
    with pytest.raises(engine.EngineError) as e:
        engine.screen_files(REF, [PAIR[0], tmp_path / "missing.fq"])
    assert e.value.code == engine.MHX_E_IO
    # cap = 0 reports the size, a buffer that is too small MHX_E_CAPACITY and the size, the right one the text
    L = engine.load()
    want_text, _ = engine.screen_files(REF, PAIR[:1])
    arr = (ctypes.c_char_p * 1)(os.fsencode(str(PAIR[0])))
    need, size = ctypes.c_size_t(0), ctypes.c_double(0)
    assert L.mhx_screen_files(os.fsencode(str(REF)), arr, 1, None, 0, ctypes.byref(need), ctypes.byref(size)) == engine.MHX_OK
    assert need.value == len(want_text.encode()) + 1
    small = ctypes.create_string_buffer(16)
    need2 = ctypes.c_size_t(0)
    assert L.mhx_screen_files(os.fsencode(str(REF)), arr, 1, small, 16, ctypes.byref(need2), None) == engine.MHX_E_CAPACITY
    assert need2.value == need.value
    buf = ctypes.create_string_buffer(need.value)
    assert L.mhx_screen_files(os.fsencode(str(REF)), arr, 1, buf, need.value, ctypes.byref(need2), None) == engine.MHX_OK
    assert buf.value.decode() == want_text


def test_read_set_without_records_succeeds_with_zero_rows(tmp_path):
    empty = [REFDATA / "test_empty_1.fq.gz", REFDATA / "test_empty_2.fq.gz"]
    with pytest.raises(engine.NoRecordsError):
        engine.sketch_files(empty, 27, 50_000, tmp_path / "e.msh", reads=True, min_mult=1)
    text, size = engine.screen_files(REF, empty)
    assert size == 0.0
    ref = mo.read_msh(REF)
    assert text == "".join("0\t0/%d\t0\t1\t%s\t%s\n" % (len(r.hashes), r.name, r.comment) for r in ref.references)
    short = tmp_path / "short.fq"
    short.write_bytes(as_fastq([b"ACGTACGTACGT", b"GGGGG"]))
    assert engine.screen_files(REF, [short]) == (text, 0.0)


def test_synthetic_reference_file_with_full_sketches(tmp_path):
    """a reference file of full sketches (low candidate rate) through the file-level call, plain and .gz reads as one set"""
    k, s = 21, 1000
    a, b = synth.make_genome(1_000_000, seed=31), synth.make_genome(1_000_000, seed=32)
    genomes = {"a.fa": a, "a_mut.fa": synth.mutate(a, 0.003, 33), "b.fa": b}
    refs = [mo.Reference(name, "synthetic", len(g), sketch_of(g, k, s)) for name, g in genomes.items()]
    msh = tmp_path / "refs.msh"
    mo.write_msh(msh, mo.SketchFile(kmer_size=k, sketch_size=s, references=refs))
    r1, r2 = tmp_path / "s_1.fq", tmp_path / "s_2.fq.gz"
    r1.write_bytes(synth.make_fastq(a, 40_000, 150, seed=41).numpy().tobytes())
    r2.write_bytes(gzip.compress(synth.make_fastq(b, 20_000, 150, seed=42).numpy().tobytes(), 1))
    ref, want, size_want = file_expectation([r1, r2], mo.read_msh(msh))
    assert want[0][1] > 900 and want[2][1] > 700
    text, size = engine.screen_files(msh, [r1, r2])
    check_text(text, size, ref, want, size_want)
    _, est = engine.sketch_files([r1, r2], k, s, tmp_path / "m.msh", reads=True, min_mult=1)
    assert size == est

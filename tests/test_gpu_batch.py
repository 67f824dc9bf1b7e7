"""Batch mode on the GPU: `mash dist` with several query files in one call (engine.dist_files_multi) against the single
calls and the CPU oracle, and `python -m auriclass_amd.batch` against the single-sample command run in the same process
-- every report compared as bytes, failures included.  Synthetic inputs are small (genomes of 200 kb) and seeded: these
tests check bytes, not speed."""
import gzip
import itertools
from pathlib import Path

import pytest

from auriclass_amd import batch, engine, synth
from auriclass_amd.main import main
from oracle import mash_oracle as mo
from tests.conftest import REFDATA

pytestmark = pytest.mark.gpu

READS = ["tests/data/NC_001416.1_1.fq.gz", "tests/data/NC_001416.1_2.fq.gz"]
ASSEMBLY = "tests/data/NC_001416.1.fasta.gz"
REF = "tests/data/ref_sketch.msh"
FIXTURE_OPTIONS = ["-r", REF, "-c", "tests/data/clade_config.csv", "--expected_genome_size", "40000", "60000"]
FASTQ_ROWS = ("tests/data/NC_001416.1.fasta\ttests/data/NC_001416.1_1.fq.gz\t9.55405e-06\t0\t48451/48476\n"
              "tests/data/NC_001604.1.fasta\ttests/data/NC_001416.1_1.fq.gz\t1\t1\t0/50000\n")


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.init(0)


def write_fasta(path, genome, name="contig"):
    Path(path).write_bytes(synth.genome_fasta(genome, n_contigs=4, name=name))
    return str(path)


def write_read_pair(stem, genome, seed, coverage=30, read_len=150):
    """Reads at `coverage` over the genome, half of them in each of <stem>_1.fq.gz / <stem>_2.fq.gz."""
    n = coverage * len(genome) // read_len
    n -= n % 2
    data = synth.make_fastq(genome, n, read_len, seed=seed, device="cpu").numpy().tobytes()
    half = (n // 2) * synth.record_bytes(read_len)
    paths = [f"{stem}_1.fq.gz", f"{stem}_2.fq.gz"]
    Path(paths[0]).write_bytes(gzip.compress(data[:half], compresslevel=1))
    Path(paths[1]).write_bytes(gzip.compress(data[half:], compresslevel=1))
    return paths


def write_sheet(path, samples):
    Path(path).write_text("".join("\t".join([name, *files]) + "\n" for name, files in samples))
    return str(path)


def single_run(name, files, options, out_dir="single"):
    """The single-sample command for one sample, in this process: its report bytes, or the exception it raises."""
    Path(out_dir).mkdir(exist_ok=True)
    report = Path(out_dir) / f"{name}.tsv"
    try:
        main([*files, "-n", name, "-o", str(report), "--log_file_path", str(Path(out_dir) / f"{name}.log"), *options])
    except Exception as exc:
        return exc
    return report.read_bytes()


def data_lines(path):
    lines = Path(path).read_bytes().split(b"\n")
    assert lines[-1] == b""
    return lines[1:-1]


# ---- 1. several query files in one distance call ----------------------------------------------------------------------
def test_multi_query_distances_equal_the_single_calls_and_the_oracle(refcwd):
    engine.sketch_files(READS, 27, 50_000, "a.msh", reads=True, min_mult=3)
    engine.sketch_files([ASSEMBLY], 27, 50_000, "b.msh")
    engine.sketch_files(["tests/data/NC_001416.1.fasta", "tests/data/NC_001604.1.fasta"], 27, 50_000, "c.msh")
    files = ["a.msh", "b.msh", "c.msh"]
    single = {f: engine.dist_files(REF, f) for f in files}
    ref = mo.read_msh(REF)
    for f in files:
        assert single[f] == mo.dist_text(ref, mo.read_msh(f)), f
    assert single["a.msh"] == FASTQ_ROWS
    assert [len(single[f].splitlines()) for f in files] == [2, 2, 4]
    for order in itertools.permutations(files):
        assert engine.dist_files_multi(REF, list(order)) == "".join(single[f] for f in order), order
    assert engine.dist_files_multi(REF, ["c.msh"]) == single["c.msh"]
    assert engine.dist_files_multi(REF, ["b.msh", "b.msh"]) == single["b.msh"] * 2

    def after_a_refusal():
        assert engine.dist_files(REF, "a.msh") == FASTQ_ROWS
        assert engine.dist_files_multi(REF, ["a.msh"]) == FASTQ_ROWS

    # a query of another k
    engine.sketch_files([ASSEMBLY], 21, 50_000, "k21.msh")
    with pytest.raises(engine.EngineError) as alone:
        engine.dist_files(REF, "k21.msh")
    assert alone.value.code == engine.MHX_E_MISMATCH
    with pytest.raises(engine.EngineError) as multi:
        engine.dist_files_multi(REF, ["a.msh", "k21.msh", "c.msh"])
    assert (multi.value.code, multi.value.message) == (alone.value.code, alone.value.message)
    after_a_refusal()
    # an unreadable path in the middle
    with pytest.raises(engine.EngineError) as alone:
        engine.dist_files(REF, "nope.msh")
    with pytest.raises(engine.EngineError) as multi:
        engine.dist_files_multi(REF, ["a.msh", "nope.msh", "c.msh"])
    assert (multi.value.code, multi.value.message) == (alone.value.code, alone.value.message)
    assert "nope.msh" in multi.value.message
    after_a_refusal()
    # query files of different sketch sizes
    engine.sketch_files([ASSEMBLY], 27, 1000, "s1000.msh")
    assert len(engine.dist_files(REF, "s1000.msh").splitlines()) == 2
    with pytest.raises(engine.EngineError) as multi:
        engine.dist_files_multi(REF, ["a.msh", "s1000.msh"])
    assert multi.value.code == engine.MHX_E_MISMATCH
    after_a_refusal()
    # no query at all
    with pytest.raises(engine.EngineError) as multi:
        engine.dist_files_multi(REF, [])
    assert multi.value.code == engine.MHX_E_ARG
    after_a_refusal()


# ---- 2. a batch large enough to leave the generic kernel --------------------------------------------------------------
def test_96_query_files_against_24_references_take_the_batched_kernels(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    base = synth.make_genome(200_000, seed=11)
    refs = [write_fasta(f"ref{i:02d}.fasta", synth.mutate(base, 0.002 * i, seed=100 + i)) for i in range(24)]
    engine.sketch_files(refs, 27, 50_000, "refs.msh")
    assert len(mo.read_msh("refs.msh").references) == 24
    queries = []
    for i in range(96):
        fasta = write_fasta(f"q{i:02d}.fasta", synth.mutate(base, 0.0005 * (i + 1), seed=200 + i))
        engine.sketch_files([fasta], 27, 50_000, f"q{i:02d}.msh")
        queries.append(f"q{i:02d}.msh")
    assert len(mo.read_msh(queries[0]).references[0].hashes) == 50_000
    singles = [engine.dist_files("refs.msh", q) for q in queries]
    assert all(len(t.splitlines()) == 24 for t in singles)
    text = engine.dist_files_multi("refs.msh", queries)
    blocks = engine.load().mhx_last_dist_fallback_blocks()
    print("fallback blocks of the 96 x 24 call:", blocks)
    assert text == "".join(singles)
    assert blocks >= 0   # -1: the pair kernel did everything, i.e. nothing was batched
    assert singles[0] == mo.dist_text(mo.read_msh("refs.msh"), mo.read_msh(queries[0]))
    assert len({t.split("\t")[2] for t in text.splitlines()}) > 100   # (the distances are not all alike)


# ---- 3. the reference's reports -----------------------------------------------------------------------------------------
def test_batch_writes_the_references_reports(refcwd):
    sheet = write_sheet("fq.tsv", [("isolate", READS)])
    assert batch.main([sheet, "-O", "out_fq", *FIXTURE_OPTIONS, "--log_file_path", "fq.log", "--verbose"]) == 0
    want = (REFDATA / "reference_report_fastq.tsv").read_bytes()
    assert Path("out_fq/report.isolate.tsv").read_bytes() == want
    assert Path("out_fq/report.tsv").read_bytes() == want
    assert Path("out_fq/failed.tsv").read_text() == "Sample\tError\tMessage\n"
    log = Path("fq.log").read_text()
    assert "[isolate] [mash sketch] Estimated genome size: 48454.7" in log and "[mash dist] mash dist" in log
    sheet = write_sheet("fa.tsv", [("isolate", [ASSEMBLY])])
    assert batch.main([sheet, "-O", "out_fa", *FIXTURE_OPTIONS, "--log_file_path", "fa.log"]) == 0
    want = (REFDATA / "reference_report_fasta.tsv").read_bytes()
    assert Path("out_fa/report.isolate.tsv").read_bytes() == want
    assert Path("out_fa/report.tsv").read_bytes() == want
    # before anything runs: a broken sheet, a missing reference sketch
    with pytest.raises(ValueError, match="line 2"):
        batch.main([write_sheet("bad.tsv", [("a", [ASSEMBLY]), ("a", READS)]), "-O", "out_bad", *FIXTURE_OPTIONS, "--log_file_path", "x.log"])
    with pytest.raises(FileNotFoundError):
        batch.main([sheet, "-O", "out_bad", "-r", "tests/data/nope.msh", "-c", "tests/data/clade_config.csv", "--log_file_path", "x.log"])
    assert not Path("out_bad/report.tsv").exists()


# ---- 4. batch = the single runs -----------------------------------------------------------------------------------------
def test_mixed_batch_equals_the_single_runs_byte_for_byte(refcwd):
    """Assemblies and 30x read pairs of mutated copies of one 200 kb genome against three references (clade I, clade II,
    outgroup) built here: the single-sample reports cover PASS, WARN, FAIL by species and FAIL by other Candida, and the
    batch writes the same bytes for every sample, with the default group size and with groups of 3."""
    base = synth.make_genome(200_000, seed=1)
    clade2 = synth.mutate(base, 0.01, seed=2)
    outgroup = synth.mutate(base, 0.05, seed=3)
    refs = [write_fasta("ref_I.fasta", base), write_fasta("ref_II.fasta", clade2), write_fasta("ref_out.fasta", outgroup)]
    engine.sketch_files(refs, 27, 50_000, "refs.msh")
    Path("clades.csv").write_text("filename,clade\nref_I.fasta,I\nref_II.fasta,II\nref_out.fasta,outgroup\n")
    genomes = {
        "near_I": synth.mutate(base, 0.0005, seed=4),       # PASS (clade I)
        "far_I": synth.mutate(base, 0.005, seed=5),         # WARN (high distance)
        "near_out": synth.mutate(outgroup, 0.001, seed=6),  # FAIL (other Candida)
        "unrelated": synth.make_genome(200_000, seed=7),    # FAIL (species)
        "near_II": synth.mutate(clade2, 0.0005, seed=8),    # PASS (clade II)
    }
    samples = [("phage_reads", READS), ("phage_assembly", [ASSEMBLY])]
    for name, genome in genomes.items():
        samples.append((f"asm_{name}", [write_fasta(f"{name}.fasta", genome, name=name)]))
    # two files, one sample: 200 000 + 39 937 bases miss the expected genome size -> WARN
    samples.append(("two_files", ["near_I.fasta", "tests/data/NC_001604.1.fasta"]))
    for i, name in enumerate(("near_I", "far_I", "near_out", "near_II")):
        samples.append((f"reads_{name}", write_read_pair(f"reads_{name}", genomes[name], seed=50 + i)))
    assert len(samples) == 12
    options = ["-r", "refs.msh", "-c", "clades.csv", "--expected_genome_size", "150000", "230000"]

    singles = {name: single_run(name, files, options) for name, files in samples}
    for name, got in singles.items():
        assert isinstance(got, bytes), (name, got)
    rows = {name: got.decode().splitlines()[1].split("\t") for name, got in singles.items()}
    for name, row in rows.items():
        print(name, row)
    decisions = {name: row[3] for name, row in rows.items()}
    assert {"PASS", "WARN", "FAIL"} <= set(decisions.values())
    assert any(row[4].startswith("FAIL") for row in rows.values())                                # qc_species
    assert any(row[5].startswith("FAIL") for row in rows.values())                                # qc_other_candida
    assert any(row[6].startswith("WARN") for row in rows.values())                                # the genome size one sample misses
    # the assemblies, as the recipe was checked with the CPU oracle
    assert [decisions[f"asm_{n}"] for n in genomes] == ["PASS", "WARN", "FAIL", "FAIL", "PASS"]
    assert rows["asm_near_I"][1] == "I" and rows["asm_near_II"][1] == "II"
    assert rows["asm_near_out"][1] == "other Candida/CUG-Ser1 clade sp." and rows["asm_unrelated"][1] == "not Candida auris"
    assert decisions["two_files"] == "WARN" and rows["two_files"][6].startswith("WARN")

    sheet = write_sheet("sheet.tsv", samples)
    assert batch.main([sheet, "-O", "out", *options, "--log_file_path", "batch.log"]) == 0
    for name, _ in samples:
        assert Path(f"out/report.{name}.tsv").read_bytes() == singles[name], name
    header = singles[samples[0][0]].split(b"\n")[0] + b"\n"
    want_report = header + b"".join(singles[name][len(header):] for name, _ in samples)
    assert Path("out/report.tsv").read_bytes() == want_report
    assert Path("out/failed.tsv").read_text() == "Sample\tError\tMessage\n"

    args = batch.build_batch_parser().parse_args([sheet, "-O", "out3", *options])
    summary = batch.run_batch(batch.read_sheet(sheet), args, group_size=3)
    assert [(r.name, r.ok) for r in summary.samples] == [(name, True) for name, _ in samples]
    assert summary.seconds_sketch > 0 and summary.seconds_dist > 0 and summary.seconds_classify > 0
    for name, _ in samples:
        assert Path(f"out3/report.{name}.tsv").read_bytes() == singles[name], name
    assert Path("out3/report.tsv").read_bytes() == want_report


# ---- 5. failures stay with their sample -----------------------------------------------------------------------------------
def test_failures_stay_with_their_sample(refcwd):
    fastq = gzip.decompress(Path(READS[0]).read_bytes())
    lines = fastq.split(b"\n")
    record = (len(lines) // 4 // 2) * 4                      # a record in the middle of the file
    assert lines[record].startswith(b"@") and len(lines[record + 3]) == len(lines[record + 1]) > 10
    lines[record + 3] = lines[record + 3][:-5]
    Path("damaged.fq").write_bytes(b"\n".join(lines))
    samples = [
        ("good_reads", READS),
        ("empty", ["tests/data/test_empty_1.fq.gz", "tests/data/test_empty_2.fq.gz"]),
        ("missing", ["tests/data/nope_1.fq.gz", "tests/data/nope_2.fq.gz"]),
        ("sketch_as_input", [REF]),
        ("mixed", [READS[0], ASSEMBLY]),
        ("damaged", ["damaged.fq"]),
        ("good_assembly", [ASSEMBLY]),
    ]
    singles = {name: single_run(name, files, FIXTURE_OPTIONS) for name, files in samples}
    good, bad = ["good_reads", "good_assembly"], [name for name, _ in samples[1:-1]]
    assert singles["good_reads"] == (REFDATA / "reference_report_fastq.tsv").read_bytes().replace(b"isolate", b"good_reads")
    assert isinstance(singles["good_assembly"], bytes)
    for name in bad:
        assert isinstance(singles[name], Exception), name
        print(name, type(singles[name]).__name__, singles[name])

    sheet = write_sheet("sheet.tsv", samples)
    assert batch.main([sheet, "-O", "out", *FIXTURE_OPTIONS, "--log_file_path", "batch.log"]) == 1
    for name in good:
        assert Path(f"out/report.{name}.tsv").read_bytes() == singles[name], name
    for name in bad:
        assert not Path(f"out/report.{name}.tsv").exists(), name
    failed = Path("out/failed.tsv").read_text().split("\n")
    assert failed[0] == "Sample\tError\tMessage" and failed[-1] == "" and len(failed) == 2 + len(bad)
    for line, name in zip(failed[1:-1], bad):
        sample, error, message = line.split("\t")
        assert (sample, error) == (name, type(singles[name]).__name__), line
        assert message == " ".join(str(singles[name]).split("\n")).replace("\t", " "), line
    assert data_lines("out/report.tsv") == [singles[name].split(b"\n")[1] for name in good]
    log = Path("batch.log").read_text()
    for name in bad:
        assert f"[{name}] sample failed: {type(singles[name]).__name__}" in log, name
    # the same with every sample a group of its own, and with the damaged file last in a group of two
    args = batch.build_batch_parser().parse_args([sheet, "-O", "out1", *FIXTURE_OPTIONS])
    summary = batch.run_batch(batch.read_sheet(sheet), args, group_size=1)
    assert [(r.name, r.ok, r.error) for r in summary.samples] == [
        (name, name in good, None if name in good else type(singles[name]).__name__) for name, _ in samples]
    assert Path("out1/failed.tsv").read_text() == Path("out/failed.tsv").read_text()
    assert Path("out1/report.tsv").read_bytes() == Path("out/report.tsv").read_bytes()
    # a further single-sample run in the same process works
    assert single_run("again", READS, FIXTURE_OPTIONS, "again") == singles["good_reads"].replace(b"good_reads", b"again")


# ---- 6. stop on a device error ---------------------------------------------------------------------------------------------
def test_a_device_error_ends_the_batch(refcwd, monkeypatch):
    """Control flow only: engine.sketch_files is replaced by a Python function that raises EngineError(MHX_E_HIP) for the
    third sample; the device itself is never disturbed."""
    samples = [(f"s{i}", [ASSEMBLY] if i % 2 else READS) for i in range(1, 6)]
    sheet = write_sheet("sheet.tsv", samples)
    singles = {name: single_run(name, files, FIXTURE_OPTIONS) for name, files in samples[:2]}
    real_sketch, real_dist = engine.sketch_files, engine.dist_files_multi
    calls = {"sketch": 0, "dist": 0}

    def sketch(*a, **kw):
        calls["sketch"] += 1
        if calls["sketch"] == 3:
            raise engine.EngineError(engine.MHX_E_HIP, "H2D copy failed (made up by the test)")
        return real_sketch(*a, **kw)

    def dist(*a, **kw):
        calls["dist"] += 1
        return real_dist(*a, **kw)

    monkeypatch.setattr(engine, "sketch_files", sketch)
    monkeypatch.setattr(engine, "dist_files_multi", dist)
    # groups of two: the first group is finished when the third sample meets the error
    args = batch.build_batch_parser().parse_args([sheet, "-O", "out2", *FIXTURE_OPTIONS])
    with pytest.raises(engine.EngineError) as ei:
        batch.run_batch(batch.read_sheet(sheet), args, group_size=2)
    assert ei.value.code == engine.MHX_E_HIP
    assert calls == {"sketch": 3, "dist": 1}                    # samples four and five never reached the engine
    assert data_lines("out2/report.tsv") == [singles["s1"].split(b"\n")[1], singles["s2"].split(b"\n")[1]]
    assert Path("out2/report.s1.tsv").read_bytes() == singles["s1"] and Path("out2/report.s2.tsv").read_bytes() == singles["s2"]
    assert Path("out2/failed.tsv").read_text() == ("Sample\tError\tMessage\n"
                                                   "s3\tEngineError\tmhx error -6: H2D copy failed (made up by the test)\n")
    # one group: the first two are sketched but not finished, and no distance call is started after the error
    calls.update(sketch=0, dist=0)
    with pytest.raises(engine.EngineError):
        batch.main([sheet, "-O", "out", *FIXTURE_OPTIONS, "--log_file_path", "batch.log"])
    assert calls == {"sketch": 3, "dist": 0}
    assert data_lines("out/report.tsv") == [] and len(data_lines("out/failed.tsv")) == 1
    # an engine error that says nothing about the device's state stays with its sample
    calls.update(sketch=0, dist=0)
    fatal = {"code": engine.MHX_E_FORMAT}

    def sketch_refusing(*a, **kw):
        calls["sketch"] += 1
        if calls["sketch"] == 3:
            raise engine.EngineError(fatal["code"], "made up by the test")
        return real_sketch(*a, **kw)

    monkeypatch.setattr(engine, "sketch_files", sketch_refusing)
    assert batch.main([sheet, "-O", "out_fmt", *FIXTURE_OPTIONS, "--log_file_path", "fmt.log"]) == 1
    assert calls == {"sketch": 5, "dist": 1}
    assert len(data_lines("out_fmt/report.tsv")) == 4
    assert Path("out_fmt/failed.tsv").read_text() == "Sample\tError\tMessage\ns3\tEngineError\tmhx error -5: made up by the test\n"
    # and with the real engine back, the same sheet runs through
    monkeypatch.setattr(engine, "sketch_files", real_sketch)
    monkeypatch.setattr(engine, "dist_files_multi", real_dist)
    assert batch.main([sheet, "-O", "out_ok", *FIXTURE_OPTIONS, "--log_file_path", "ok.log"]) == 0
    assert len(data_lines("out_ok/report.tsv")) == 5

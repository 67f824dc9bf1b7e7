#!/usr/bin/env python3
"""A run of samples in ONE process: `python -m auriclass_amd.batch SHEET -O OUTDIR [options of auriclass]`.

The single-sample command (auriclass_amd.main) pays for an interpreter, pandas and the HIP runtime once per sample, and
reads, checks and uploads the same reference sketch every time.  Here the device is opened once, every sample is sketched
by the same call as there, and the distances of up to 1024 samples are computed by ONE `engine.dist_files_multi` call --
the many-queries x few-references shape the distance kernels were tuned for.  Each sample still gets the report that
the single-sample command writes for it, byte for byte: the same FastqAuriclass / FastaAuriclass object is built, its own
rows of the distance text go through the same `pd.read_csv` call, and `_classify_and_report()` is unchanged.

Sample sheet: UTF-8, one sample per line, `name<TAB>file[<TAB>file ...]`; blank lines and lines starting with `#` are
skipped.  All files of a line are one sample.  Outputs in OUTDIR: `report.<name>.tsv` per successful sample, `report.tsv`
(header once, then every successful sample's line in sheet order), `failed.tsv` (`Sample<TAB>Error<TAB>Message`).

A sample that fails stays a failed sample: its exception is logged and recorded and the batch goes on.  An EngineError
that says the device or the library is not in a known state (MHX_E_HIP, MHX_E_NO_DEVICE, MHX_E_INTERNAL) ends the batch
at once: nothing further is started on the device, the reports of what was finished are written, the error is re-raised.
"""
from __future__ import annotations

import argparse
import logging
import sys
import tempfile
import time
from contextlib import contextmanager
from dataclasses import dataclass, field
from datetime import datetime
from pathlib import Path
from typing import Iterator, List, Optional, Sequence

from auriclass_amd import engine
from auriclass_amd.args import add_classification_options
from auriclass_amd.classes import _REPORT_COLUMNS, FastaAuriclass, FastqAuriclass
from auriclass_amd.general import (
    add_tag,
    check_dependencies,
    confirm_input_type,
    guess_input_type,
    validate_argument_logic,
    validate_input_files,
)
from auriclass_amd.main import _default_data_file
from auriclass_amd.version import __description__

GROUP_SIZE = 1024  # samples per distance call: bounds the temporary .msh files and the staging at ~0.4 GB at s = 50 000
FATAL_ENGINE_CODES = (engine.MHX_E_HIP, engine.MHX_E_NO_DEVICE, engine.MHX_E_INTERNAL)
FAILED_HEADER = "Sample\tError\tMessage\n"


# --------------------------------------------------------------------------- sample sheet
@dataclass
class Sample:
    name: str
    files: List[str]
    line: int  # 1-based line of the sheet


def parse_sheet(data: bytes) -> List[Sample]:
    """The samples of a sheet, in its order.  ValueError naming the line number for a line that breaks a rule."""
    samples: List[Sample] = []
    seen = {}
    for number, raw in enumerate(data.split(b"\n"), start=1):
        try:
            line = raw.decode("utf-8")
        except UnicodeDecodeError as exc:
            raise ValueError(f"sample sheet line {number}: not valid UTF-8 ({exc.reason})") from None
        if line.endswith("\r"):
            line = line[:-1]
        if line.strip() == "" or line.startswith("#"):
            continue
        name, *files = line.split("\t")
        if name == "":
            raise ValueError(f"sample sheet line {number}: empty sample name")
        if "/" in name or "\0" in name or name in (".", ".."):
            raise ValueError(f"sample sheet line {number}: sample name {name!r} cannot be part of a file name")
        if name in seen:
            raise ValueError(f"sample sheet line {number}: sample name {name!r} already used on line {seen[name]}")
        if not files:
            raise ValueError(f"sample sheet line {number}: sample {name!r} has no input file")
        if any(f == "" for f in files):
            raise ValueError(f"sample sheet line {number}: sample {name!r} has an empty file field")
        seen[name] = number
        samples.append(Sample(name, files, number))
    return samples


def read_sheet(path) -> List[Sample]:
    return parse_sheet(Path(path).read_bytes())


# --------------------------------------------------------------------------- command line
def build_batch_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m auriclass_amd.batch", description=__description__ + " (a run of samples in one process)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument_group("REQUIRED").add_argument(
        "sample_sheet", type=Path, help="Tab-separated sample sheet: name<TAB>file[<TAB>file ...], one sample per line")
    g = p.add_argument_group("Main arguments")
    g.add_argument("-O", "--output_dir", default=Path("."), type=Path,
                   help="Directory of report.<name>.tsv, report.tsv and failed.tsv (created if missing)")
    add_classification_options(g, p)
    return p


# --------------------------------------------------------------------------- results
@dataclass
class SampleResult:
    name: str
    ok: bool = False
    report_path: Optional[Path] = None
    error: Optional[str] = None    # class name of the exception
    message: Optional[str] = None  # its text


@dataclass
class BatchSummary:
    samples: List[SampleResult] = field(default_factory=list)  # finished samples (ok or failed), in sheet order
    seconds_sketch: float = 0.0
    seconds_dist: float = 0.0
    seconds_classify: float = 0.0

    @property
    def n_ok(self) -> int:
        return sum(1 for r in self.samples if r.ok)

    @property
    def n_failed(self) -> int:
        return sum(1 for r in self.samples if not r.ok)


def _one_line(text: str) -> str:
    return text.replace("\t", " ").replace("\r", " ").replace("\n", " ")


def write_batch_reports(output_dir, results: Sequence[SampleResult]) -> None:
    """`report.tsv` and `failed.tsv` of a batch from its per-sample outcomes (in sheet order).  The data line of a sample
    is copied from its own report file as bytes, not written again."""
    output_dir = Path(output_dir)
    header = ("\t".join(_REPORT_COLUMNS) + "\n").encode()
    with open(output_dir / "report.tsv", "wb") as out:
        out.write(header)
        for r in results:
            if not r.ok:
                continue
            data = Path(r.report_path).read_bytes()
            if not data.startswith(header):
                raise ValueError(f"{r.report_path} does not start with the report header")
            out.write(data[len(header):])
    with open(output_dir / "failed.tsv", "w", encoding="utf-8", newline="") as out:
        out.write(FAILED_HEADER)
        for r in results:
            if not r.ok:
                out.write(f"{r.name}\t{_one_line(r.error or '')}\t{_one_line(r.message or '')}\n")


# --------------------------------------------------------------------------- runner
@contextmanager
def _records_carry(names: List[Optional[str]]) -> Iterator[None]:
    """While active, every log record made while names[0] is set starts with "[<that name>] " -- whatever handlers are
    installed (main() of the single-sample command, run in the same process, replaces them)."""
    previous = logging.getLogRecordFactory()

    def factory(*args, **kwargs):
        record = previous(*args, **kwargs)
        if names[0] is not None:
            record.msg = "[%s] %s" % (names[0], record.getMessage())
            record.args = None
        return record

    logging.setLogRecordFactory(factory)
    try:
        yield
    finally:
        logging.setLogRecordFactory(previous)


def _is_fatal(exc: BaseException) -> bool:
    return isinstance(exc, engine.EngineError) and exc.code in FATAL_ENGINE_CODES


def run_batch(samples: Sequence[Sample], args: argparse.Namespace, group_size: int = GROUP_SIZE) -> BatchSummary:
    """Classifies `samples` with the options in `args` (a namespace of build_batch_parser()).  Returns the summary;
    raises what main() of the single-sample command raises for a bad reference sketch, clade config or option, and
    re-raises an EngineError of FATAL_ENGINE_CODES after writing the reports of what was finished."""
    if group_size < 1:
        raise ValueError("group_size must be at least 1")
    # once per batch: what the single-sample command does once per sample
    if args.reference_sketch_path == "":
        args.reference_sketch_path = _default_data_file("Candida_auris_clade_references.msh")
    if args.clade_config_path == "":
        args.clade_config_path = _default_data_file("clade_config.csv")
    validate_input_files([args.reference_sketch_path])
    validate_input_files([args.clade_config_path])
    args = validate_argument_logic(args)
    check_dependencies()
    output_dir = Path(args.output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)

    summary = BatchSummary()
    current: List[Optional[str]] = [None]

    def failed(sample: Sample, exc: BaseException) -> SampleResult:
        logging.error(f"sample failed: {type(exc).__name__}: {exc}")
        return SampleResult(sample.name, False, None, type(exc).__name__, str(exc))

    def sketch(sample: Sample, msh: Path):
        validate_input_files(sample.files)
        if args.fastq or args.fasta:
            input_type = "fastq" if args.fastq else "fasta"
            confirm_input_type(sample.files, input_type)
        else:
            input_type = guess_input_type(sample.files)
        obj = (FastqAuriclass if input_type == "fastq" else FastaAuriclass)(
            name=sample.name,
            output_report_path=output_dir / f"report.{sample.name}.tsv",
            read_paths=sample.files,
            reference_sketch_path=args.reference_sketch_path,
            kmer_size=int(args.kmer_size),
            sketch_size=int(args.sketch_size),
            minimal_kmer_coverage=int(args.minimal_kmer_coverage),
            clade_config_path=args.clade_config_path,
            genome_size_range=[int(size) for size in args.expected_genome_size],
            non_candida_threshold=float(args.non_candida_threshold),
            high_dist_threshold=float(args.high_dist_threshold),
            no_qc=args.no_qc,
        )
        obj.query_sketch_path = msh
        if input_type == "fastq":
            obj.sketch_fastq_query()
        else:
            obj.sketch_fasta_query()
        return obj

    def run_group(first: int, group: Sequence[Sample], tmpdir: Path) -> None:
        results: List[SampleResult] = [SampleResult(s.name) for s in group]
        sketched = []  # (position in the group, object, number of sketches in its .msh)
        t0 = time.perf_counter()
        try:
            for pos, sample in enumerate(group):
                current[0] = sample.name
                try:
                    obj = sketch(sample, tmpdir / f"{first + pos}.msh")
                    sketched.append((pos, obj, 1 if isinstance(obj, FastqAuriclass) else len(sample.files)))
                except Exception as exc:
                    results[pos] = failed(sample, exc)
                    if _is_fatal(exc):
                        summary.samples.extend(r for r in results[:pos + 1] if r.error)  # the sketched ones stay unfinished
                        raise
                finally:
                    current[0] = None
        finally:
            summary.seconds_sketch += time.perf_counter() - t0
        pieces: List[str] = []
        if sketched:
            t0 = time.perf_counter()
            logging.info(add_tag("mash dist", f"mash dist {args.reference_sketch_path} <{len(sketched)} query sketches of samples "
                                              f"{group[sketched[0][0]].name} .. {group[sketched[-1][0]].name}>"))
            try:
                text = engine.dist_files_multi(args.reference_sketch_path, [obj.query_sketch_path for _, obj, _ in sketched])
            except Exception as exc:  # the call stands for one `mash dist` per sample: each of them has failed this way
                for pos, _, _ in sketched:
                    current[0] = group[pos].name
                    results[pos] = failed(group[pos], exc)
                    current[0] = None
                summary.samples.extend(results)
                if _is_fatal(exc):
                    raise
                return
            finally:
                summary.seconds_dist += time.perf_counter() - t0
            lines = text.split("\n")
            if lines.pop() != "":
                raise RuntimeError("distance text does not end with a newline")
            n_sketches = sum(n for _, _, n in sketched)
            n_refs, rest = divmod(len(lines), n_sketches)
            if rest:
                raise RuntimeError(f"{len(lines)} distance rows for {n_sketches} query sketches")
            at = 0
            for _, _, n in sketched:
                rows = lines[at:at + n * n_refs]
                at += n * n_refs
                pieces.append("".join(row + "\n" for row in rows))
        t0 = time.perf_counter()
        try:
            for (pos, obj, _), piece in zip(sketched, pieces):
                current[0] = group[pos].name
                try:
                    obj.set_mash_output(piece)
                    if isinstance(obj, FastaAuriclass):
                        obj.parse_genome_size()
                    obj._classify_and_report()
                    results[pos] = SampleResult(obj.name, True, Path(obj.output_report_path))
                except Exception as exc:
                    results[pos] = failed(group[pos], exc)
                    if _is_fatal(exc):
                        summary.samples.extend(r for r in results if r.ok or r.error)
                        raise
                finally:
                    current[0] = None
        finally:
            summary.seconds_classify += time.perf_counter() - t0
        summary.samples.extend(results)

    with _records_carry(current):
        try:
            for first in range(0, len(samples), group_size):
                with tempfile.TemporaryDirectory() as tmpdir:
                    run_group(first, samples[first:first + group_size], Path(tmpdir))
        finally:
            write_batch_reports(output_dir, summary.samples)
    return summary


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_batch_parser().parse_args(argv)
    samples = read_sheet(args.sample_sheet)
    output_dir = Path(args.output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    log_path = args.log_file_path or output_dir / f"report.{datetime.now().strftime('%Y-%m-%d_%H-%M-%S')}.log"
    logging.basicConfig(filename=log_path, filemode="w", format="%(asctime)s %(levelname)s %(message)s",
                        datefmt="%H:%M:%S", force=True)
    logging.getLogger().addHandler(logging.StreamHandler())
    if args.verbose:
        logging.getLogger().setLevel(logging.INFO)
    if args.debug:
        logging.getLogger().setLevel(logging.DEBUG)

    summary = run_batch(samples, args)
    logging.info(f"batch: {summary.n_ok} of {len(samples)} samples classified, {summary.n_failed} failed; "
                 f"sketching {summary.seconds_sketch:.3f} s, distance calls {summary.seconds_dist:.3f} s, "
                 f"classification and reports {summary.seconds_classify:.3f} s")
    return 0 if summary.n_ok == len(samples) else 1


if __name__ == "__main__":
    sys.exit(main())

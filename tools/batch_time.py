#!/usr/bin/env python3
"""Throughput of a run of samples: one `python -m auriclass_amd.main` process per sample (one after another, and 8 at a
time) against ONE `python -m auriclass_amd.batch` process, on inputs of the size a user would run.

    python tools/batch_time.py --output profiles/batch_throughput.txt

Inputs come from seeds (auriclass_amd.synth): a 12 Mb genome, 24 references (6 clades of 4 mutated copies), N assemblies
and M paired .fq.gz samples at 30x of further mutated copies; AuriClass's defaults (k = 27, s = 50 000, m = 3).  The
two ways are timed interleaved, `--repeats` times each, per kind of input; the reports they write are compared as bytes.
Every step that uses the GPU is a child process under a time limit of its own, and the command ends at the first step
that fails.  Never more than 8 children have the device open at a time."""
from __future__ import annotations

import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GENOME_BASES = 12_000_000
READ_LEN = 150
CLADES = ["I", "II", "III", "IV", "V", "outgroup"]


class Out:
    def __init__(self, path):
        self.file = open(path, "w") if path else None

    def __call__(self, text=""):
        print(text, flush=True)
        if self.file:
            self.file.write(text + "\n")
            self.file.flush()


def child_env(extra=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(ROOT) + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.update(extra or {})
    return env


def step(what, argv, limit, cwd, env=None):
    """One child process under its time limit; the whole command ends here when it fails."""
    t0 = time.perf_counter()
    try:
        done = subprocess.run(argv, cwd=cwd, env=child_env(env), timeout=limit, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        sys.exit(f"batch_time: step '{what}' ran longer than {limit} s; stopping")
    if done.returncode != 0:
        sys.exit(f"batch_time: step '{what}' failed with status {done.returncode}; stopping\n{done.stderr[-2000:]}")
    return time.perf_counter() - t0, done


# --------------------------------------------------------------------------- steps run as children
def generate(work: Path, n_assemblies: int, n_read_pairs: int, coverage: int) -> None:
    """Inputs, reference sketch and clade config under `work` (uses the GPU for the reads and the reference sketch)."""
    import torch

    from auriclass_amd import engine, synth

    device = "cuda" if torch.cuda.is_available() else "cpu"
    base = synth.make_genome(GENOME_BASES, seed=1)
    refs, rows = [], ["filename,clade"]
    clade_genomes = []
    for c, clade in enumerate(CLADES):
        root = base if c == 0 else synth.mutate(base, 0.05 if clade == "outgroup" else 0.004 * c, seed=10 + c)
        clade_genomes.append(root)
        for j in range(4):
            g = root if j == 0 else synth.mutate(root, 0.0002 * j, seed=100 + 10 * c + j)
            path = f"ref_{clade}_{j}.fasta"
            (work / path).write_bytes(synth.genome_fasta(g, name=f"ref_{clade}_{j}"))
            refs.append(path)
            rows.append(f"{path},{clade}")
    (work / "clades.csv").write_text("\n".join(rows) + "\n")
    os.chdir(work)
    engine.sketch_files(refs, 27, 50_000, "refs.msh")
    for i in range(n_assemblies):
        g = synth.mutate(clade_genomes[i % 5], 0.0005, seed=1000 + i)
        Path(f"asm_{i:03d}.fasta").write_bytes(synth.genome_fasta(g, name=f"asm_{i:03d}"))
    n_reads = coverage * GENOME_BASES // READ_LEN
    n_reads -= n_reads % 2
    half = (n_reads // 2) * synth.record_bytes(READ_LEN)
    packers = []
    for i in range(n_read_pairs):
        g = synth.mutate(clade_genomes[i % 5], 0.0005, seed=2000 + i)
        data = synth.make_fastq(g, n_reads, READ_LEN, seed=3000 + i, device=device).cpu().numpy()
        for mate, part in ((1, data[:half]), (2, data[half:])):
            path = f"reads_{i:03d}_{mate}.fq"
            part.tofile(path)
            packers.append(subprocess.Popen(["gzip", "-1", "-f", path]))  # (host only; at most 2 x n_read_pairs of them)
        del data
    if any(p.wait() != 0 for p in packers):
        raise SystemExit("gzip failed")


def dist_laps(work: Path, n_assemblies: int) -> None:
    """The assemblies' sketch files, repeated up to 1024 query files, through one dist_files_multi call (its phase times
    go to stderr when MHX_DIST_TIMING is set); the second call is the one to read, the first pins and allocates."""
    from auriclass_amd import engine

    os.chdir(work)
    files = []
    for i in range(n_assemblies):
        engine.sketch_files([f"asm_{i:03d}.fasta"], 27, 50_000, f"lap_{i:03d}.msh")
        files.append(f"lap_{i:03d}.msh")
    queries = (files * (1024 // len(files) + 1))[:1024]
    for call in (1, 2):
        print(f"-- call {call}: 1024 query files x 24 references", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        text = engine.dist_files_multi("refs.msh", queries)
        dt = time.perf_counter() - t0
        print(f"-- call {call}: {dt * 1e3:.1f} ms in all, {len(text.splitlines())} rows, {len(text)} bytes of text, "
              f"fallback blocks {engine.load().mhx_last_dist_fallback_blocks()}", file=sys.stderr, flush=True)


# --------------------------------------------------------------------------- the measurement
def single_argv(name, files, report, log):
    return [sys.executable, "-m", "auriclass_amd.main", *files, "-n", name, "-o", str(report), "--log_file_path", str(log),
            "-r", "refs.msh", "-c", "clades.csv"]


def run_sequential(samples, out_dir: Path, work: Path, limit: int) -> float:
    out_dir.mkdir(parents=True, exist_ok=True)
    total = 0.0
    for name, files in samples:
        dt, _ = step(f"single run of {name}", single_argv(name, files, out_dir / f"{name}.tsv", out_dir / f"{name}.log"), limit, work)
        total += dt
    return total


def run_concurrent(samples, out_dir: Path, work: Path, limit: int, width: int = 8) -> float:
    """`width` single-sample processes at a time (never more with the device open); ends at the first failure."""
    out_dir.mkdir(parents=True, exist_ok=True)
    todo = list(samples)
    live = []  # (name, process, deadline)
    failure = None
    t0 = time.perf_counter()
    while (todo and failure is None) or live:
        while todo and failure is None and len(live) < width:
            name, files = todo.pop(0)
            p = subprocess.Popen(single_argv(name, files, out_dir / f"{name}.tsv", out_dir / f"{name}.log"), cwd=work, env=child_env(),
                                 stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            live.append((name, p, time.perf_counter() + limit))
        time.sleep(0.005)
        for item in list(live):
            name, p, deadline = item
            rc = p.poll()
            if rc is None and time.perf_counter() > deadline:
                p.kill()
                p.wait()
                rc = -9
            if rc is None:
                continue
            live.remove(item)
            if rc != 0 and failure is None:
                failure = f"single run of {name} (8 at a time) ended with status {rc}"
    if failure:
        sys.exit(f"batch_time: {failure}; stopping")
    return time.perf_counter() - t0


def run_batch(samples, out_dir: Path, work: Path, limit: int):
    sheet = work / f"{out_dir.name}.tsv"
    sheet.write_text("".join("\t".join([name, *files]) + "\n" for name, files in samples))
    dt, done = step(f"batch of {len(samples)} samples", [sys.executable, "-m", "auriclass_amd.batch", str(sheet), "-O", str(out_dir),
                                                          "--log_file_path", str(out_dir) + ".log", "--verbose", "-r", "refs.msh", "-c", "clades.csv"],
                    limit, work)
    split = [ln for ln in Path(str(out_dir) + ".log").read_text().splitlines() if " batch: " in ln]
    return dt, (split[-1].split(" batch: ", 1)[1] if split else "?")


def spread(values):
    return f"median {statistics.median(values):.2f}  min {min(values):.2f}  max {max(values):.2f}"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--assemblies", type=int, default=32)
    ap.add_argument("--read-pairs", type=int, default=8)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--output", help="also write the report to this file")
    ap.add_argument("--workdir", help="where the inputs go (default: a temporary directory, removed at the end)")
    ap.add_argument("--step", choices=["generate", "dist-laps"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        work = Path(a.workdir)
        generate(work, a.assemblies, a.read_pairs, a.coverage) if a.step == "generate" else dist_laps(work, a.assemblies)
        return

    out = Out(a.output)
    work = Path(a.workdir or tempfile.mkdtemp(prefix="batch_time_")).resolve()
    work.mkdir(parents=True, exist_ok=True)
    try:
        me = [sys.executable, str(Path(__file__).resolve()), "--workdir", str(work), "--assemblies", str(a.assemblies),
              "--read-pairs", str(a.read_pairs), "--coverage", str(a.coverage)]
        dt, _ = step("generate inputs", me + ["--step", "generate"], 900, work)
        out(f"# batch throughput: {a.assemblies} assemblies and {a.read_pairs} paired .fq.gz samples ({a.coverage}x) of a "
            f"{GENOME_BASES / 1e6:.0f} Mb genome, 24 references, k = 27, s = 50 000, m = 3; {a.repeats} repeats, interleaved")
        out(f"# inputs generated in {dt:.1f} s")
        kinds = {
            "assemblies": [(f"asm_{i:03d}", [f"asm_{i:03d}.fasta"]) for i in range(a.assemblies)],
            "read pairs": [(f"reads_{i:03d}", [f"reads_{i:03d}_1.fq.gz", f"reads_{i:03d}_2.fq.gz"]) for i in range(a.read_pairs)],
        }
        times = {kind: {"seq": [], "par8": [], "batch": []} for kind in kinds}
        splits = {kind: [] for kind in kinds}
        for rep in range(a.repeats):
            for kind, samples in kinds.items():
                tag = f"{kind.split()[0]}_{rep}"
                times[kind]["seq"].append(run_sequential(samples, work / f"seq_{tag}", work, 300))
                times[kind]["par8"].append(run_concurrent(samples, work / f"par_{tag}", work, 300))
                dt, split = run_batch(samples, work / f"batch_{tag}", work, 900)
                times[kind]["batch"].append(dt)
                splits[kind].append(split)
                print(f"[batch_time] repeat {rep}, {kind}: " + ", ".join(f"{way} {times[kind][way][-1]:.2f} s" for way in ("seq", "par8", "batch")),
                      file=sys.stderr, flush=True)
                for name, _ in samples:  # the three ways wrote the same report bytes
                    want = (work / f"seq_{tag}" / f"{name}.tsv").read_bytes()
                    if (work / f"par_{tag}" / f"{name}.tsv").read_bytes() != want or (work / f"batch_{tag}" / f"report.{name}.tsv").read_bytes() != want:
                        sys.exit(f"batch_time: the reports of {name} differ between the single runs and the batch (repeat {rep}); stopping")
                if len((work / f"batch_{tag}" / "report.tsv").read_bytes().splitlines()) != len(samples) + 1:
                    sys.exit("batch_time: report.tsv of the batch lacks samples; stopping")
        out("# reports: identical bytes from the single runs (sequential, 8 at a time) and the batch, every sample, every repeat")
        out()
        for kind, samples in kinds.items():
            n = len(samples)
            out(f"## {n} {kind}")
            for way, label in (("seq", "(a)  one process per sample, sequential"), ("par8", "(a8) one process per sample, 8 at a time"),
                               ("batch", "(b)  one batch process")):
                rates = [n / t for t in times[kind][way]]
                out(f"{label:44s} samples/s: {spread(rates)}    seconds: " + " ".join(f"{t:.2f}" for t in times[kind][way]))
            out(f"(b) over (a), medians: {statistics.median(times[kind]['seq']) / statistics.median(times[kind]['batch']):.1f}x; "
                f"(b) over (a8): {statistics.median(times[kind]['par8']) / statistics.median(times[kind]['batch']):.1f}x")
            for rep, split in enumerate(splits[kind]):
                out(f"batch's own split, repeat {rep}: {split}")
            out()
        _, done = step("1024-query distance call", me + ["--step", "dist-laps"], 600, work, env={"MHX_DIST_TIMING": "1"})
        out("## one dist_files_multi call: 1024 query files (the assemblies' sketches, repeated) x 24 references, MHX_DIST_TIMING laps")
        for line in done.stderr.splitlines():
            if line.startswith("[mhx dist_files]") or line.startswith("-- call"):
                out(line)
    finally:
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()

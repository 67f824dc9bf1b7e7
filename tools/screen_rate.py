"""Rate of the containment screen (`mash screen`, engine.Screener) on the C3 input -- 10 M x 150 bp reads resident in HBM --
against 24 clade-like references, next to the sketch step on the same bytes in the same session:

    ms per reset + push_device + finish   screen without the set-size sketch | screen with it | Sketcher(k, s, m = 1)

at (k = 21, s = 1000) and (k = 27, s = 50 000), the variants interleaved round by round; one more row per setting for the
small-reference regime (a 5 kb genome among the references puts T_screen high: every window, or every fifth, probes the
table) -- the slow case, measured on a tenth of the reads.  --file-level adds one paired .fq.gz sample (12 Mb genome, 30x)
through mhx_screen_files and mhx_sketch_files, interleaved.

    python tools/screen_rate.py [--reads N] [--rounds R] [--file-level]
"""
import argparse
import gzip
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from auriclass_amd import engine, synth  # noqa: E402


def gpu_sketch(genome: np.ndarray, k: int, s: int) -> np.ndarray:
    sk = engine.Sketcher(k, s, 1, expected_bytes=genome.size + 1)
    sk.push_host(genome.tobytes() + b"\n", engine.FMT_SEQ)
    h, _ = sk.finish()
    sk.close()
    return h


def pack(refs):
    stride = max(len(r) for r in refs)
    rows = np.zeros((len(refs), stride), dtype=np.uint64)
    for i, r in enumerate(refs):
        rows[i, :len(r)] = r
    return rows, np.array([len(r) for r in refs], dtype=np.uint32)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--file-level", action="store_true")
    args = ap.parse_args()
    engine.init(0)
    print(engine.device_name())
    g = synth.make_genome(12_000_000, 42)
    fq = synth.make_fastq(g, args.reads, 150, 43, device="cuda")
    torch.cuda.synchronize()
    nbytes = fq.numel()
    bases = args.reads * 150
    clade = [g] + [synth.mutate(g, 0.0005 * (1 + i % 6), 100 + i) for i in range(23)]
    small = synth.make_genome(5_000, 7)
    for k, s in ((21, 1000), (27, 50_000)):
        refs = [gpu_sketch(x, k, s) for x in clade]
        rows, lens = pack(refs)
        distinct = np.unique(np.concatenate(refs)).size
        print(f"\nk = {k}, s = {s}: 24 references, {int(lens.sum())} hashes, {distinct} distinct, T_screen / 2^64 = {int(max(r[-1] for r in refs)) / 2.0 ** 64:.3g}")
        bare = engine.Screener(k, rows, lens, s, with_set_size=False)
        full = engine.Screener(k, rows, lens, s, with_set_size=True)
        sk = engine.Sketcher(k, s, 1, expected_bytes=nbytes)

        def run(obj):
            obj.reset()
            obj.push_device(fq.data_ptr(), nbytes, engine.FMT_FASTQ4)
            return obj.finish()

        variants = (("screen, no set-size sketch", bare), ("screen with set-size sketch", full), ("sketch step (Sketcher, m = 1)", sk))
        times = {name: [] for name, _ in variants}
        for rd in range(args.rounds + 1):
            for name, obj in variants:
                t = timed(lambda: run(obj))
                if rd:
                    times[name].append(t)
        shared = run(bare)[0]
        print(f"    shared of the first / last reference: {int(shared[0])}/{int(lens[0])}  {int(shared[-1])}/{int(lens[-1])}")
        base = statistics.median(times[variants[2][0]])
        for name, _ in variants:
            ts = times[name]
            med = statistics.median(ts)
            print(f"    {name:32s} median {med:8.2f} ms  min {min(ts):8.2f}  max {max(ts):8.2f}  ({med / base:5.2f} x sketch step, {bases / med / 1e6:7.1f} Gbases/s)")
        spread = max((max(ts) - min(ts)) / statistics.median(ts) for ts in times.values())
        print(f"    noise floor of this block (largest (max - min) / median over {args.rounds} rounds): {100 * spread:.2f} %")
        bare.close(); full.close(); sk.close()
        # the slow case: a reference whose sketch is (nearly) the whole small genome -- T_screen near 2^64
        rows2, lens2 = pack(refs + [gpu_sketch(small, k, s)])
        slow = engine.Screener(k, rows2, lens2, s, with_set_size=False)
        part = (args.reads // 10) * synth.record_bytes(150)
        ts = []
        for rd in range(4):
            slow.reset()
            t = timed(lambda: (slow.push_device(fq.data_ptr(), part, engine.FMT_FASTQ4), slow.finish()))
            if rd:
                ts.append(t)
        print(f"    SLOW CASE, 25th reference = a 5 kb genome (T_screen / 2^64 = {int(rows2[-1, lens2[-1] - 1]) / 2.0 ** 64:.3g}), a tenth of the reads: "
              f"median {statistics.median(ts):8.2f} ms  ({(args.reads // 10) * 150 / statistics.median(ts) / 1e6:7.1f} Gbases/s)")
        slow.close()
    if not args.file_level:
        return
    # one paired .fq.gz sample (12 Mb genome, 30x) through both file-level calls, interleaved
    k, s = 27, 50_000
    n = 12_000_000 * 30 // 150
    rb = synth.record_bytes(150)
    host = fq[: n * rb].cpu().numpy()
    d = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    files = []
    for i in range(2):
        p = os.path.join(d, f"sample_{i + 1}.fq.gz")
        with gzip.open(p, "wb", compresslevel=1) as fh:
            fh.write(host[i * (n // 2) * rb:(i + 1) * (n // 2) * rb].tobytes())
        files.append(p)
    msh = os.path.join(d, "refs.msh")
    refs = [gpu_sketch(x, k, s) for x in clade]
    engine.msh_write(msh, k, s, [f"clade_{i}.fa" for i in range(24)], ["synthetic"] * 24, [12_000_000] * 24, refs)
    tt = {"mhx_screen_files": [], "mhx_sketch_files (reads, m = 1)": []}
    for rd in range(4):
        a = timed(lambda: engine.screen_files(msh, files))
        b = timed(lambda: engine.sketch_files(files, k, s, os.path.join(d, "o.msh"), reads=True, min_mult=1))
        if rd:
            tt["mhx_screen_files"].append(a)
            tt["mhx_sketch_files (reads, m = 1)"].append(b)
    print(f"\nfile level, paired .fq.gz sample ({n} reads, k = {k}, s = {s}, 24 references), route {engine.last_fastq_route()}:")
    for name, ts in tt.items():
        print(f"    {name:34s} median {statistics.median(ts):9.1f} ms  min {min(ts):9.1f}  max {max(ts):9.1f}")
    for p in files + [msh, os.path.join(d, "o.msh")]:
        os.remove(p)
    os.rmdir(d)


if __name__ == "__main__":
    main()

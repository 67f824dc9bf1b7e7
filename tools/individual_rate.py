"""What sketching every record of a multi-FASTA on its own costs (`mash sketch -i`, k = 21, s = 1000), on synthetic files
from auriclass_amd/synth.py:

    short      20 000 records of 2 000 bases   (plasmid genes, marker loci: every record below the cut of the segmented sketch)
    assembly   40 records of 10^5 .. 10^6 bases (every record above the cut: the existing sketcher, one record after another)

Three ways, interleaved round by round, host clock around calls that are complete when they return:

    (a) segments   mhx_sketch_segments on the resident dense stream, rows left on the device
    (b) loop       what there was before it: Sketcher.reset / push_device / finish per record on the same resident stream
    (c) file       the file-level call (read, parse on the device, sketch, write the .msh)

After a warm-up of each, every way is timed --rounds times (default 3); the best and all rounds are printed, the rows of (a)
are compared with the lists of (b).  The baseline is (b).

    python tools/individual_rate.py [--rounds R] [--out FILE] [--inputs short,assembly]
    python tools/individual_rate.py --once        (one warmed call of (a) on `short` and nothing else: for a kernel trace)
"""
import argparse
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
K, S = 21, 1000


def make_input(name):
    import numpy as np

    from auriclass_amd import synth

    if name == "short":
        lengths = np.full(20_000, 2_000, dtype=np.int64)
    else:
        lengths = np.random.default_rng(3).integers(100_000, 1_000_001, size=40)
    genome = synth.make_genome(int(lengths.sum()), seed=17)
    off = np.zeros(lengths.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    fasta = []
    for i in range(lengths.size):
        seq = genome[int(off[i]):int(off[i + 1])].tobytes()
        fasta.append(b">rec_%d synthetic\n" % i)
        fasta.append(b"\n".join(seq[j:j + 70] for j in range(0, len(seq), 70)) + b"\n")
    return genome, off, b"".join(fasta)


def measure(name, rounds, once, say):
    import numpy as np
    import torch

    from auriclass_amd import engine

    genome, off, fasta = make_input(name)
    n_seg = off.size - 1
    dev = "cuda:0"
    d_bytes = torch.zeros(genome.size + 64, dtype=torch.uint8, device=dev)
    d_bytes[:genome.size] = torch.from_numpy(genome).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    stride = S
    d_rows = torch.zeros((n_seg, stride), dtype=torch.int64, device=dev)
    d_len = torch.zeros(n_seg, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def way_a():
        t0 = time.perf_counter()
        engine.sketch_segments_device(d_bytes.data_ptr(), genome.size, d_off.data_ptr(), n_seg, K, S, d_rows.data_ptr(), d_len.data_ptr(), stride)
        return time.perf_counter() - t0

    if once:
        way_a()
        way_a()
        return
    sk = engine.Sketcher(K, S, 1)
    base = d_bytes.data_ptr()
    lists = [None] * n_seg

    def way_b(first=n_seg):
        t0 = time.perf_counter()
        for i in range(first):
            sk.reset()
            sk.push_device(base + int(off[i]), int(off[i + 1] - off[i]), engine.FMT_SEQ)
            lists[i], _ = sk.finish()
        return time.perf_counter() - t0

    with tempfile.TemporaryDirectory() as tmp:
        path, out = Path(tmp) / f"{name}.fa", Path(tmp) / f"{name}.msh"
        path.write_bytes(fasta)

        def way_c():
            t0 = time.perf_counter()
            engine.sketch_files([path], K, S, out, individual=True)
            return time.perf_counter() - t0

        way_a(), way_b(min(n_seg, 200)), way_c()   # warm-up: code objects, buffers, the page cache
        times = {"segments": [], "loop": [], "file": []}
        for _ in range(rounds):
            times["segments"].append(way_a())
            times["loop"].append(way_b())
            times["file"].append(way_c())
    rows, lens = d_rows.cpu().numpy().view(np.uint64), d_len.cpu().numpy().view(np.uint32)
    same = all(lens[i] == lists[i].size and np.array_equal(rows[i, :lens[i]], lists[i]) for i in range(n_seg))
    say(f"{name}: {n_seg} records, {genome.size} bases, k = {K}, s = {S}; rows of (a) equal the lists of (b): {same}")
    for what, label in (("segments", "(a) mhx_sketch_segments, resident stream"), ("loop", "(b) reset / push_device / finish per record"),
                        ("file", "(c) sketch_files(individual=True), file to .msh")):
        v = times[what]
        say(f"  {label:48s} best {min(v) * 1e3:10.2f} ms   rounds " + " ".join(f"{x * 1e3:.2f}" for x in v) +
            f"   {n_seg / min(v):12.0f} records/s  {genome.size / min(v) / 1e6:9.1f} Mbase/s")
    say(f"  (b) / (a) = {min(times['loop']) / min(times['segments']):.2f}   spread of (a) {100 * (max(times['segments']) / min(times['segments']) - 1):.1f} %, "
        f"of (b) {100 * (max(times['loop']) / min(times['loop']) - 1):.1f} %")
    sk.close()
    if not same:
        raise SystemExit("the two ways disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--inputs", default="short,assembly")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from auriclass_amd import engine

    engine.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if args.once:
        return measure("short", 1, True, say)
    say(f"tools/individual_rate.py on {engine.device_name()}: best of {args.rounds} interleaved rounds, host clock, every call complete on return")
    for name in args.inputs.split(","):
        measure(name, args.rounds, False, say)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The sketcher's calls on small inputs, once each, as the program of a kernel trace: what a change of the sketcher's host
side must leave as it was is the ORDER of the kernels each call launches (and their grids).  k = 21, s = 1000 unless said:

    the five cases of tests/test_gpu_push_plan.py (33 tiles for m = 1, 65 for m = 3, whole and in two parts; a sequence stream)
    s = 8192 (queued candidates, ordering on the device), a push from host memory, 3 kb and 4 kb reads (the repair pass:
    the 3 kb input is the one of tests/test_gpu_first_launch_split.py, whose reads leave tiles to the repair pass),
    a screener push, and two sketchers' export_begin / export_pack / merge_slabs with the slabs in host memory

One line per call with a digest of what it returned, so that two libraries (MHX_LIB) can be compared by their output too.
The merge takes the binned path; under MHX_MERGE_TABLE=1 (read once per process) the table path -- `--merge-only` runs
nothing but the merge, for the trace of that second process.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/push_trace.py [--merge-only]
    python3 tools/push_trace.py --dispatches DIR/.../*_kernel_trace.csv    kernel name and grid of such a trace in launch order
"""
import csv
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TILE = 16384
K, S = 21, 1000


def dispatches(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id") or 0)))
    grid = [c for c in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Grid_Size") if rows and c in rows[0]]
    return [" ".join([r["Kernel_Name"].split("(")[0]] + [r[c] for c in grid]) for r in rows]


def digest(*parts):
    h = hashlib.sha256()
    for part in parts:
        h.update(getattr(part, "tobytes", lambda: repr(part).encode())())
    return h.hexdigest()[:16]


def main():
    if sys.argv[1:2] == ["--dispatches"]:
        print("\n".join(dispatches(sys.argv[2])))
        return
    import torch

    from auriclass_amd import engine, synth

    engine.init(0)
    rb = synth.record_bytes(150)

    def fastq(tiles, seed=0):
        n_reads = (tiles * TILE - 100) // rb
        genome = synth.make_genome(max(400, n_reads * 150 // 12), seed=300 + tiles + seed)
        return synth.make_fastq(genome, n_reads, 150, seed=400 + tiles + seed, device="cpu").numpy()

    def on_device(data):
        dev = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
        dev[:data.size] = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        return dev

    def sketched(data, s, m, fmt, cuts=(), host=False):
        sk = engine.Sketcher(K, s, m, expected_bytes=0)
        if host:
            sk.push_host(data, fmt)
        else:
            dev = on_device(data)
            edges = [0, *cuts, data.size]
            for a, b in zip(edges[:-1], edges[1:]):
                sk.push_device(dev.data_ptr() + a, b - a, fmt)
        sk.sync()
        launches = sk.stats()["launches"]
        h, c = sk.finish()
        sk.close()
        return digest(h, c, launches) + f" ({launches} launches)"

    def merged():
        data = fastq(40, seed=7)
        n_reads = data.size // rb
        dev = on_device(data)
        sks, hdrs = [], []
        for lo, hi in ((0, n_reads // 2), (n_reads // 2, n_reads)):
            sk = engine.Sketcher(K, S, 1, expected_bytes=(hi - lo) * rb)
            sk.push_device(dev.data_ptr() + lo * rb, (hi - lo) * rb, engine.FMT_FASTQ4)
            sk.sync()
            sks.append(sk)
            hdrs.append(sk.export_begin())
        hdrs = np.stack(hdrs)
        cap = (int(hdrs[:, 0].max()) + 1023) // 1024 * 1024
        words = cap + cap // 2
        slabs = np.zeros(2 * words, np.int64)       # host memory, as gloo gathers them
        for r, sk in enumerate(sks):
            sk.export_pack(slabs.ctypes.data + r * words * 8, cap)
        h, c = sks[0].merge_slabs(slabs.ctypes.data, False, 2, cap, hdrs, 0)
        path = sks[0].merge_info()["path"]
        for sk in sks:
            sk.close()
        return digest(h, c, path) + f" (path {path})"

    def screened():
        refs = []
        for i in range(4):
            g = synth.make_genome(60_000, seed=900 + i)
            sk = engine.Sketcher(K, S, 1, expected_bytes=g.size + 1)
            sk.push_host(g.tobytes() + b"\n", engine.FMT_SEQ)
            refs.append(sk.finish()[0])
            sk.close()
        rows = np.zeros((len(refs), S), np.uint64)
        for i, r in enumerate(refs):
            rows[i, :len(r)] = r
        sc = engine.Screener(K, rows, np.array([len(r) for r in refs], np.uint32), S)
        reads = synth.make_fastq(synth.make_genome(60_000, seed=900), 2000, 150, seed=77, device="cpu").numpy()
        dev = on_device(reads)
        sc.push_device(dev.data_ptr(), reads.size, engine.FMT_FASTQ4)
        sc.sync()
        shared, median, size, _ = sc.finish()
        sc.close()
        return digest(shared, median, size)

    def record_start(tile):
        return (tile * TILE - 50) // rb * rb

    fq33, fq65 = fastq(33), fastq(65)
    long_reads = synth.make_fastq(synth.make_genome(30_000, seed=77), 55, 3000, seed=78, device="cpu").numpy()    # ~20 tiles
    long_reads_4k = synth.make_fastq(synth.make_genome(30_000, seed=79), 40, 4000, seed=80, device="cpu").numpy()  # ~20 tiles
    seq = np.frombuffer(synth.make_genome(33 * TILE - 101, seed=533).tobytes() + b"\n", np.uint8)
    calls = [("m=1 33 tiles whole", lambda: sketched(fq33, S, 1, engine.FMT_FASTQ4)),
             ("m=1 33 tiles as 20 + 13", lambda: sketched(fq33, S, 1, engine.FMT_FASTQ4, (record_start(20),))),
             ("m=3 65 tiles whole", lambda: sketched(fq65, S, 3, engine.FMT_FASTQ4)),
             ("m=3 65 tiles as 40 + 25", lambda: sketched(fq65, S, 3, engine.FMT_FASTQ4, (record_start(40),))),
             ("m=1 33 tiles sequence stream", lambda: sketched(seq, S, 1, engine.FMT_SEQ)),
             ("s=8192 40 tiles", lambda: sketched(fastq(40), 8192, 1, engine.FMT_FASTQ4)),
             ("push from host memory", lambda: sketched(fq33, S, 1, engine.FMT_FASTQ4, host=True)),
             ("3 kb reads (repair pass)", lambda: sketched(long_reads, S, 1, engine.FMT_FASTQ4)),
             ("4 kb reads", lambda: sketched(long_reads_4k, S, 1, engine.FMT_FASTQ4)),
             ("screener push", screened),
             ("merge of two sketchers, host slabs", merged)]
    if sys.argv[1:2] == ["--merge-only"]:
        calls = calls[-1:]
    for what, call in calls:
        print(f"{what}: {call()}", flush=True)


if __name__ == "__main__":
    main()

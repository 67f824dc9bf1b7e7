"""Device vs host gunzip of a synthetic .fq.gz, interleaved, best of N, in Gbases/s (bases = sequence bytes).  Both legs
start from the compressed bytes in host memory and end with the inflated bytes in device memory:
  host    mhx_gunzip_buffer_mt (the ingest's decoders, default thread budget) straight into pinned memory, one H2D copy
  device  mhx_gunzip_device into a preallocated device buffer

    python tools/device_inflate_rate.py [--reads 3000000] [--levels 1 6] [--reps 3] [--threads 32]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from auriclass_amd import engine, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3_000_000)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 6])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0, help="host decoder threads (0: the ingest's cap, 32)")
    a = ap.parse_args()
    engine.init(0)
    L = engine.load()
    genome = synth.make_genome(5_000_000, seed=1)
    fq = synth.make_fastq(genome, a.reads, 150, seed=2, device="cpu").numpy().tobytes()
    bases = a.reads * 150
    threads = a.threads or int(os.environ.get("MHX_INGEST_THREADS", "32"))
    pinned = torch.empty(len(fq), dtype=torch.uint8, pin_memory=True)
    out = torch.empty(len(fq), dtype=torch.uint8, device="cuda")
    need = ctypes.c_size_t(0)
    for level in a.levels:
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        gz = c.compress(fq) + c.flush()
        best = {"host": 1e9, "device": 1e9}
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = L.mhx_gunzip_buffer_mt(gz, len(gz), ctypes.c_void_p(pinned.data_ptr()), len(fq), ctypes.byref(need), threads)
            assert rc == 0 and need.value == len(fq)
            out.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            best["host"] = min(best["host"], time.perf_counter() - t)
            t = time.perf_counter()
            engine.gunzip_device(gz, out=out)
            best["device"] = min(best["device"], time.perf_counter() - t)
        st = engine.inflate_stats()
        print(json.dumps({"level": level, "fastq_bytes": len(fq), "gz_bytes": len(gz), "host_threads": threads,
                          "host_s": round(best["host"], 4), "device_s": round(best["device"], 4),
                          "host_gbases_s": round(bases / best["host"] / 1e9, 3),
                          "device_gbases_s": round(bases / best["device"] / 1e9, 3),
                          "device_over_host": round(best["host"] / best["device"], 3), "device_stats": st}), flush=True)


if __name__ == "__main__":
    main()

"""Diagnostic: where a tighten pass spends its time, from a -DMHX_TIGHTEN_STAMPS build (MHX_LIB=.../<variant>.so):
wall-clock ticks (10 ns) per phase of table_tighten_kernel, summed over the workgroups of every pass of one sketch step.

    MHX_LIB=auriclass_amd/lib_variants/tstamp.so python tools/tighten_stamps.py [--reads N] [--k K --s S --m M]
"""
import argparse
import ctypes
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from auriclass_amd import engine, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=4_000_000)
ap.add_argument("--k", type=int, default=21)
ap.add_argument("--s", type=int, default=1000)
ap.add_argument("--m", type=int, default=1)
args = ap.parse_args()
engine.init(0)
g = synth.make_genome(12_000_000, 42)
fq = synth.make_fastq(g, args.reads, 150, 43, device="cuda")
torch.cuda.synchronize()
sk = engine.Sketcher(args.k, args.s, args.m, expected_bytes=fq.numel())
L = engine.load()
L.mhx_sketcher_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
out = np.zeros(8, np.uint64)
for _ in range(3):   # the counters are cleared by reset(): the last step's passes, finish()'s included, remain
    sk.reset(); sk.push_device(fq.data_ptr(), fq.numel(), engine.FMT_FASTQ4); sk.finish()
    L.mhx_sketcher_debug_stamps(sk._h, out.ctypes.data)
names = ["LDS clear, T, phase chain", "key loop", "flushes", "release + ticket", "tail (last workgroup of a pass)"]
wgs = int(out[5])
print(f"workgroups over all passes of the step: {wgs}")
for n, v in zip(names[:4], out[:4]):
    print(f"{n:32s} {10.0 * float(v) / max(wgs, 1):9.1f} ns per workgroup")
print(f"{names[4]:32s} {10.0 * float(out[4]):9.1f} ns summed over the passes")

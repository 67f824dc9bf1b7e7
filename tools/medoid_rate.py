"""What the medoids of a partition of one sketch set cost (mhx_dist_medoids) against what a user did before they existed: the
whole triangle pulled to the host (mhx_dist_triangle) followed by per-cluster sums and an argmin in numpy -- and against one
clustering call on the same set (mhx_dist_cluster), the other pass over the same blocks.  The synthetic set of
tools/cluster_rate.py with its planted clades, k = 21, at 2048 x 1000 and 16 384 x 1000, under three partitions:

    (1) clusters     the labels of dist_cluster at the bound 0.011: clades of 8 and singletons, mostly small clusters
    (2) one cluster  label = 0 everywhere: every block runs, every pair adds to two sums
    (3) singletons   label[i] = i: no block runs at all

Per partition: engine.dist_medoids_device (rows and labels resident on the device, results left there), wall time around a call
that is complete when it returns and mhx_last_dist_kernel_ms of the call, with the blocks run of the blocks scheduled
(mhx_last_medoid_blocks); next to it
    (t) dist_triangle (host form) + for every cluster the sums of its members' rows and an argmin, in numpy (float64)
    (c) one dist_cluster_device call at the bound 0.011
The medoids of (t) are compared with the library's: they may differ where two sums tie or differ in the last bits of a float.
Last, partition (2) with the two forms of the sum kernel, each in processes of its own (MHX_LIB), interleaved: the wave's
combine (34 adds per wave at the most, the library as built) against two adds per pair (a -DMHX_MEDOID_PAIR_ATOMICS build,
auriclass_amd/lib_variants/medoid_pair_atomics.so by tools/build_variants.sh; skipped when it is not there).

    python tools/medoid_rate.py [--rounds R] [--shapes 2048x1000,16384x1000] [--bound 0.011] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21
VARIANT = ROOT / "auriclass_amd" / "lib_variants" / "medoid_pair_atomics.so"


def host_medoids(dist, label, chunk=512):
    """what a user writes: per cluster the sums of the members' distances to each other, and the first argmin"""
    import numpy as np

    n = label.size
    medoid = np.arange(n, dtype=np.uint32)
    order = np.argsort(label, kind="stable")
    bounds = np.flatnonzero(np.diff(label[order])) + 1
    for members in np.split(order, bounds):
        c = members.size
        if c < 2:
            continue
        m = members.astype(np.int64)
        total = np.zeros(c)
        for at in range(0, c, chunk):
            i, j = m[at:at + chunk, None], m[None, :]
            hi, lo = np.maximum(i, j), np.minimum(i, j)
            d = dist[np.where(hi > lo, hi * (hi - 1) // 2 + lo, 0)]
            d[hi == lo] = 0.0
            total[at:at + chunk] = d.sum(axis=1)
        medoid[members] = members[int(np.argmin(total))]
    return medoid


def time_one_cluster(shape, rounds):
    """child process: the kernel time of partition (2) with the library MHX_LIB names, as one JSON line"""
    import numpy as np
    import torch

    import cluster_rate
    from auriclass_amd import engine

    engine.init(0)
    L = engine.load()
    n, s = shape
    rows, lens, _ = cluster_rate.make_set(n, s, seed=n + s)
    d_rows = torch.from_numpy(rows.view(np.int64)).to("cuda:0")
    d_len = torch.from_numpy(lens.view(np.int32)).to("cuda:0")
    d_label = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_medoid = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_sum = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds + 1):
        engine.dist_medoids_device(d_rows.data_ptr(), d_len.data_ptr(), n, rows.shape[1], K, s, d_label.data_ptr(), d_medoid.data_ptr(), d_sum.data_ptr())
        ms.append(L.mhx_last_dist_kernel_ms())
    print(json.dumps({"kernel_ms": ms[1:], "medoid": int(d_medoid[0].item()), "sum0": int(d_sum[0].item()), "digest": int(d_sum.sum().item())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="2048x1000,16384x1000")
    ap.add_argument("--bound", type=float, default=0.011)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        time_one_cluster(tuple(int(x) for x in args.child.split("x")), args.rounds)
        return
    import numpy as np
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    import cluster_rate
    from auriclass_amd import engine

    engine.init(0)
    L = engine.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def row(label, v, unit="ms", scale=1e3):
        v = [x * scale for x in v]
        say(f"  {label:66s} median {statistics.median(v):10.3f} {unit}  best {min(v):10.3f}  worst {max(v):10.3f}   rounds " + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)

    say(f"tools/medoid_rate.py on {engine.device_name()}: k = {K}, bound {args.bound}, {args.rounds} rounds after a warm-up; wall = host clock around a call "
        "that is complete when it returns")
    for shape in args.shapes.split(","):
        n, s = (int(x) for x in shape.split("x"))
        rows, lens, _ = cluster_rate.make_set(n, s, seed=n + s)
        stride = rows.shape[1]
        dev = "cuda:0"
        d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_out = torch.zeros(n, dtype=torch.int32, device=dev)
        d_degree = torch.zeros(n, dtype=torch.int32, device=dev)
        d_medoid = torch.zeros(n, dtype=torch.int32, device=dev)
        d_sum = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # (c) one clustering call, which also gives partition (1)
        wall, kern = [], []
        for _ in range(args.rounds + 1):
            t0 = time.perf_counter()
            clusters, edges = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, args.bound, d_out.data_ptr(), d_degree.data_ptr())
            wall.append(time.perf_counter() - t0)
            kern.append(L.mhx_last_dist_kernel_ms())
        labels = {"(1) clusters": d_out.cpu().numpy().view(np.uint32).copy(), "(2) one cluster": np.zeros(n, np.uint32), "(3) singletons": np.arange(n, dtype=np.uint32)}
        sizes = np.bincount(labels["(1) clusters"], minlength=n)
        say(f"n = {n}, s = {s}: {n * (n - 1) // 2} pairs; partition (1): {clusters} clusters, {int((sizes > 1).sum())} of them with more than one member, the largest {int(sizes.max())}; "
            f"R = {L.mhx_last_dist_ranges()}")
        row("(c) dist_cluster_device, wall", wall[1:])
        row("    its kernel time (mhx_last_dist_kernel_ms)", kern[1:], scale=1.0)
        # (t) the triangle on the host, once for all partitions
        tri_wall = []
        for _ in range(2):
            t0 = time.perf_counter()
            _, _, dist = engine.dist_triangle(rows, lens, K, s)
            tri_wall.append(time.perf_counter() - t0)
        tri = row("(t) dist_triangle (host pointers, distances in host libm), wall", tri_wall[1:])
        for name, label in labels.items():
            d_label = torch.from_numpy(label.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            wall, kern = [], []
            for _ in range(args.rounds + 1):
                t0 = time.perf_counter()
                ran = engine.dist_medoids_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, d_label.data_ptr(), d_medoid.data_ptr(), d_sum.data_ptr())
                wall.append(time.perf_counter() - t0)
                kern.append(L.mhx_last_dist_kernel_ms())
            scheduled = L.mhx_last_medoid_blocks() & 0xFFFFFFFF
            medoid = d_medoid.cpu().numpy().view(np.uint32)
            say(f" partition {name}: blocks run {ran} of {scheduled} scheduled, fallback blocks {L.mhx_last_dist_fallback_blocks()}")
            a = row("dist_medoids_device, wall", wall[1:])
            row("    its kernel time (mhx_last_dist_kernel_ms)", kern[1:], scale=1.0)
            t0 = time.perf_counter()
            user = host_medoids(dist, label)
            sums = (time.perf_counter() - t0) * 1e3
            same = int((user == medoid).sum())
            say(f"  {'(t) + per-cluster sums and argmin in numpy: ' + format(sums, '.3f') + ' ms, with the triangle':66s} {tri + sums:17.3f} ms   = {(tri + sums) / a:.1f} x dist_medoids_device;"
                f" medoids equal for {same} of {n} lists")
        del dist
        # the two forms of the sum kernel at partition (2), a process each, interleaved
        if not VARIANT.exists():
            say("  per-pair atomics: no auriclass_amd/lib_variants/medoid_pair_atomics.so (tools/build_variants.sh medoid_pair_atomics \"-DMHX_MEDOID_PAIR_ATOMICS\"): skipped")
            continue
        got = {"combined": [], "per pair": []}
        digests = set()
        for _ in range(2):
            for form, lib in (("combined", engine.LIB_PATH), ("per pair", VARIANT)):
                r = subprocess.run([sys.executable, __file__, "--child", shape, "--rounds", str(args.rounds)], env=dict(os.environ, MHX_LIB=str(lib)), capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"the {form} form failed: {r.stderr[-2000:]}")
                res = json.loads(r.stdout.strip().splitlines()[-1])
                got[form] += res["kernel_ms"]
                digests.add((res["medoid"], res["sum0"], res["digest"]))
        say(f" partition (2), the two forms of the sum kernel, two processes each, interleaved; results equal: {len(digests) == 1}")
        a = row("combined (one add per query row and per reference), kernel time", got["combined"], scale=1.0)
        b = row("per-pair atomics (-DMHX_MEDOID_PAIR_ATOMICS), kernel time", got["per pair"], scale=1.0)
        say(f"  combined / per pair = {a / b:.3f}")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

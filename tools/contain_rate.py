"""What the containment from sketches costs (mhx_dist_contain), rows resident on the device.  Queries are synthetic
INDEPENDENT sketches (the generator of tools/triangle_rate.py: every list holds s values uniform below its own maximum),
every eighth of them a reference with 3 % of its hashes replaced; a reference set of up to 64 lists is clade-like (four bases, every member a base with 0.2 % .. 5 % of its hashes replaced,
as the references of one species are), a larger one independent like the queries.

    shapes     queries x references x s: 1 x 24 and 1024 x 24 at s = 50 000, 1024 x 1024 at s = 1000

Four ways on the same rows, alternating within one call, every way of every shape warmed up first:

    (a) range route   mhx_dist_contain as it schedules itself: one split, range pass, contain_finish_kernel
    (b) pair kernel   MHX_DIST_GENERIC=1: contain_pairs_kernel alone, one workgroup per pair
    (c) Jaccard path  mhx_dist_batch on the same rows: what `mash dist` costs here
    (d) host          numpy intersect1d per pair on 16 threads, on at most --host-pairs pairs and scaled to all of them

(a) and (b) run TWICE per round -- a1 b1 a2 b2 c -- so that the spread of one build against itself stands next to the
difference between the two.  Time: the kernel time of the call (mhx_last_dist_kernel_ms: device events around everything it
launches, flag read-backs included); (d) wall time.  The integers of (a) and (b) must be equal.

Keep rule: the range route stays if at 1024 x 24, s = 50 000 the median of (a) is below the median of (b) by more than the
larger of the two self-spreads |a1 - a2| and |b1 - b2| (medians).

    python tools/contain_rate.py [--rounds R] [--out FILE] [--shapes 1x24x50000,...] [--resources COMPILE_LOG]

--resources: a compile log of mhx_contain.hip made with -Rpass-analysis=kernel-resource-usage; its register, LDS, scratch
and occupancy lines are copied to the end of the output.
"""
import argparse
import os
import re
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21
KEEP_SHAPE = (1024, 24, 50000)


def mutated(rng, base, share):
    """`base` (s ascending hashes) with a share of them replaced by fresh values below its maximum: s ascending hashes again"""
    import numpy as np

    s = base.size
    drop = rng.random(s) < share
    v = np.unique(np.concatenate([base[~drop], rng.integers(0, int(base[-1]), size=int(drop.sum()), dtype=np.uint64)]))
    while v.size < s:   # a fresh value fell on a kept one
        v = np.unique(np.concatenate([v, rng.integers(0, int(base[-1]), size=s - v.size, dtype=np.uint64)]))
    return v[:s]


def clade_rows(n, s, seed):
    """n <= 64 lists of s hashes in four clades"""
    import numpy as np

    from triangle_rate import make_rows

    rng = np.random.default_rng(seed)
    bases, lens = make_rows(4, s, seed)
    rows = np.zeros((n, bases.shape[1]), np.uint64)
    for i in range(n):
        rows[i, :s] = mutated(rng, bases[i % 4, :s], 0.002 * 1.4 ** (i // 4 + i % 3))
    return rows, np.full(n, s, np.uint32)


def measure(nq, nr, s, rounds, host_pairs, say):
    import numpy as np
    import torch

    from triangle_rate import make_rows

    from auriclass_amd import engine

    L = engine.load()
    dev = "cuda:0"
    Q, ql = make_rows(nq, s, 7 + nq + s)
    R, rl = clade_rows(nr, s, nr + s) if nr <= 64 else make_rows(nr, s, nr + s)
    rng = np.random.default_rng(nq * 31 + nr)
    for i in range(0, nq, 8):   # every eighth query is a reference with 3 % of its hashes replaced: shared counts that are not zero
        Q[i, :s] = mutated(rng, R[i % nr, :s], 0.03)
    stride = Q.shape[1]
    d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, ql, R, rl)]
    out = {w: [torch.zeros((nq, nr), dtype=torch.int32, device=dev) for _ in range(3)] for w in ("a", "b")}
    jac = [torch.zeros((nq, nr), dtype=torch.int32, device=dev), torch.zeros((nq, nr), dtype=torch.int32, device=dev),
           torch.zeros((nq, nr), dtype=torch.float64, device=dev)]
    torch.cuda.synchronize()

    def contain(way):
        if way == "b":
            os.environ["MHX_DIST_GENERIC"] = "1"
        o = out[way]
        ms = engine.dist_contain_device(d[0].data_ptr(), d[1].data_ptr(), nq, s, d[2].data_ptr(), d[3].data_ptr(), nr, s, stride, o[0].data_ptr(),
                                        o[1].data_ptr(), o[2].data_ptr())
        os.environ.pop("MHX_DIST_GENERIC", None)
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    def jaccard():
        ms = engine.dist_batch_device(d[0].data_ptr(), d[1].data_ptr(), nq, d[2].data_ptr(), d[3].data_ptr(), nr, stride, K, s, jac[0].data_ptr(),
                                      jac[1].data_ptr(), jac[2].data_ptr())
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    def host():
        pairs = [(i, j) for i in range(nq) for j in range(nr)]
        step = max(1, len(pairs) // host_pairs)
        some = pairs[::step]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            got = list(pool.map(lambda p: np.intersect1d(Q[p[0], :s], R[p[1], :s], assume_unique=True).size, some))
        return (time.perf_counter() - t0) * 1e3 * len(pairs) / len(some), len(some), sum(got)

    order = ("a1", "b1", "a2", "b2", "c")
    calls = {"a1": lambda: contain("a"), "b1": lambda: contain("b"), "a2": lambda: contain("a"), "b2": lambda: contain("b"), "c": jaccard}
    info = {w: calls[w]()[1:] for w in order}   # warm-up: code objects, the workspace, the outputs' pages
    same = all(bool(torch.equal(x, y)) for x, y in zip(out["a"], out["b"]))
    times = {w: [] for w in order}
    for _ in range(rounds):
        for w in order:
            times[w].append(calls[w]()[0])
    host_ms, host_n, host_shared = host()
    med = {w: statistics.median(v) for w, v in times.items()}
    shared = int(out["a"][0].to(torch.int64).sum())
    say(f"{nq} queries x {nr} references, s = {s}: {nq * nr} pairs, {shared} shared hashes in all; the integers of (a) and (b) are equal: {same}")
    labels = {"a1": "(a) range route, first", "a2": "(a) range route, second", "b1": "(b) pair kernel, first", "b2": "(b) pair kernel, second",
              "c": "(c) mhx_dist_batch (Jaccard path)"}
    for w in ("a1", "a2", "b1", "b2", "c"):
        v = times[w]
        say(f"  {labels[w]:36s} R = {info[w][0]:5d}  fallback blocks {info[w][1]:3d}  ms: median {med[w]:9.4f}  best {min(v):9.4f}  worst {max(v):9.4f}   "
            f"{nq * nr / med[w] / 1e3:9.1f} M pairs/s   rounds " + " ".join(f"{x:.4f}" for x in v))
    say(f"  {'(d) numpy intersect1d, 16 threads':36s} {host_ms:9.1f} ms for all pairs, scaled from {host_n} pairs ({host_shared} shared hashes among them)")
    a, b = (med["a1"] + med["a2"]) / 2, (med["b1"] + med["b2"]) / 2
    spread = max(abs(med["a1"] - med["a2"]), abs(med["b1"] - med["b2"]))
    say(f"  (a) {a:.4f} ms, (b) {b:.4f} ms: (b) - (a) = {b - a:.4f} ms, self-spread {spread:.4f} ms ((a) {abs(med['a1'] - med['a2']):.4f}, (b) "
        f"{abs(med['b1'] - med['b2']):.4f});  (a) / (b) = {a / b:.3f}   (a) / (c) = {a / med['c']:.3f}   (d) / (a) = {host_ms / a:.0f}")
    if (nq, nr, s) == KEEP_SHAPE:
        routed = info["a1"][0] != 0 and info["a1"][1] == 0
        keep = routed and b - a > spread
        say(f"  KEEP RULE at this shape: the range route {'ran on every block' if routed else 'did NOT run on every block'}; it "
            f"{'beats' if b - a > spread else 'does NOT beat'} the pair kernel by more than the self-spread -> the range route {'STAYS' if keep else 'GOES'}")
    if not same:
        raise SystemExit("the range route and the pair kernel disagree")


def resource_lines(path):
    keep = re.compile(r"Function Name|SGPRs:|VGPRs:|ScratchSize|Occupancy|LDS Size")
    lines = []
    for line in Path(path).read_text().splitlines():
        if keep.search(line):
            lines.append("  " + line.split("remark:")[-1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip())
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x24x50000,1024x24x50000,1024x1024x1000")
    ap.add_argument("--host-pairs", type=int, default=256)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    from auriclass_amd import engine

    engine.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")

    say(f"tools/contain_rate.py on {engine.device_name()}: {args.rounds} rounds of a1 b1 a2 b2 c after a warm-up of each; kernel time of the call "
        "(mhx_last_dist_kernel_ms); (d) wall time")
    for shape in args.shapes.split(","):
        nq, nr, s = (int(x) for x in shape.split("x"))
        measure(nq, nr, s, args.rounds, args.host_pairs, say)
    if args.resources:
        say("resources of the kernels of mhx_contain.hip (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):")
        for line in resource_lines(args.resources):
            say(line)


if __name__ == "__main__":
    main()

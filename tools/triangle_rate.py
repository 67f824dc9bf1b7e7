"""What all pairs within one sketch set cost (mhx_dist_triangle), on synthetic INDEPENDENT sketches: every list holds s
values uniform below its own maximum (a genome's sketch: the s smallest of its hashes; the maxima differ as genome sizes
do), rows resident on the device, k = 21.

    shapes     n = 4096 and 16 384 at s = 1000, n = 2048 at s = 10 000

Three ways on the same rows, interleaved round by round, device pointers in and out:

    (a) triangle   mhx_dist_triangle with its own geometry (the smallest power of two R with s <= 16 R)
    (b) dist-geo   mhx_dist_triangle with MHX_TRI_GEOMETRY=dist (1024 x dist_windows(s) ranges)
    (c) square     mhx_dist_batch(set, set): the full [n][n] square, the yardstick (unchanged code)

The figure is the kernel time of a call (mhx_last_dist_kernel_ms: device events around everything the call launches,
flag read-backs between groups of blocks included).  After one warm-up of each way, every way is timed --rounds times
(default 5); median, best, worst and the spread are printed, with pairs/s of the pairs a way DELIVERS (n (n - 1) / 2 for
the triangle, n^2 for the square).  The results of (a) and (b) are compared with the lower triangle of (c).

    python tools/triangle_rate.py [--rounds R] [--out FILE] [--shapes 4096x1000,16384x1000,2048x10000]
    python tools/triangle_rate.py --once triangle|dist-geo|square --shapes 4096x1000   (two calls of one way: for a kernel trace)
"""
import argparse
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
K = 21


def make_rows(n, s, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    top = (rng.uniform(0.5, 1.0, size=(n, 1)) * float(2 ** 64 - 2 ** 12)).astype(np.uint64)   # per-list maximum
    stride = (s + 15) // 16 * 16   # rows of whole 128-byte lines
    rows = np.zeros((n, stride), np.uint64)
    rows[:, :s] = np.sort(rng.integers(0, top, size=(n, s), dtype=np.uint64), axis=1)
    if (rows[:, 1:s] <= rows[:, :s - 1]).any():
        raise SystemExit("a synthetic list holds a value twice; take another seed")
    return rows, np.full(n, s, np.uint32)


def measure(n, s, rounds, once, say):
    import numpy as np
    import torch

    from auriclass_amd import engine

    L = engine.load()
    rows, lens = make_rows(n, s, seed=n + s)
    dev = "cuda:0"
    d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    stride = rows.shape[1]
    pairs = n * (n - 1) // 2
    tri = [torch.zeros(pairs, dtype=torch.int32, device=dev), torch.zeros(pairs, dtype=torch.int32, device=dev),
           torch.zeros(pairs, dtype=torch.float64, device=dev)]
    torch.cuda.synchronize()

    def triangle(geometry):
        if geometry:
            os.environ["MHX_TRI_GEOMETRY"] = geometry
        else:
            os.environ.pop("MHX_TRI_GEOMETRY", None)
        ms = engine.dist_triangle_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, tri[0].data_ptr(), tri[1].data_ptr(), tri[2].data_ptr())
        os.environ.pop("MHX_TRI_GEOMETRY", None)
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    sq = None

    def square():
        nonlocal sq
        if sq is None:
            sq = [torch.zeros((n, n), dtype=torch.int32, device=dev), torch.zeros((n, n), dtype=torch.int32, device=dev),
                  torch.zeros((n, n), dtype=torch.float64, device=dev)]
            torch.cuda.synchronize()
        ms = engine.dist_batch_device(d_rows.data_ptr(), d_len.data_ptr(), n, d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s,
                                      sq[0].data_ptr(), sq[1].data_ptr(), sq[2].data_ptr())
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    ways = {"triangle": lambda: triangle(None), "dist-geo": lambda: triangle("dist"), "square": square}
    if once:
        ways[once]()
        ways[once]()
        return
    lower = torch.tril_indices(n, n, -1, device=dev)   # row-major lower triangle: the packed order
    info, times, same = {}, {w: [] for w in ways}, {}
    for w, call in ways.items():   # warm-up: code objects, the workspace, the outputs' pages
        _, ranges, fallbacks = call()
        info[w] = (ranges, fallbacks)
    for w in ("triangle", "dist-geo"):
        ways[w]()
        same[w] = bool(torch.equal(tri[0], sq[0][lower[0], lower[1]]) and torch.equal(tri[1], sq[1][lower[0], lower[1]]))
    for _ in range(rounds):
        for w, call in ways.items():
            times[w].append(call()[0])
    say(f"n = {n}, s = {s}, k = {K}: {pairs} pairs in the triangle, {n * n} in the square; common / denom of (a) and (b) equal "
        f"the square's lower triangle: {same['triangle']} / {same['dist-geo']}")
    med = {w: statistics.median(v) for w, v in times.items()}
    for w, label in (("triangle", "(a) mhx_dist_triangle, own geometry"), ("dist-geo", "(b) mhx_dist_triangle, MHX_TRI_GEOMETRY=dist"),
                     ("square", "(c) mhx_dist_batch(set, set)")):
        v = times[w]
        delivered = n * n if w == "square" else pairs
        say(f"  {label:46s} R = {info[w][0]:5d}  fallback blocks {info[w][1]}  kernel ms: median {med[w]:9.3f}  best {min(v):9.3f}  "
            f"worst {max(v):9.3f}  spread {100 * (max(v) / min(v) - 1):5.1f} %   {delivered / med[w] / 1e3:9.1f} M pairs/s   rounds "
            + " ".join(f"{x:.3f}" for x in v))
    say(f"  (a) / (c) = {med['triangle'] / med['square']:.3f}   (b) / (c) = {med['dist-geo'] / med['square']:.3f}   (a) / (b) = "
        f"{med['triangle'] / med['dist-geo']:.3f}   (medians; the expectation for the triangle is at most 0.6 of the square)")
    if not all(same.values()):
        raise SystemExit("the triangle and the square disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="4096x1000,16384x1000,2048x10000")
    ap.add_argument("--once", choices=("triangle", "dist-geo", "square"), default=None)
    args = ap.parse_args()
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    from auriclass_amd import engine

    engine.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    shapes = [tuple(int(x) for x in shape.split("x")) for shape in args.shapes.split(",")]
    if not args.once:
        say(f"tools/triangle_rate.py on {engine.device_name()}: {args.rounds} interleaved rounds after a warm-up of each way, kernel time "
            "of a call (mhx_last_dist_kernel_ms)")
    for n, s in shapes:
        measure(n, s, args.rounds, args.once, say)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

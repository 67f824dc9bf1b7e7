"""What complete and average linkage of one sketch set cost on the device (mhx_dist_linkage), against what a user does
today: the whole triangle pulled to the host and scipy.cluster.hierarchy.linkage over it.  One synthetic set with planted
chains per shape (tools/cluster_rate.py's), k = 21, both linkages.

Ways, interleaved round by round, each timed with a host clock around a call that is complete when it returns:

    (a) linkage, device   engine.dist_linkage_device: rows resident on the device, the merges left there
    (b) linkage, host     engine.dist_linkage: rows staged from the host, the merges copied back, heights on the host
    (c) triangle + scipy  engine.dist_triangle (host form), the packed lower triangle turned into scipy's condensed form, then
                          scipy.cluster.hierarchy.linkage(method = complete | average); left out, and said so, without scipy
    (t) one mhx_dist_triangle, device pointers, kernel time: what the call spends before its first step

Before anything is timed the merges (ids and sizes, hence the memberships of every merged cluster) of (a) and (b) must be
equal.  After one warm-up of each way, every way is timed --rounds times (default 7); median, best, worst and spread are
printed, then the steps per second, the rows scanned again per step and the kernel time outside the triangle.  A step is
three launches (pick, update, rescan); the host enqueues all of them without a readback in between.

    python tools/linkage_rate.py [--rounds R] [--user-rounds U] [--shapes 4096x1000,8192x1000] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21
NAMES = {1: "complete", 2: "average"}


def scipy_linkage(n, dist, method):
    """what a user writes: the packed lower triangle (pair (i, j), j < i, at i (i - 1) / 2 + j) as scipy's condensed upper
    triangle, then the hierarchy"""
    import numpy as np
    from scipy.cluster.hierarchy import linkage

    square = np.zeros((n, n), np.float64)
    square[np.tril_indices(n, -1)] = dist
    condensed = square.T[np.triu_indices(n, 1)]
    return linkage(condensed, method=method)


def measure(shape, args, say, have_scipy):
    import numpy as np
    import torch

    from auriclass_amd import engine
    from cluster_rate import make_set

    L = engine.load()
    n, s = (int(x) for x in shape.split("x"))
    rows, lens, planted = make_set(n, s, seed=n + s)
    dev = "cuda:0"
    d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d32 = [torch.zeros(n - 1, dtype=torch.int32, device=dev) for _ in range(3)]
    d64 = [torch.zeros(n - 1, dtype=torch.int64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stride = rows.shape[1]
    kernel_ms = {("device", 1): [], ("device", 2): [], "triangle": []}
    rescans = {}

    def way_device(linkage):
        t0 = time.perf_counter()
        engine.dist_linkage_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, linkage, *(o.data_ptr() for o in d32), *(o.data_ptr() for o in d64))
        took = time.perf_counter() - t0
        kernel_ms[("device", linkage)].append(L.mhx_last_dist_kernel_ms())
        rescans[linkage] = L.mhx_last_linkage_rescans()
        return took, [o.cpu().numpy().view(np.uint32) for o in d32]

    def way_host(linkage):
        t0 = time.perf_counter()
        got = engine.dist_linkage(rows, lens, K, s, linkage)
        return time.perf_counter() - t0, list(got[:3])

    def way_user(linkage):
        t0 = time.perf_counter()
        _, _, dist = engine.dist_triangle(rows, lens, K, s)
        t1 = time.perf_counter()
        scipy_linkage(n, dist, NAMES[linkage])
        return time.perf_counter() - t0, t1 - t0

    def way_triangle():
        pairs = n * (n - 1) // 2
        c = torch.zeros(pairs, dtype=torch.int32, device=dev)
        d = torch.zeros(pairs, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.mhx_dist_triangle(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, c.data_ptr(), d.data_ptr(), None, 1)
        if rc:
            raise SystemExit(f"mhx_dist_triangle failed: {rc}")
        kernel_ms["triangle"].append(L.mhx_last_dist_kernel_ms())

    # warm-up and the equality of the two forms
    same = True
    for linkage in (1, 2):
        _, got_a = way_device(linkage)
        _, got_b = way_host(linkage)
        same = same and all(np.array_equal(x, y) for x, y in zip(got_a, got_b)) and int(got_a[2][-1]) == n
        if have_scipy:
            way_user(linkage)
    way_triangle()
    say(f"tools/linkage_rate.py on {engine.device_name()}: n = {n}, s = {s}, k = {K}: {n * (n - 1) // 2} pairs, {n - 1} steps of 3 launches "
        f"({planted} planted chain links); R = {L.mhx_last_dist_ranges()}, fallback blocks {L.mhx_last_dist_fallback_blocks()}; "
        f"merges of the device form and the host form equal: {same}")
    if not same:
        raise SystemExit("the device form and the host form disagree")
    for key in kernel_ms:
        kernel_ms[key].clear()
    wall = {(w, lk): [] for w in ("device", "host", "user", "user_triangle") for lk in (1, 2)}
    for r in range(args.rounds):
        for linkage in (1, 2):
            wall[("device", linkage)].append(way_device(linkage)[0])
            wall[("host", linkage)].append(way_host(linkage)[0])
            if have_scipy and r < args.user_rounds:
                took, first = way_user(linkage)
                wall[("user", linkage)].append(took)
                wall[("user_triangle", linkage)].append(first)
        way_triangle()

    def row(label, v, unit="ms", scale=1e3):
        v = [x * scale for x in v]
        say(f"  {label:58s} median {statistics.median(v):10.3f} {unit}  best {min(v):10.3f}  worst {max(v):10.3f}  spread {100 * (max(v) / min(v) - 1):5.1f} %   rounds "
            + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)
    say(f"{args.rounds} interleaved rounds ({args.user_rounds if have_scipy else 0} of (c)) after a warm-up of each way; wall = host clock around a call that is complete when it returns")
    t = row("(t) one mhx_dist_triangle, device pointers, kernel time", kernel_ms["triangle"], scale=1.0)
    for linkage in (1, 2):
        say(f" {NAMES[linkage]} linkage")
        a = row("(a) dist_linkage_device, wall", wall[("device", linkage)])
        ka = row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms[("device", linkage)], scale=1.0)
        row("(b) dist_linkage (host pointers), wall", wall[("host", linkage)])
        if have_scipy:
            c = row("(c) dist_triangle + scipy linkage, wall", wall[("user", linkage)])
            row("    of which dist_triangle, wall", wall[("user_triangle", linkage)])
            say(f"  (a) / (c) = {a / c:.4f}   (medians of the wall times)")
        else:
            say("  (c) left out: scipy is not installed here")
        steps_ms = ka - t
        say(f"  kernel time outside the triangle {ka:.3f} - {t:.3f} = {steps_ms:.3f} ms: {(n - 1) / (steps_ms / 1e3):.0f} steps / s, {steps_ms * 1e3 / (n - 1):.2f} us per step "
            f"of 3 launches; rows scanned again {rescans[linkage]}, {rescans[linkage] / (n - 1):.2f} per step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--user-rounds", type=int, default=7)
    ap.add_argument("--shapes", default="4096x1000,8192x1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.user_rounds = max(1, min(args.user_rounds, args.rounds))
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    from auriclass_amd import engine

    try:
        import scipy.cluster.hierarchy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    engine.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    for shape in args.shapes.split(","):
        measure(shape, args, say, have_scipy)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""What the single-linkage tree of one sketch set costs (mhx_dist_mst) in its two pair sources, against what a user did
before it existed: the whole triangle pulled to the host, an argsort of all pairs and a union-find in Python.  One synthetic
set with planted chains per shape (tools/cluster_rate.py's: n / 16 clades of 8 lists, every next one its predecessor with
15 % of the hashes replaced, the other half independent, all permuted), k = 21.

Ways, interleaved round by round, each timed with a host clock around a call that is complete when it returns:

    (a) tree, device, stored      engine.dist_mst_device under MHX_MST_STORE=1: rows resident on the device, the packed
                                  triangle written once, every round one pass over it
    (b) tree, device, recomputed  the same under MHX_MST_STORE=0: the triangle's blocks run again every round, O(n) workspace
    (c) tree, host                engine.dist_mst: rows staged from the host, the edges sorted and copied back (default source)
    (d) triangle + host Kruskal   engine.dist_triangle (host form), numpy's lexsort by (-common / denom, lo, hi), a union-find
                                  in Python that stops at n - 1 edges; fewer rounds (--user-rounds): it takes seconds
    (t) one mhx_dist_triangle     device pointers, kernel time: the baseline the recomputed form multiplies

Before anything is timed the edge sets of (a), (b), (c) and (d) must be equal.  After one warm-up of each way, every way is
timed --rounds times (default 7); median, best, worst and spread are printed, then (a) / (d), (b) / (a), the rounds taken and
the kernel time per round of either source against (t).

    python tools/mst_rate.py [--rounds R] [--user-rounds U] [--shapes 4096x1000,8192x1000] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21


def host_kruskal(n, common, denom):
    """what a user writes: all pairs sorted by the index (descending), then (lo, hi); a union-find until the tree is whole"""
    import numpy as np

    ii = np.repeat(np.arange(n, dtype=np.uint32), np.arange(n))   # pair (i, j) at i (i - 1) / 2 + j
    jj = (np.arange(ii.size, dtype=np.int64) - ii.astype(np.int64) * (ii.astype(np.int64) - 1) // 2).astype(np.uint32)
    jac = np.where(common == denom, 1.0, common / np.maximum(denom, 1))
    order = np.lexsort((ii, jj, -jac))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    tree = []
    for e in order.tolist():
        a, b = find(int(ii[e])), find(int(jj[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            tree.append((int(ii[e]), int(jj[e]), int(common[e]), int(denom[e])))
            if len(tree) == n - 1:
                break
    return tree


def measure(shape, args, say):
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
    d_out = [torch.zeros(n - 1, dtype=torch.int32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    stride = rows.shape[1]
    kernel_ms = {"stored": [], "recomputed": [], "triangle": []}
    rounds_taken = {}

    def way_device(store):
        os.environ["MHX_MST_STORE"] = "1" if store else "0"
        t0 = time.perf_counter()
        engine.dist_mst_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, *(o.data_ptr() for o in d_out))
        took = time.perf_counter() - t0
        del os.environ["MHX_MST_STORE"]
        key = "stored" if store else "recomputed"
        kernel_ms[key].append(L.mhx_last_dist_kernel_ms())
        rounds_taken[key] = L.mhx_last_mst_rounds()
        return took, sorted(zip(*(o.cpu().numpy().view(np.uint32).tolist() for o in d_out)))

    def way_host():
        t0 = time.perf_counter()
        ei, ej, ec, ed, _ = engine.dist_mst(rows, lens, K, s)
        return time.perf_counter() - t0, sorted(zip(ei.tolist(), ej.tolist(), ec.tolist(), ed.tolist()))

    def way_user():
        t0 = time.perf_counter()
        common, denom, _ = engine.dist_triangle(rows, lens, K, s)
        t1 = time.perf_counter()
        tree = host_kruskal(n, common, denom)
        return time.perf_counter() - t0, sorted(tree), t1 - t0

    def way_triangle():
        pairs = n * (n - 1) // 2
        c = torch.zeros(pairs, dtype=torch.int32, device=dev)
        d = torch.zeros(pairs, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.mhx_dist_triangle(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, c.data_ptr(), d.data_ptr(), None, 1)
        if rc:
            raise SystemExit(f"mhx_dist_triangle failed: {rc}")
        kernel_ms["triangle"].append(L.mhx_last_dist_kernel_ms())

    # warm-up and the equality of the four results
    _, set_a = way_device(True)
    _, set_b = way_device(False)
    _, set_c = way_host()
    _, set_d, _ = way_user()
    way_triangle()
    same = set_a == set_b == set_c == set_d and len(set_a) == n - 1
    say(f"tools/mst_rate.py on {engine.device_name()}: n = {n}, s = {s}, k = {K}: {n * (n - 1) // 2} pairs, {n - 1} tree edges, "
        f"{sum(1 for e in set_a if e[2])} of them with a shared hash ({planted} planted); R = {L.mhx_last_dist_ranges()}, "
        f"fallback blocks {L.mhx_last_dist_fallback_blocks()}; rounds: stored {rounds_taken['stored']}, recomputed {rounds_taken['recomputed']}; "
        f"edge sets of the four ways equal: {same}")
    if not same:
        raise SystemExit("the tree's forms and the host Kruskal disagree")
    for key in kernel_ms:
        kernel_ms[key].clear()
    wall = {"stored": [], "recomputed": [], "host": [], "user": []}
    user_triangle = []
    for r in range(args.rounds):
        wall["stored"].append(way_device(True)[0])
        wall["recomputed"].append(way_device(False)[0])
        wall["host"].append(way_host()[0])
        way_triangle()
        if r < args.user_rounds:
            took, _, first = way_user()
            wall["user"].append(took)
            user_triangle.append(first)

    def row(label, v, unit="ms", scale=1e3):
        v = [x * scale for x in v]
        say(f"  {label:58s} median {statistics.median(v):9.3f} {unit}  best {min(v):9.3f}  worst {max(v):9.3f}  spread {100 * (max(v) / min(v) - 1):5.1f} %   rounds "
            + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)
    say(f"{args.rounds} interleaved rounds ({args.user_rounds} of (d)) after a warm-up of each way; wall = host clock around a call that is complete when it returns")
    a = row("(a) dist_mst_device, stored, wall", wall["stored"])
    ka = row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms["stored"], scale=1.0)
    b = row("(b) dist_mst_device, recomputed, wall", wall["recomputed"])
    kb = row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms["recomputed"], scale=1.0)
    row("(c) dist_mst (host pointers), wall", wall["host"])
    d = row("(d) dist_triangle + lexsort + union-find in Python, wall", wall["user"])
    row("    of which dist_triangle, wall", user_triangle)
    t = row("(t) one mhx_dist_triangle, device pointers, kernel time", kernel_ms["triangle"], scale=1.0)
    ra, rb = rounds_taken["stored"], rounds_taken["recomputed"]
    say(f"  (a) / (d) = {a / d:.4f}   (b) / (a) = {b / a:.3f}   (medians of the wall times)")
    say(f"  per round: stored ({ka:.3f} - {t:.3f}) / {ra} = {(ka - t) / ra:.3f} ms   recomputed {kb:.3f} / {rb} = {kb / rb:.3f} ms = {kb / rb / t:.3f} triangles")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--user-rounds", type=int, default=2)
    ap.add_argument("--shapes", default="4096x1000,8192x1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.user_rounds = max(1, min(args.user_rounds, args.rounds))
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    from auriclass_amd import engine

    engine.init(0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    for shape in args.shapes.split(","):
        measure(shape, args, say)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

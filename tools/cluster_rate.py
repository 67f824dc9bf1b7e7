"""What the single-linkage clustering of one sketch set costs (mhx_dist_cluster) against what a user did before it existed:
the edge list of the same bound (mhx_dist_triangle_edges, host form: exact) pulled to the host, and a union-find over it in
Python.  One synthetic set with planted clades, k = 21:

    n lists of s hashes (default 8192 x 1000): n / 16 clades of 8 lists -- a fresh list, and every next one its predecessor
    with 15 % of the hashes replaced (0.006 .. 0.009 apart; two steps apart 0.0127 and more) --, the other half independent
    lists, all permuted.  At the bound 0.011 the edges are the 7 consecutive pairs of every clade.

Ways, interleaved round by round, each timed with a host clock around a call that is complete when it returns:

    (a) cluster, device   engine.dist_cluster_device: rows resident on the device, labels and degrees left there
                          (also: mhx_last_dist_kernel_ms of the call, device events around everything it launches)
    (b) cluster, host     engine.dist_cluster: rows staged from the host, labels and degrees copied back
    (c) edges + host UF   engine.dist_triangle_edges (rows staged from the host, the list filtered, sorted and copied back),
                          then a union-find with path halving over the list in Python and numpy's bincount for the degrees

Before anything is timed the labels, degrees and counts of (a), (b) and (c) must be equal.  After one warm-up of each way,
every way is timed --rounds times (default 7); median, best, worst and spread are printed.  A last line times (a) at the
bound 1.0, where every pair is an edge: the most unions and the most contended degree counters the set can ask for.

    python tools/cluster_rate.py [--rounds R] [--shape 8192x1000] [--bound 0.011] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
K = 21


def make_set(n, s, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    stride = (s + 15) // 16 * 16   # rows of whole 128-byte lines
    rows = np.zeros((n, stride), np.uint64)
    fresh = lambda count: np.sort(rng.integers(0, 2 ** 64 - 2 ** 12, size=(count, s), dtype=np.uint64), axis=1)   # noqa: E731
    clades, members = n // 16, 8
    lists = fresh(n - clades * (members - 1))
    out = []
    for c in range(clades):
        cur = lists[c]
        out.append(cur)
        for _ in range(members - 1):
            cur = cur.copy()
            at = rng.random(s) < 0.15
            cur[at] = rng.integers(0, 2 ** 64 - 2 ** 12, size=int(at.sum()), dtype=np.uint64)
            cur.sort()
            out.append(cur)
    out.extend(lists[clades:])
    order = rng.permutation(n)
    for to, src in enumerate(order):
        rows[to, :s] = out[src]
    if (rows[:, 1:s] <= rows[:, :s - 1]).any():
        raise SystemExit("a synthetic list holds a value twice; take another seed")
    return rows, np.full(n, s, np.uint32), clades * (members - 1)


def host_union_find(n, ei, ej):
    """what a user writes: labels = the lowest index of every component"""
    import numpy as np

    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in zip(ei.tolist(), ej.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([find(i) for i in range(n)], np.uint32)
    degree = (np.bincount(ei, minlength=n) + np.bincount(ej, minlength=n)).astype(np.uint32)
    return label, degree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", default="8192x1000")
    ap.add_argument("--bound", type=float, default=0.011)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the engine's library: the two then share one device runtime)

    from auriclass_amd import engine

    engine.init(0)
    L = engine.load()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    n, s = (int(x) for x in args.shape.split("x"))
    rows, lens, planted = make_set(n, s, seed=n + s)
    dev = "cuda:0"
    d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_label = torch.zeros(n, dtype=torch.int32, device=dev)
    d_degree = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stride = rows.shape[1]
    kernel_ms = {"device": [], "edges": []}

    def way_device():
        t0 = time.perf_counter()
        res = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, args.bound, d_label.data_ptr(), d_degree.data_ptr())
        took = time.perf_counter() - t0
        kernel_ms["device"].append(L.mhx_last_dist_kernel_ms())
        return took, res

    def way_host():
        t0 = time.perf_counter()
        res = engine.dist_cluster(rows, lens, K, s, args.bound)
        return time.perf_counter() - t0, res

    def way_edges():
        t0 = time.perf_counter()
        ei, ej, _, _, _ = engine.dist_triangle_edges(rows, lens, K, s, args.bound)
        t1 = time.perf_counter()
        kernel_ms["edges"].append(L.mhx_last_dist_kernel_ms())
        label, degree = host_union_find(n, ei, ej)
        t2 = time.perf_counter()
        return t2 - t0, (label, degree, int((label == np.arange(n)).sum()), int(ei.size)), t1 - t0

    # warm-up and the equality of the three results
    _, (clusters_a, edges_a) = way_device()
    label_a, degree_a = d_label.cpu().numpy().view(np.uint32), d_degree.cpu().numpy().view(np.uint32)
    _, (label_b, degree_b, clusters_b, edges_b) = way_host()
    _, (label_c, degree_c, clusters_c, edges_c), _ = way_edges()
    same = (np.array_equal(label_a, label_b) and np.array_equal(label_a, label_c) and np.array_equal(degree_a, degree_b) and np.array_equal(degree_a, degree_c)
            and (clusters_a, edges_a) == (clusters_b, edges_b) == (clusters_c, edges_c))
    say(f"tools/cluster_rate.py on {engine.device_name()}: n = {n}, s = {s}, k = {K}, bound {args.bound}: {n * (n - 1) // 2} pairs, {edges_a} edges "
        f"({planted} planted), {clusters_a} clusters; R = {L.mhx_last_dist_ranges()}, fallback blocks {L.mhx_last_dist_fallback_blocks()}; "
        f"labels, degrees and counts of the three ways equal: {same}")
    if not same:
        raise SystemExit("the clustering and the edge list with a host union-find disagree")
    for key in kernel_ms:
        kernel_ms[key].clear()
    wall = {"device": [], "host": [], "edges": []}
    edges_only = []
    for _ in range(args.rounds):
        wall["device"].append(way_device()[0])
        wall["host"].append(way_host()[0])
        took, _, first = way_edges()
        wall["edges"].append(took)
        edges_only.append(first)

    def row(label, v, unit="ms", scale=1e3):
        v = [x * scale for x in v]
        say(f"  {label:58s} median {statistics.median(v):9.3f} {unit}  best {min(v):9.3f}  worst {max(v):9.3f}  spread {100 * (max(v) / min(v) - 1):5.1f} %   rounds "
            + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)
    say(f"{args.rounds} interleaved rounds after a warm-up of each way; wall = host clock around a call that is complete when it returns")
    a = row("(a) dist_cluster_device, wall", wall["device"])
    row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms["device"], scale=1.0)
    b = row("(b) dist_cluster (host pointers), wall", wall["host"])
    c = row("(c) dist_triangle_edges + union-find in Python, wall", wall["edges"])
    row("    of which dist_triangle_edges, wall", edges_only)
    row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms["edges"], scale=1.0)
    say(f"  (a) / (c) = {a / c:.3f}   (b) / (c) = {b / c:.3f}   (medians of the wall times)")
    # the most unions and the most contended counters a set of this size can ask for: every pair an edge, one cluster
    full = []
    for _ in range(1 + min(3, args.rounds)):
        res = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, 1.0, d_label.data_ptr(), d_degree.data_ptr())
        full.append(L.mhx_last_dist_kernel_ms())
    ok = res == (1, n * (n - 1) // 2) and not d_label.any().item() and bool((d_degree == n - 1).all().item())
    row(f"(d) dist_cluster_device at the bound 1.0 (every pair an edge), kernel time; result as expected: {ok}", full[1:], scale=1.0)
    if not ok:
        raise SystemExit("the bound 1.0 did not give one cluster of all pairs")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

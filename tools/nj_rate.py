"""What neighbour joining over one sketch set costs on the device (mhx_dist_nj), against what a user does today: the whole
triangle pulled to the host and a neighbour-joining tool over it -- here a vectorised float64 neighbour joining in numpy, its
Q matrix computed in row blocks on 16 threads.  That is the textbook algorithm in floating point (no clamp, no fixed point,
ties wherever rounding puts them), so only TIMES are compared, never trees.  One synthetic set with planted clades per shape
(tools/cluster_rate.py's), k = 21.

Ways, each timed with a host clock around a call that is complete when it returns:

    (a) nj, device        engine.dist_nj_device: rows resident on the device, the records left there
    (b) nj, host          engine.dist_nj: rows staged from the host, the records copied back, lengths on the host
    (c) triangle + numpy  engine.dist_triangle (host form), the packed lower triangle as a square matrix, then numpy_nj;
                          run once per shape, and left out -- and said so -- where n^3 scaling of the shape before puts it
                          beyond --numpy-limit seconds
    (t) one mhx_dist_triangle, device pointers, kernel time: what the call spends before its first join

Before anything is timed the records and lengths of (a) and (b) must be the same bytes.  The pick scan reads the words of all
active rows once per join: its bytes are computed from the records (8 bytes per word, the sum of the active ids per join) and
divided by the kernel time outside the triangle -- the time of ALL three launches of all joins, so the figure is a lower
bound of the scan's own rate -- and printed next to the measured HBM copy rate of the chip.  A shape whose time, scaled by n^3
from the shape before, would pass --limit seconds is left out, and said so.

    python tools/nj_rate.py [--rounds R] [--shapes 1024x1000,4096x1000,16384x1000] [--limit 60] [--numpy-limit 300] [--long-call 5] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21
THREADS = 16
HBM_MEASURED = 6.29e12   # bytes / s, float4 copy on one MI355X (8.0e12 by the data sheet)


def numpy_nj(D, pool):
    """textbook neighbour joining over the square float64 matrix D (used up): [(i, j, len_i, len_j)] by position-free ids"""
    import numpy as np

    n = D.shape[0]
    ids = np.arange(n)
    np.fill_diagonal(D, 0.0)
    r = D.sum(axis=1)
    m = n
    out = []

    def part(lo, hi):
        q = D[lo:hi, :m] * (m - 2.0)
        q -= r[lo:hi, None]
        q -= r[None, :m]
        q[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        at = int(q.argmin())
        return float(q.flat[at]), lo + at // m, at % m
    while m > 2:
        step = -(-m // THREADS)
        _, i, j = min(pool.map(lambda lo: part(lo, min(lo + step, m)), range(0, m, step)))
        if j < i:
            i, j = j, i
        dij = D[i, j]
        out.append((int(ids[i]), int(ids[j]), 0.5 * dij + (r[i] - r[j]) / (2.0 * (m - 2)), 0.5 * dij + (r[j] - r[i]) / (2.0 * (m - 2))))
        new = 0.5 * (D[i, :m] + D[j, :m] - dij)
        new[i] = new[j] = 0.0
        r[:m] += new - D[i, :m] - D[j, :m]
        r[i] = new.sum()
        D[i, :m] = new
        D[:m, i] = new
        last = m - 1   # position j takes the last node
        D[j, :m] = D[last, :m]
        D[:m, j] = D[:m, last]
        D[j, j] = 0.0
        r[j] = r[last]
        ids[j] = ids[last]
        m -= 1
    if n >= 2:
        out.append((int(ids[0]), int(ids[1]), float(D[0, 1]), 0.0))
    return out


def scan_words(n, join_a):
    """the words the pick scans of a call read: the sum of the active ids at every join among more than two nodes"""
    total, left = 0, n * (n - 1) // 2
    for t in range(n - 2):
        total += left
        left -= int(join_a[t])
    return total


def measure(shape, args, say, before):
    import numpy as np
    import torch

    from auriclass_amd import engine
    from cluster_rate import make_set

    L = engine.load()
    n, s = (int(x) for x in shape.split("x"))
    if before is not None and before["device"] * (n / before["n"]) ** 3 > args.limit:
        say(f"n = {n}, s = {s}: left out: {before['device']:.2f} s at n = {before['n']} scaled by n^3 is {before['device'] * (n / before['n']) ** 3:.0f} s, beyond {args.limit:.0f} s")
        return before
    rows, lens, planted = make_set(n, s, seed=n + s)
    dev = "cuda:0"
    d_rows = torch.from_numpy(rows.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d32 = [torch.zeros(n - 1, dtype=torch.int32, device=dev) for _ in range(2)]
    d64 = [torch.zeros(n - 1, dtype=torch.int64, device=dev) for _ in range(3)]
    f64 = [torch.zeros(n - 1, dtype=torch.float64, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stride = rows.shape[1]
    kernel_ms, tri_ms = [], []

    def way_device():
        t0 = time.perf_counter()
        engine.dist_nj_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, *(o.data_ptr() for o in d32 + d64 + f64))
        took = time.perf_counter() - t0
        kernel_ms.append(L.mhx_last_dist_kernel_ms())
        return took

    def way_host():
        t0 = time.perf_counter()
        got = engine.dist_nj(rows, lens, K, s)
        return time.perf_counter() - t0, got

    def way_triangle():
        pairs = n * (n - 1) // 2
        c = torch.zeros(pairs, dtype=torch.int32, device=dev)
        d = torch.zeros(pairs, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = L.mhx_dist_triangle(d_rows.data_ptr(), d_len.data_ptr(), n, stride, K, s, c.data_ptr(), d.data_ptr(), None, 1)
        if rc:
            raise SystemExit(f"mhx_dist_triangle failed: {rc}")
        tri_ms.append(L.mhx_last_dist_kernel_ms())

    # warm-up and the equality of the two forms
    warm = way_device()
    clamps = L.mhx_last_nj_clamps()
    warm_host, host = way_host()
    got = [o.cpu().numpy() for o in d32 + d64 + f64]
    same = all(x.tobytes() == y.tobytes() for x, y in zip(got, host))
    way_triangle()
    words = scan_words(n, host[0])
    say(f"tools/nj_rate.py on {engine.device_name()}: n = {n}, s = {s}, k = {K}: {n * (n - 1) // 2} pairs, {n - 1} joins of 3 launches ({planted} planted clade "
        f"links); R = {L.mhx_last_dist_ranges()}; records and lengths of the device form and the host form the same bytes: {same}; updates clamped {clamps}; "
        f"negative branch lengths {int((host[5] < 0).sum() + (host[6] < 0).sum())}")
    if not same:
        raise SystemExit("the device form and the host form disagree")
    wall = {"device": [warm], "host": [warm_host]}
    if warm < args.long_call:
        kernel_ms.clear()
        tri_ms.clear()
        wall = {"device": [], "host": []}
        for _ in range(args.rounds):
            wall["device"].append(way_device())
            wall["host"].append(way_host()[0])
            way_triangle()
        say(f"{args.rounds} interleaved rounds after a warm-up of each way; wall = host clock around a call that is complete when it returns")
    else:
        say(f"a call takes more than {args.long_call:.0f} s: the first call of each way is the one timed; wall = host clock around a call that is complete when it returns")

    def row(label, v, unit="ms", scale=1e3):
        v = [x * scale for x in v]
        say(f"  {label:58s} median {statistics.median(v):11.3f} {unit}  best {min(v):11.3f}  worst {max(v):11.3f}  spread {100 * (max(v) / min(v) - 1):5.1f} %   rounds "
            + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)
    t = row("(t) one mhx_dist_triangle, device pointers, kernel time", tri_ms, scale=1.0)
    a = row("(a) dist_nj_device, wall", wall["device"])
    ka = row("    its kernel time (mhx_last_dist_kernel_ms)", kernel_ms, scale=1.0)
    row("(b) dist_nj (host pointers), wall", wall["host"])
    joins_ms = ka - t
    rate = 8 * words / (joins_ms / 1e3)
    say(f"  kernel time outside the triangle {ka:.3f} - {t:.3f} = {joins_ms:.3f} ms: {(n - 1) / (joins_ms / 1e3):.0f} joins / s, {joins_ms * 1e3 / (n - 1):.2f} us per join of 3 launches")
    say(f"  the pick scans read {words} words = {8 * words / 1e9:.2f} GB ({words / n ** 3:.3f} n^3 words; the words of the call: {8 * n * (n - 1) // 2 / 1e6:.0f} MB): over that time "
        f"{rate / 1e12:.3f} TB/s, a lower bound of the scan's own rate (the time holds all three launches), {100 * rate / HBM_MEASURED:.0f} % of the {HBM_MEASURED / 1e12:.2f} TB/s "
        f"an HBM copy reaches here (8.0 by the data sheet); words that fit the 256 MB Infinity Cache need not come from HBM")
    numpy_s = None
    guess = None if before is None or before.get("numpy") is None else before["numpy"] * (n / before["n"]) ** 3
    if guess is not None and guess > args.numpy_limit:
        say(f"  (c) left out: {before['numpy']:.1f} s at n = {before['n']} scaled by n^3 is {guess:.0f} s, beyond {args.numpy_limit:.0f} s")
        numpy_s, n_numpy = before["numpy"], before["n"]
    else:
        with ThreadPoolExecutor(THREADS) as pool:
            t0 = time.perf_counter()
            _, _, dist = engine.dist_triangle(rows, lens, K, s)
            t1 = time.perf_counter()
            square = np.zeros((n, n), np.float64)
            square[np.tril_indices(n, -1)] = dist
            square += square.T
            numpy_nj(square, pool)
            t2 = time.perf_counter()
        say(f"  (c) dist_triangle + numpy float64 neighbour joining on {THREADS} threads, wall, one run: {(t2 - t0) * 1e3:.0f} ms, of which dist_triangle {(t1 - t0) * 1e3:.0f} ms")
        say(f"  (a) / (c) = {a / ((t2 - t0) * 1e3):.4f}   (a different algorithm: times only)")
        numpy_s, n_numpy = t2 - t0, n
    return {"n": n_numpy, "device": a / 1e3 * (n_numpy / n) ** 3, "numpy": numpy_s}   # (both scale by n^3 from the same n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="1024x1000,4096x1000,16384x1000")
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--numpy-limit", type=float, default=300.0)
    ap.add_argument("--long-call", type=float, default=5.0, help="seconds of one call beyond which no further rounds are run")
    ap.add_argument("--out", default=None)
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
    before = None
    for shape in args.shapes.split(","):
        before = measure(shape, args, say, before)


if __name__ == "__main__":
    main()

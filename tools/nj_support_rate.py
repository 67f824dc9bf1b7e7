"""What the jackknife support of a neighbour-joining tree costs on the device (mhx_dist_nj_support) at R = 100 replicates,
against the path a user had before it: R times (resample the lists in numpy on the host, then engine.dist_nj over them).  One
synthetic set with planted clades per shape (tools/cluster_rate.py's), k = 21, keep = 0.5, seed = 42.

Ways, each timed with a host clock around calls that are complete when they return:

    (a) support, host     engine.dist_nj_support: rows staged from the host once, everything allocated once, R replicates of
                          resample, cut, a 4-byte readback, triangle, init and joins, the splits counted on the host as they come
    (b) numpy + dist_nj   the main tree by engine.dist_nj, then per replicate the keep function over all hashes in numpy
                          (vectorised uint64), the cut, a fresh row matrix, engine.dist_nj at sketch size s_r; and
                          engine.nj_split_support over the joins at the end

Before anything is timed the two ways must agree: the same main records, the same joins of every replicate, the same support.
A shape whose time would pass --limit seconds, scaled by n^2 from the shape before (below a few thousand lists a join is bound by
its launches, so a tree costs less than n^3 says), is left out, and said so.

    python tools/nj_support_rate.py [--replicates 100] [--rounds 2] [--shapes 24x1000,256x1000,2048x1000] [--limit 120] [--out FILE]
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
KEEP, SEED = 0.5, 42


def numpy_replicate(rows, lens, s, seed, r, keep):
    """the rule of include/mhx.h in numpy: (rows, lens, s_r) of replicate r"""
    import numpy as np

    u = np.uint64
    with np.errstate(over="ignore"):
        z = rows + u((seed + (r + 1) * 0x9E3779B97F4A7C15) % 2 ** 64)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z ^= z >> u(31)
    inside = np.arange(rows.shape[1])[None, :] < lens[:, None]
    kept = ((z >> u(32)) < u(int(keep * 2.0 ** 32))) & inside
    count = kept.sum(axis=1)
    full = count[lens == s]
    s_r = int(full.min()) if full.size else s
    out = np.zeros_like(rows)
    out_len = np.minimum(count, s_r).astype(np.uint32)
    for i in range(rows.shape[0]):
        out[i, :out_len[i]] = rows[i, kept[i]][:out_len[i]]
    return out, out_len, s_r


def measure(shape, args, say, before):
    import numpy as np

    from auriclass_amd import engine
    from cluster_rate import make_set

    n, s = (int(x) for x in shape.split("x"))
    R = args.replicates
    if before is not None and before["t"] * (n / before["n"]) ** 2 > args.limit:
        say(f"n = {n}, s = {s}: left out: {before['t']:.2f} s at n = {before['n']} scaled by n^2 is {before['t'] * (n / before['n']) ** 2:.0f} s, beyond {args.limit:.0f} s")
        return before
    rows, lens, planted = make_set(n, s, seed=n + s)

    def way_support():
        t0 = time.perf_counter()
        got = engine.dist_nj_support(rows, lens, K, s, R, KEEP, SEED)
        return time.perf_counter() - t0, got

    def way_today():
        t0 = time.perf_counter()
        main = engine.dist_nj(rows, lens, K, s)
        rep_a, rep_b = (np.zeros((R, n - 1), np.uint32) for _ in range(2))
        rep_s = np.zeros(R, np.uint32)
        for r in range(R):
            cut, cut_len, s_r = numpy_replicate(rows, lens, s, SEED, r, KEEP)
            rep_a[r], rep_b[r] = engine.dist_nj(cut, cut_len, K, s_r)[:2]
            rep_s[r] = s_r
        support = engine.nj_split_support(main[0], main[1], rep_a, rep_b, n)
        return time.perf_counter() - t0, main + (support, rep_a, rep_b, rep_s)

    warm_a, a = way_support()
    warm_b, b = way_today()
    same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    sup = a[7]
    say(f"tools/nj_support_rate.py on {engine.device_name()}: n = {n}, s = {s}, k = {K}, R = {R}, keep = {KEEP}, seed = {SEED} ({planted} planted clade links); "
        f"s_r {int(a[10].min())} .. {int(a[10].max())}; support: {int((sup == R).sum())} of {n - 1} joins in every replicate, {int((sup == 0).sum())} in none, "
        f"{int(((sup > 0) & (sup < R)).sum())} in between; main records, every replicate's joins and sizes and the support of the two ways the same bytes: {same}")
    if not same:
        raise SystemExit("the two ways disagree")
    wall = {"a": [warm_a], "b": [warm_b]}
    if max(warm_a, warm_b) < args.long_call:
        wall = {"a": [], "b": []}
        for _ in range(args.rounds):
            wall["a"].append(way_support()[0])
            wall["b"].append(way_today()[0])
        say(f"{args.rounds} interleaved rounds after a warm-up of each way; wall = host clock around calls that are complete when they return")
    else:
        say(f"a way takes more than {args.long_call:.0f} s: the first run of each way is the one timed")

    def row(label, v):
        v = [x * 1e3 for x in v]
        say(f"  {label:52s} median {statistics.median(v):11.3f} ms  best {min(v):11.3f}  worst {max(v):11.3f}   rounds " + " ".join(f"{x:.3f}" for x in v))
        return statistics.median(v)
    ta = row("(a) dist_nj_support (host pointers), wall", wall["a"])
    tb = row("(b) numpy resample + dist_nj, R times, wall", wall["b"])
    say(f"  (a) / (b) = {ta / tb:.3f}; (a) per replicate {ta / (R + 1):.3f} ms, (b) per replicate {tb / (R + 1):.3f} ms (the main tree counted as one)")
    return {"n": n, "t": max(ta, tb) / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shapes", default="24x1000,256x1000,2048x1000")
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--long-call", type=float, default=20.0, help="seconds of one way beyond which no further rounds are run")
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

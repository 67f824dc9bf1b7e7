"""What winner-take-all costs on top of the containment from sketches (mhx_dist_contain_winner), rows resident on the device.
The rows are those of tools/contain_rate.py: queries are synthetic independent sketches, every `every`-th of them a reference
with 3 % of its hashes replaced; a reference set of up to 64 lists is clade-like (four bases, every member a base with 0.2 %
.. 5 % of its hashes replaced), a larger one independent like the queries.  Genome lengths are given, with ties.

    shapes     queries x references x s x every:
               1024 x 24 x 50 000 x 1   the AuriClass shape, every sample related to the references: every pair shares
               1024 x 24 x 50 000 x 8   the same with one sample in eight related (the rows of tools/contain_rate.py)
               64 x 10 000 x 1000 x 1   most pairs share nothing: the skip of the claim pass matters

Three ways on the same rows, alternating within one call, every way of every shape warmed up first:

    (w) winner      mhx_dist_contain_winner: the plain pass, the claim pass and the tally; kernel time of the call
    (p) plain       mhx_dist_contain alone; kernel time of the call.  (w) - (p) is what the winner passes add
    (h) host        mhx_dist_contain, its three outputs copied to the host, and the winner assignment in numpy -- per query the
                    references that share something sorted by the rule, intersect1d and searchsorted per pair in that order, a
                    boolean word per position of the query's list -- which is what a user would write today; wall time, on at
                    most --host-queries queries and scaled to all of them

(w) and (p) run TWICE per round -- w1 p1 w2 p2 -- so that the spread of one build against itself stands next to the
difference between the two.  The `won` of (h) must equal the `won` of (w) on the queries (h) ran.

    python tools/contain_winner_rate.py [--rounds R] [--out FILE] [--shapes 1024x24x50000x1,...] [--host-queries N]
"""
import argparse
import functools
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def host_winner(Q, R, lengths, shared, n_qry, n_ref, queries):
    """won [len(queries), nr] in numpy from the plain outputs: what a user would write on the host"""
    import numpy as np

    nr = R.shape[0]
    won = np.zeros((len(queries), nr), np.uint32)
    for t, qi in enumerate(queries):
        refs = [int(r) for r in np.nonzero(shared[qi])[0]]

        def before(a, b):   # the rule's order: -1 when a ranks before b
            x, y = int(shared[qi, a]) * int(n_ref[qi, b]), int(shared[qi, b]) * int(n_ref[qi, a])
            if x != y:
                return -1 if x > y else 1
            if lengths[a] != lengths[b]:
                return -1 if lengths[a] > lengths[b] else 1
            return -1 if a < b else 1

        refs.sort(key=functools.cmp_to_key(before))
        taken = np.zeros(Q.shape[1], bool)
        for r in refs:
            q = Q[qi, :n_qry[qi, r]]
            at = np.searchsorted(q, np.intersect1d(q, R[r, :n_ref[qi, r]], assume_unique=True))
            won[t, r] = int((~taken[at]).sum())
            taken[at] = True
    return won


def measure(nq, nr, s, every, rounds, host_queries, say):
    import numpy as np
    import torch

    from contain_rate import clade_rows, mutated
    from triangle_rate import make_rows

    from auriclass_amd import engine

    L = engine.load()
    dev = "cuda:0"
    Q, ql = make_rows(nq, s, 7 + nq + s)
    R, rl = clade_rows(nr, s, nr + s) if nr <= 64 else make_rows(nr, s, nr + s)
    rng = np.random.default_rng(nq * 31 + nr)
    for i in range(0, nq, every):
        Q[i, :s] = mutated(rng, R[i % nr, :s], 0.03)
    lengths = (4_000_000 + (np.arange(nr, dtype=np.uint64) * 7) % 5).astype(np.uint64)
    stride = Q.shape[1]
    d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, ql, R, rl, lengths)]
    out = {w: [torch.zeros((nq, nr), dtype=torch.int32, device=dev) for _ in range(4)] for w in ("w", "p")}
    torch.cuda.synchronize()

    def winner():
        o = out["w"]
        ms = engine.dist_contain_winner_device(d[0].data_ptr(), d[1].data_ptr(), nq, s, d[2].data_ptr(), d[3].data_ptr(), nr, s, stride, d[4].data_ptr(),
                                               o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr())
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks(), L.mhx_last_contain_winner_pairs()

    def plain():
        o = out["p"]
        ms = engine.dist_contain_device(d[0].data_ptr(), d[1].data_ptr(), nq, s, d[2].data_ptr(), d[3].data_ptr(), nr, s, stride, o[1].data_ptr(),
                                        o[2].data_ptr(), o[3].data_ptr())
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks(), 0

    queries = list(range(0, nq, max(1, nq // host_queries)))[:host_queries]

    def host():
        t0 = time.perf_counter()
        plain()
        shared, n_qry, n_ref = (o.cpu().numpy().view(np.uint32) for o in out["p"][1:])
        won = host_winner(Q, R, lengths, shared, n_qry, n_ref, queries)
        return (time.perf_counter() - t0) * 1e3, won

    order = ("w1", "p1", "w2", "p2")
    calls = {"w1": winner, "p1": plain, "w2": winner, "p2": plain}
    info = {w: calls[w]()[1:] for w in order}   # warm-up: code objects, the workspace, the outputs' pages
    same_plain = all(bool(torch.equal(x, y)) for x, y in zip(out["w"][1:], out["p"][1:]))
    times = {w: [] for w in order}
    for _ in range(rounds):
        for w in order:
            times[w].append(calls[w]()[0])
    host_ms, host_won = host()
    t0 = time.perf_counter()
    plain()
    plain_wall = (time.perf_counter() - t0) * 1e3
    host_all = plain_wall + (host_ms - plain_wall) * nq / len(queries)
    got = out["w"][0].cpu().numpy().view(np.uint32)
    same_won = bool(np.array_equal(got[queries], host_won))
    med = {w: statistics.median(v) for w, v in times.items()}
    say(f"{nq} queries x {nr} references, s = {s}, every {every}. query related: {nq * nr} pairs, {info['w1'][2]} of them share something and are walked; "
        f"{int(got.sum())} hashes won in all; shared / n_qry / n_ref of (w) equal (p)'s: {same_plain}; won of (h) equals (w)'s on {len(queries)} queries: {same_won}")
    labels = {"w1": "(w) winner, first", "w2": "(w) winner, second", "p1": "(p) plain, first", "p2": "(p) plain, second"}
    for w in order:
        v = times[w]
        say(f"  {labels[w]:24s} R = {info[w][0]:5d}  fallback blocks {info[w][1]:3d}  ms: median {med[w]:9.4f}  best {min(v):9.4f}  worst {max(v):9.4f}   rounds "
            + " ".join(f"{x:.4f}" for x in v))
    w, p = (med["w1"] + med["w2"]) / 2, (med["p1"] + med["p2"]) / 2
    say(f"  (h) plain call, D2H and numpy winner assignment: {host_ms:.1f} ms wall for {len(queries)} queries, {host_all:.1f} ms scaled to {nq} (the plain call "
        f"alone: {plain_wall:.3f} ms wall)")
    say(f"  (w) {w:.4f} ms, (p) {p:.4f} ms: the winner passes add {w - p:.4f} ms; self-spread (w) {abs(med['w1'] - med['w2']):.4f}, (p) "
        f"{abs(med['p1'] - med['p2']):.4f};  (w) / (p) = {w / p:.2f}   (h) / (w) = {host_all / w:.0f}")
    if not (same_plain and same_won):
        raise SystemExit("the ways disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x24x50000x1,1024x24x50000x8,64x10000x1000x1")
    ap.add_argument("--host-queries", type=int, default=32)
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

    say(f"tools/contain_winner_rate.py on {engine.device_name()}: {args.rounds} rounds of w1 p1 w2 p2 after a warm-up of each; kernel time of the call "
        "(mhx_last_dist_kernel_ms); (h) wall time")
    for shape in args.shapes.split(","):
        nq, nr, s, every = (int(x) for x in shape.split("x"))
        measure(nq, nr, s, every, args.rounds, args.host_queries, say)


if __name__ == "__main__":
    main()

"""What the unbounded containment call costs (mhx_dist_contain_within) next to its two yardsticks, rows resident on the device,
k = 21.  Data: independent synthetic sketches as tools/contain_search_rate.py makes them, plus a crowd -- `crowd` references
(default 150, spread evenly over the set) are copies of one base list with 0 .. 30 % of their hashes replaced, and EVERY query
is that base list with 2 % replaced, so every query holds about `crowd` references at the bound of the run.

    shapes     queries x references x s_q x s_r: 1024 x 100 000 at 1000 both, 1024 x 24 at 50 000 both (the crowd is the
               whole set there)

Four ways on the same rows, interleaved round by round, device pointers in and out, all at the same bound (min_identity 0.9,
min_shared 1) unless said otherwise:

    (a) all        mhx_dist_contain_within with room for every hit: row_off and the four hit arrays, exact and in final order
    (b) all, new bound   the same call at a min_identity that differs from call to call (0.9 + i * 1e-9), so that the host
                   builds the need table anew every time: what a first call, or a call with another bound, costs
    (c) counting   the counting form of (a): row_off alone, no arrival list, no atomic
    (s) yardstick 1  mhx_dist_contain_search at top = 64 with the same bound: the same schedule and a smaller answer
    (y) yardstick 2  mhx_dist_contain into the three full [nq][nr] matrices, then the need-table test and `nonzero` in torch on
                   the device, and the three gathers of the hits

Time, ONE base for all: the whole route as its caller sees it -- torch device events recorded before the first call and after
the last one has returned (every engine call waits for its own work), and the wall clock around the same span with a device
synchronise at its end; the engine's kernel time (mhx_last_dist_kernel_ms) is printed next to it, apart.  After one warm-up
of each way every way is timed --rounds times (default 5); median, best and worst are printed: the spread between runs.  The
CSR of (a) must equal that of (y) entry for entry, and its rows cut to 64 by rank must hold the references of (s).

Bytes: what each route returns, what torch allocates at its peak over (y) (torch.cuda.max_memory_allocated, its outputs
included), and what the first call of each route takes from the driver beyond that (free device memory before and after: the
engine's workspace, which only grows -- (a) runs first).

    python tools/contain_within_rate.py [--rounds R] [--crowd N] [--out FILE] [--shapes 1024x100000x1000x1000,...]

No ratio is asked of this tool.  It prints whether (a) is slower than (s) by more than the spread of (s).
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
MIN_IDENTITY = 0.9


def make_sets(nq, nr, s_q, s_r, crowd):
    import numpy as np

    from contain_rate import mutated
    from triangle_rate import make_rows

    Q, ql = make_rows(nq, s_q, 7 + nq + s_q)
    R, rl = make_rows(nr, s_r, nr + s_r)
    rng = np.random.default_rng(nq * 31 + nr)
    s = min(s_q, s_r)
    base = R[0, :s].copy()
    members = np.unique(np.linspace(0, nr - 1, min(crowd, nr)).astype(np.int64))
    for j, i in enumerate(members):
        m = mutated(rng, base, 0.3 * j / max(1, len(members) - 1))
        R[i, :] = 0
        R[i, :len(m)] = m
        rl[i] = len(m)
    for i in range(nq):
        m = mutated(rng, base, 0.02)
        Q[i, :] = 0
        Q[i, :len(m)] = m
        ql[i] = len(m)
    if R.shape[1] != Q.shape[1]:   # one stride for both sets
        width = max(R.shape[1], Q.shape[1])
        wide = lambda M: np.concatenate([M, np.zeros((M.shape[0], width - M.shape[1]), np.uint64)], axis=1)
        Q, R = wide(Q), wide(R)
    return Q, ql, R, rl


def measure(nq, nr, s_q, s_r, crowd, rounds, say):
    import numpy as np
    import torch

    from auriclass_amd import engine
    from tests import contain_search_rule as search_rule

    L = engine.load()
    dev = "cuda:0"
    Q, ql, R, rl = make_sets(nq, nr, s_q, s_r, crowd)
    stride = Q.shape[1]
    d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, ql, R, rl)]
    p = [t.data_ptr() for t in d]
    limit = min(stride, s_r)
    # the need table of the yardstick, built once outside the timing by the engine's own rule through the counting form's host
    # side is not reachable from here: the definition over the monotone identity, by bisection per n (tests tie it to is_hit)
    need_host = np.empty(limit + 1, np.int64)
    for n in range(limit + 1):
        lo, hi = 1, n + 1
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if search_rule.is_hit(mid, n, K, MIN_IDENTITY, 1) else (mid + 1, hi)
        need_host[n] = lo
    need = torch.from_numpy(need_host).to(dev)
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info()[0]
    n_total = engine.dist_contain_within_device(p[0], p[1], nq, s_q, p[2], p[3], nr, s_r, stride, K, MIN_IDENTITY, 1,
                                                torch.zeros(nq + 1, dtype=torch.int64, device=dev).data_ptr(), 0, 0, 0, 0, 0)
    cap = n_total + 1024   # (b) moves the bound by 1e-9 per call: room to spare
    row_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    hit = [torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(4)]
    top = [torch.zeros((nq, 64), dtype=torch.int32, device=dev) for _ in range(4)]
    n_top = torch.zeros(nq, dtype=torch.int32, device=dev)
    ways = ("all", "all-i", "count", "search", "table")
    kernel_ms = {w: [] for w in ways}
    wall_ms = {w: [] for w in ways}

    def whole(way, route):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        route()
        kernel_ms[way].append(L.mhx_last_dist_kernel_ms())
        t1.record()
        torch.cuda.synchronize()
        wall_ms[way].append((time.perf_counter() - w0) * 1e3)
        return t0.elapsed_time(t1), L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    def within(min_identity, store=True):
        o = [row_off.data_ptr()] + ([h.data_ptr() for h in hit] + [cap] if store else [0, 0, 0, 0, 0])
        return engine.dist_contain_within_device(p[0], p[1], nq, s_q, p[2], p[3], nr, s_r, stride, K, min_identity, 1, *o)

    bound = {"i": 0}

    def new_bound():
        bound["i"] += 1
        return within(MIN_IDENTITY + 1e-9 * bound["i"])

    yard = {}

    def table():
        full = [torch.empty((nq, nr), dtype=torch.int32, device=dev) for _ in range(3)]
        engine.dist_contain_device(p[0], p[1], nq, s_q, p[2], p[3], nr, s_r, stride, full[0].data_ptr(), full[1].data_ptr(), full[2].data_ptr())
        shared, n_qry, n_ref = full
        qi, ri = torch.nonzero(shared.to(torch.int64) >= need[n_ref.to(torch.int64)], as_tuple=True)
        yard["row_off"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(qi, minlength=nq), 0)])
        yard["hits"] = [ri.to(torch.int32), shared[qi, ri], n_ref[qi, ri], n_qry[qi, ri]]

    routes = {"all": lambda: within(MIN_IDENTITY), "all-i": new_bound, "count": lambda: within(MIN_IDENTITY, False),
              "search": lambda: engine.dist_contain_search_device(p[0], p[1], nq, s_q, p[2], p[3], nr, s_r, stride, K, 64, MIN_IDENTITY, 1,
                                                                  *[t.data_ptr() for t in top], n_top.data_ptr()),
              "table": table}
    info, taken = {}, {}
    for w in ("all", "search"):
        before = free()
        info[w] = whole(w, routes[w])[1:]
        taken[w] = before - free()
    torch.cuda.reset_peak_memory_stats()
    base, before = torch.cuda.memory_allocated(), free()
    info["table"] = whole("table", table)[1:]
    peak = torch.cuda.max_memory_allocated() - base
    taken["table"] = before - free()
    same = bool(torch.equal(row_off, yard["row_off"]) and all(torch.equal(a[:n_total], b) for a, b in zip(hit, yard["hits"])))
    per = (row_off[1:] - row_off[:-1])
    in_top = bool(torch.equal(n_top.to(torch.int64), per.clamp(max=64)))
    info["all-i"] = whole("all-i", new_bound)[1:]
    info["count"] = whole("count", routes["count"])[1:]
    for v in list(kernel_ms.values()) + list(wall_ms.values()):   # the warm-ups are not rounds
        v.clear()
    times = {w: [] for w in ways}
    for _ in range(rounds):
        for w in ways:
            times[w].append(whole(w, routes[w])[0])
    say(f"{nq} queries x {nr} references, s_q = {s_q}, s_r = {s_r}, k = {K}, min_identity = {MIN_IDENTITY}, min_shared = 1: {nq * nr} pairs, {n_total} hits "
        f"({float(per.float().mean()):.1f} per query, at most {int(per.max())}); the CSR of (a) equals the yardstick's: {same}; the search's list lengths are its rows cut to 64: {in_top}")
    med = {w: statistics.median(v) for w, v in times.items()}
    labels = (("all", "(a) mhx_dist_contain_within"), ("all-i", "(b) the same, need table built per call"), ("count", "(c) the counting form"),
              ("search", "(s) mhx_dist_contain_search, top = 64"), ("table", "(y) mhx_dist_contain + torch nonzero"))
    for w, label in labels:
        v = times[w]
        say(f"  {label:42s} R = {info[w][0]:5d}  fallback blocks {info[w][1]}  whole route, event ms: median {med[w]:10.3f}  best {min(v):10.3f}  worst {max(v):10.3f}  "
            f"spread {max(v) - min(v):.3f}  wall ms: median {statistics.median(wall_ms[w]):.3f}  kernel ms (mhx_last_dist_kernel_ms, the engine call alone) median "
            f"{statistics.median(kernel_ms[w]):.3f}   rounds " + " ".join(f"{x:.3f}" for x in v))
    spread_s = max(times["search"]) - min(times["search"])
    more = med["all"] - med["search"]
    say(f"  (a) - (s), medians: {more:+.3f} ms; the spread of (s) is {spread_s:.3f} ms: (a) is {'SLOWER than (s) by more than its spread' if more > spread_s else 'within the spread of (s), or faster'}"
        f"   (a) / (y) = {med['all'] / med['table']:.3f}   (b) - (a) = {med['all-i'] - med['all']:+.3f} ms   (c) - (a) = {med['count'] - med['all']:+.3f} ms")
    say(f"  bytes returned: (a) {(nq + 1) * 8 + 4 * n_total * 4}, (c) {(nq + 1) * 8}, (s) {4 * nq * 64 * 4 + nq * 4}, (y) the three matrices {3 * nq * nr * 4} before the filter; "
        f"taken from the driver by the first call: (a) {taken['all']}, (s) {taken['search']}, (y) {taken['table']}; torch's peak over (y), matrices included: {peak}")
    if not same or not in_top:
        raise SystemExit("the routes disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--crowd", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x100000x1000x1000,1024x24x50000x50000")
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

    say(f"tools/contain_within_rate.py on {engine.device_name()}: {args.rounds} interleaved rounds after a warm-up of each way; every way timed as a "
        "whole route on one base (device events and the wall clock around everything its caller waits for); the engine's kernel ms apart")
    for shape in args.shapes.split(","):
        nq, nr, s_q, s_r = (int(x) for x in shape.split("x"))
        measure(nq, nr, s_q, s_r, args.crowd, args.rounds, say)


if __name__ == "__main__":
    main()

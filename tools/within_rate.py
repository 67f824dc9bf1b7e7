"""What the bounded neighbourhood call costs (mhx_dist_within: all references within a distance of each query, as CSR) next
to the two routes there were before it, rows resident on the device, k = 21, max_dist = 0.05.

    shapes     queries x references x s: 1024 x 24 at s = 50 000 (four clades of six references, every query a 1 % mutation
               of a reference: six hits each), and 1024 x 100 000 at s = 1000 with a clade-structured reference set -- 600
               clades of 150 near-identical isolates (0.2 % .. 2 % of the hashes replaced), 10 000 independent lists -- every
               query a 1 % mutation of a clade's base: about 150 hits each, more than a search list holds

Three ways on the same rows, interleaved round by round, device pointers in and out:

    (w) within     mhx_dist_within with room for every hit: the CSR, exact and in its final order; the cmin table of the bound
                   is the engine's from the call before (an untimed call at the same bound precedes every timed one)
    (n) within, new bound   the same call at a bound that differs from call to call (0.05 + i * 1e-9), so that the host builds
                   and copies the cmin table anew every time: what a first call, or a call with another bound, costs
    (a) search     mhx_dist_search at top = 64: the same schedule (one split of both sets, the same blocks), so the difference
                   to (w) is the price of the take-out into cells, the scan, the gather and the table; it keeps at most 64
                   hits per query and is prefiltered only
    (b) matrix     mhx_dist_batch into the full [nq][nr] matrices (common, denom, dist), then `dist <= max_dist` and
                   nonzero() with torch on the device: the same pairs as (w) in the same order, through a cell per pair

Time, ONE base for all: the whole route as its caller sees it -- torch device events recorded before the first call and after
the last one has returned (every engine call waits for its own work), and the wall clock around the same span with a device
synchronise at its end; the engine's kernel time (mhx_last_dist_kernel_ms) is printed next to it, apart.  After one warm-up
of each way every way is timed --rounds times (default 7); median, best and worst are printed, and the spread (worst - best)
of (a) is the unit in which the cost of (w) over (a) is stated.  The pairs of (w) must equal those of (b) entry for entry.

Bytes: what each route's outputs hold and what torch allocates at its peak over (b), its matrices included.

    python tools/within_rate.py [--rounds R] [--out FILE] [--shapes 1024x24x50000,1024x100000x1000]

No ratio is asked of this tool.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
K = 21
D = 0.05


def make_rows(torch, n, s, gen, dev):
    """n ascending lists of s hashes below 2^62 (duplicates within a list: one chance in 10^13 per list)"""
    out = torch.empty((n, s), dtype=torch.int64, device=dev)
    for i0 in range(0, n, 8192):
        i1 = min(n, i0 + 8192)
        out[i0:i1] = torch.sort(torch.randint(0, 2 ** 62, (i1 - i0, s), dtype=torch.int64, device=dev, generator=gen), dim=1).values
    return out


def mutate(torch, rows, share, gen, dev):
    """every list with a share (a number, or one per list) of its hashes replaced by fresh ones"""
    out = torch.empty_like(rows)
    for i0 in range(0, rows.shape[0], 8192):
        part = rows[i0:i0 + 8192]
        fresh = torch.randint(0, 2 ** 62, part.shape, dtype=torch.int64, device=dev, generator=gen)
        sh = share[i0:i0 + 8192, None] if torch.is_tensor(share) else share
        out[i0:i0 + 8192] = torch.sort(torch.where(torch.rand(part.shape, device=dev, generator=gen) < sh, fresh, part), dim=1).values
    return out


def make_sets(torch, nq, nr, s, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(nq * 31 + nr + s)
    members = 150 if nr >= 1500 else 6
    nclades = max(1, (nr - nr // 10) // members) if nr >= 1500 else nr // members
    bases = make_rows(torch, nclades, s, gen, dev)
    in_clades = nclades * members
    share = 0.002 + 0.018 * torch.rand(in_clades, device=dev, generator=gen)
    R = torch.cat([mutate(torch, bases.repeat_interleave(members, dim=0), share, gen, dev), make_rows(torch, nr - in_clades, s, gen, dev)])
    R = R[torch.randperm(nr, device=dev, generator=gen)]   # the members of a clade lie all over the set
    Q = mutate(torch, bases[torch.arange(nq, device=dev) % nclades], 0.01, gen, dev)
    stride = (s + 15) // 16 * 16
    pad = lambda rows: torch.cat([rows, torch.zeros((rows.shape[0], stride - s), dtype=torch.int64, device=dev)], dim=1).contiguous()
    return pad(Q), torch.full((nq,), s, dtype=torch.int32, device=dev), pad(R), torch.full((nr,), s, dtype=torch.int32, device=dev), stride


def measure(nq, nr, s, rounds, say):
    import torch

    from auriclass_amd import engine

    L = engine.load()
    dev = "cuda:0"
    Q, ql, R, rl, stride = make_sets(torch, nq, nr, s, dev)
    torch.cuda.synchronize()
    top = 64
    row_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    total = engine.dist_within_device(Q.data_ptr(), ql.data_ptr(), nq, R.data_ptr(), rl.data_ptr(), nr, stride, K, s, D, row_off.data_ptr(), 0, 0, 0, 0, 0)
    per_query = (row_off[1:] - row_off[:-1])
    cap = max(total, 1)
    hit = [torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(3)]
    lists = [torch.zeros((nq, top), dtype=torch.int32, device=dev) for _ in range(3)]
    n_hits = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kernel_ms = {"within": [], "within-n": [], "search": []}
    wall_ms = {"within": [], "within-n": [], "search": [], "matrix": []}

    def whole(way, route):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        rest = route()
        t1.record()
        torch.cuda.synchronize()
        wall_ms[way].append((time.perf_counter() - w0) * 1e3)
        return (t0.elapsed_time(t1),) + rest

    def call_within(bound):
        return engine.dist_within_device(Q.data_ptr(), ql.data_ptr(), nq, R.data_ptr(), rl.data_ptr(), nr, stride, K, s, bound, row_off.data_ptr(),
                                         hit[0].data_ptr(), hit[1].data_ptr(), hit[2].data_ptr(), 0, cap)

    def within(bound=D, way="within"):
        if way == "within":   # the engine keeps the table of the last bound only, and (n) has run since: bring it back outside the timing
            call_within(bound)

        def route():
            n = call_within(bound)
            kernel_ms[way].append(L.mhx_last_dist_kernel_ms())
            return L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks(), n
        return whole(way, route)

    turn = {"i": 0}

    def within_new_bound():
        turn["i"] += 1
        return within(D + 1e-9 * turn["i"], "within-n")

    def search():
        def route():
            kernel_ms["search"].append(engine.dist_search_device(Q.data_ptr(), ql.data_ptr(), nq, R.data_ptr(), rl.data_ptr(), nr, stride, K, s, top, D,
                                                                 lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), 0, n_hits.data_ptr()))
            return L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks(), 0
        return whole("search", route)

    yard = {}

    def matrix():
        def route():
            common = torch.empty((nq, nr), dtype=torch.int32, device=dev)
            denom = torch.empty((nq, nr), dtype=torch.int32, device=dev)
            dist = torch.empty((nq, nr), dtype=torch.float64, device=dev)
            engine.dist_batch_device(Q.data_ptr(), ql.data_ptr(), nq, R.data_ptr(), rl.data_ptr(), nr, stride, K, s, common.data_ptr(), denom.data_ptr(),
                                     dist.data_ptr())
            ranges, fallbacks = L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()
            at = (dist <= D).nonzero()
            yard["q"], yard["r"] = at[:, 0], at[:, 1]
            yard["common"], yard["denom"] = common[at[:, 0], at[:, 1]], denom[at[:, 0], at[:, 1]]
            return ranges, fallbacks, int(at.shape[0])
        return whole("matrix", route)

    def agrees():
        # (the device's log against the host's at a pair exactly on the bound could differ; D = 0.05 is no pair's distance here)
        n = int(row_off[nq])
        counts = torch.bincount(yard["q"], minlength=nq)
        return bool(n == yard["q"].shape[0] and torch.equal(counts, per_query) and torch.equal(hit[0][:n].to(torch.int64), yard["r"]) and
                    torch.equal(hit[1][:n], yard["common"]) and torch.equal(hit[2][:n], yard["denom"]))

    info = {}
    info["within"] = within()[1:]
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    info["matrix"] = matrix()[1:]
    peak = torch.cuda.max_memory_allocated() - base
    same = agrees()
    info["within-n"] = within_new_bound()[1:]
    info["search"] = search()[1:]
    ways = {"within": within, "within-n": within_new_bound, "search": search, "matrix": matrix}
    for v in list(kernel_ms.values()) + list(wall_ms.values()):   # the warm-ups are not rounds
        v.clear()
    times = {w: [] for w in ways}
    for _ in range(rounds):
        for w, call in ways.items():
            times[w].append(call()[0])
    say(f"{nq} queries x {nr} references, s = {s}, k = {K}, max_dist = {D}: {nq * nr} pairs, {total} hits, per query min {int(per_query.min())} "
        f"median {int(per_query.median())} max {int(per_query.max())}, {int((per_query > top).sum())} queries beyond {top}; the pairs of (w) equal those of (b): {same}")
    med = {w: statistics.median(v) for w, v in times.items()}
    for w, label in (("within", "(w) mhx_dist_within"), ("within-n", "(n) the same, cmin table built per call"), ("search", "(a) mhx_dist_search, top = 64"),
                     ("matrix", "(b) mhx_dist_batch + torch threshold, nonzero")):
        v = times[w]
        kernel = f"  of it kernel ms (mhx_last_dist_kernel_ms) median {statistics.median(kernel_ms[w]):.3f}" if w in kernel_ms else ""
        say(f"  {label:46s} R = {info[w][0]:5d}  fallback blocks {info[w][1]}  whole route, event ms: median {med[w]:10.3f}  best {min(v):10.3f}  worst {max(v):10.3f}  "
            f"spread {max(v) - min(v):.3f}  wall ms: median {statistics.median(wall_ms[w]):.3f}{kernel}   {nq * nr / med[w] / 1e3:9.1f} M pairs/s   rounds "
            + " ".join(f"{x:.3f}" for x in v))
    spread = max(times["search"]) - min(times["search"])
    say(f"  (w) over (a): {med['within'] - med['search']:+.3f} ms = {(med['within'] - med['search']) / spread if spread > 0 else float('inf'):+.1f} spreads of (a) "
        f"({spread:.3f} ms); (n) over (a): {med['within-n'] - med['search']:+.3f} ms; (w) / (a) = {med['within'] / med['search']:.3f}; (w) / (b) = {med['within'] / med['matrix']:.3f}")
    say(f"  bytes: (w) outputs {(nq + 1) * 8 + 3 * total * 4} (row_off and three words per hit); (a) outputs {3 * nq * top * 4 + nq * 4}; (b) the three matrices "
        f"{nq * nr * 16}, torch's peak over the route (matrices included) {peak}")
    if not same:
        raise SystemExit("mhx_dist_within and the matrix route disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x24x50000,1024x100000x1000")
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

    say(f"tools/within_rate.py on {engine.device_name()}: {args.rounds} interleaved rounds after a warm-up of each way; every way timed as a whole route "
        "on one base (device events and the wall clock around everything its caller waits for); the engine's kernel ms apart")
    for shape in args.shapes.split(","):
        nq, nr, s = (int(x) for x in shape.split("x"))
        measure(nq, nr, s, args.rounds, say)


if __name__ == "__main__":
    main()

"""What the containment search costs (mhx_dist_contain_search) next to the route there was before it, rows resident on the
device, k = 21.  Data as tools/contain_rate.py makes it: queries are synthetic INDEPENDENT sketches, every eighth of them
holds a reference with 3 % of its hashes replaced (at s_q == s_r it IS that list; at s_q > s_r the reference's hashes lie
among the query's own); a reference set of up to 64 lists is clade-like, a larger one independent.

    shapes     queries x references x s_q x s_r: 1024 x 24 at 50 000 both, 1024 x 24 at 50 000 against 1000,
               1024 x 100 000 at 1000 both

Three ways on the same rows, interleaved round by round, device pointers in and out:

    (a) ranked     mhx_dist_contain_search at min_identity = 0: [nq][top] lists, ranked on the device block by block.  The
                   need table takes no pow at this bound, and the engine keeps the table of the last call anyway.
    (b) ranked, new bound   the same call at a min_identity between 0 and 1 that differs from call to call (0.5 + i * 1e-6: at
                   k = 21 every pair that shares a hash still passes), so that the host builds the need table anew every
                   time: what a first call, or a call with another bound, costs
    (y) yardstick  mhx_dist_contain into the three full [nq][nr] matrices, then the ranking with torch on the device: the hit
                   test through a need[] table built once outside the timing, a stable sort by `shared` and a stable sort by
                   the share (a double: exact below n_ref = 2^26), the first `top` of every row

Time, ONE base for all three: the whole route as its caller sees it -- torch device events recorded before the first call and
after the last one has returned (every engine call waits for its own work), and the wall clock around the same span with a
device synchronise at its end.  For (a) and (b) that holds the host's build of the need table and its blocking copy, which
lie before the engine's own first event; the engine's kernel time (mhx_last_dist_kernel_ms) is printed next to it, apart.
After one warm-up of each way every way is timed --rounds times (default 5); median, best and worst are printed: the spread
between runs.  The lists of (a) must equal those of (y) entry for entry.

Bytes: what each route's outputs hold, what torch allocates at its peak for the ranking (torch.cuda.max_memory_allocated over
the yardstick, its outputs included), and what the first call of each route takes from the driver beyond that (free device
memory before and after: the engine's workspace, which only grows -- (a) runs first).

    python tools/contain_search_rate.py [--rounds R] [--top T] [--out FILE] [--shapes 1024x24x50000x50000,...]

No ratio is asked of this tool: the case for the ranked route is memory and output size.  Where it is slower, the figures say
so: (b) at a long reference sketch is such a place.
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


def make_sets(nq, nr, s_q, s_r):
    import numpy as np

    from contain_rate import clade_rows, mutated
    from triangle_rate import make_rows

    Q, ql = make_rows(nq, s_q, 7 + nq + s_q)
    R, rl = clade_rows(nr, s_r, nr + s_r) if nr <= 64 else make_rows(nr, s_r, nr + s_r)
    rng = np.random.default_rng(nq * 31 + nr)
    for i in range(0, nq, 8):
        m = mutated(rng, R[i % nr, :s_r], 0.03)
        Q[i, :s_q] = m if s_q == s_r else np.unique(np.concatenate([m, Q[i, :s_q]]))[:s_q]
    if R.shape[1] < Q.shape[1]:   # one stride for both sets
        wide = np.zeros((nr, Q.shape[1]), np.uint64)
        wide[:, :R.shape[1]] = R
        R = wide
    return Q, ql, R, rl


def measure(nq, nr, s_q, s_r, top, rounds, say):
    import numpy as np
    import torch

    from auriclass_amd import engine

    L = engine.load()
    dev = "cuda:0"
    Q, ql, R, rl = make_sets(nq, nr, s_q, s_r)
    stride = Q.shape[1]
    d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, ql, R, rl)]
    need = torch.ones(min(stride, s_r) + 1, dtype=torch.int64, device=dev)   # min_identity 0, min_shared 1: one shared hash is a hit at every n_ref
    hit = [torch.zeros((nq, top), dtype=torch.int32, device=dev) for _ in range(4)]
    n_hits = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info()[0]

    kernel_ms = {"ranked": [], "ranked-i": []}
    wall_ms = {"ranked": [], "ranked-i": [], "yardstick": []}

    def whole(way, route):
        """(event ms, ...) of route() on the base all ways share; the wall clock goes to wall_ms[way]"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        rest = route()
        t1.record()
        torch.cuda.synchronize()
        wall_ms[way].append((time.perf_counter() - w0) * 1e3)
        return (t0.elapsed_time(t1),) + rest

    def ranked(min_identity=0.0, way="ranked"):
        def route():
            kernel_ms[way].append(engine.dist_contain_search_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, stride,
                                                                    K, top, min_identity, 1, hit[0].data_ptr(), hit[1].data_ptr(), hit[2].data_ptr(),
                                                                    hit[3].data_ptr(), n_hits.data_ptr()))
            return L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()
        return whole(way, route)

    bound = {"i": 0}

    def ranked_new_bound():
        bound["i"] += 1
        return ranked(0.5 + 1e-6 * bound["i"], "ranked-i")

    yard = {}

    def yardstick():
        def route():
            full = [torch.empty((nq, nr), dtype=torch.int32, device=dev) for _ in range(3)]
            engine.dist_contain_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, stride, full[0].data_ptr(),
                                       full[1].data_ptr(), full[2].data_ptr())
            ranges, fallbacks = L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()
            shared, n_qry, n_ref = full
            is_hit = shared.to(torch.int64) >= need[n_ref.to(torch.int64)]
            by_shared = torch.sort(torch.where(is_hit, shared, -1), dim=1, descending=True, stable=True).indices
            share = torch.where(is_hit, shared.to(torch.float64) / n_ref.clamp(min=1).to(torch.float64), -1.0)
            by_share = torch.sort(torch.gather(share, 1, by_shared), dim=1, descending=True, stable=True).indices[:, :top]
            best = torch.gather(by_shared, 1, by_share)
            yard["n"] = is_hit.sum(dim=1).clamp(max=top)
            yard["lists"] = [best] + [torch.gather(a, 1, best) for a in (shared, n_ref, n_qry)]
            return ranges, fallbacks
        return whole("yardstick", route)

    def agrees():
        n = n_hits.to(torch.int64)
        live = torch.arange(top, device=dev)[None, :] < n[:, None]
        width = yard["lists"][0].shape[1]
        return bool(torch.equal(n, yard["n"].to(torch.int64)) and
                    all(torch.equal(a[:, :width][live[:, :width]].to(torch.int64), b[live[:, :width]].to(torch.int64)) for a, b in zip(hit, yard["lists"])))

    info, taken = {}, {}
    before = free()
    info["ranked"] = ranked()[1:]   # warm-up of (a): its workspace grows now
    taken["ranked"] = before - free()
    torch.cuda.reset_peak_memory_stats()
    base, before = torch.cuda.memory_allocated(), free()
    info["yardstick"] = yardstick()[1:]
    peak = torch.cuda.max_memory_allocated() - base
    taken["yardstick"] = before - free()
    same = agrees()
    hits = int(n_hits.sum())
    info["ranked-i"] = ranked_new_bound()[1:]
    ways = {"ranked": ranked, "ranked-i": ranked_new_bound, "yardstick": yardstick}
    for v in list(kernel_ms.values()) + list(wall_ms.values()):   # the warm-ups are not rounds
        v.clear()
    times = {w: [] for w in ways}
    for _ in range(rounds):
        for w, call in ways.items():
            times[w].append(call()[0])
    say(f"{nq} queries x {nr} references, s_q = {s_q}, s_r = {s_r}, k = {K}, top = {top}, min_shared = 1: {nq * nr} pairs, "
        f"{hits} hits in the lists at min_identity = 0; the lists of (a) equal the yardstick's: {same}")
    med = {w: statistics.median(v) for w, v in times.items()}
    for w, label in (("ranked", "(a) mhx_dist_contain_search"), ("ranked-i", "(b) the same, need table built per call"), ("yardstick", "(y) mhx_dist_contain + torch ranking")):
        v = times[w]
        kernel = f"  of it kernel ms (mhx_last_dist_kernel_ms) median {statistics.median(kernel_ms[w]):.3f}" if w in kernel_ms else ""
        say(f"  {label:40s} R = {info[w][0]:5d}  fallback blocks {info[w][1]}  whole route, event ms: median {med[w]:10.3f}  best {min(v):10.3f}  worst {max(v):10.3f}  "
            f"wall ms: median {statistics.median(wall_ms[w]):.3f}{kernel}   {nq * nr / med[w] / 1e3:9.1f} M pairs/s   rounds " + " ".join(f"{x:.3f}" for x in v))
    say(f"  whole route, medians of the event ms: (a) / (y) = {med['ranked'] / med['yardstick']:.3f}   (b) / (y) = {med['ranked-i'] / med['yardstick']:.3f}")
    say(f"  bytes: (a) outputs {4 * nq * top * 4 + nq * 4}, taken from the driver by its first call {taken['ranked']}; (y) the three matrices {3 * nq * nr * 4}, "
        f"torch's peak over the route (matrices included) {peak}, taken from the driver by its first call {taken['yardstick']}")
    if not same:
        raise SystemExit("the ranked route and the yardstick disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x24x50000x50000,1024x24x50000x1000,1024x100000x1000x1000")
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

    say(f"tools/contain_search_rate.py on {engine.device_name()}: {args.rounds} interleaved rounds after a warm-up of each way; every way timed as a "
        "whole route on one base (device events and the wall clock around everything its caller waits for); the engine's kernel ms of (a) and (b) apart")
    for shape in args.shapes.split(","):
        nq, nr, s_q, s_r = (int(x) for x in shape.split("x"))
        measure(nq, nr, s_q, s_r, args.top, args.rounds, say)


if __name__ == "__main__":
    main()

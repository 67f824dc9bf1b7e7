"""What the reference-set search costs (mhx_dist_search), on synthetic INDEPENDENT sketches (the generator of
tools/triangle_rate.py: every list holds s values uniform below its own maximum), rows resident on the device, k = 21.

    shapes     queries x references x s: 1024 x 24 and 1 x 100 000 and 1024 x 100 000 at s = 1000, 64 x 4096 at s = 10 000

Three ways on the same rows, interleaved round by round, device pointers in and out:

    (a) search     mhx_dist_search with the triangle's geometry (the smallest power of two R with s <= 16 R)
    (b) dist-geo   mhx_dist_search with MHX_SEARCH_GEOMETRY=dist (1024 x dist_windows(s) ranges)
    (d) yardstick  unchanged code: mhx_dist_batch in device form, in query chunks that respect its 2^31 - 1 pair limit, then
                   torch.topk over the distances on the device
    ((c), splitting the queries once per slice instead of once per call, has no switch: it was not built)

Time: (a), (b) the kernel time of the call (mhx_last_dist_kernel_ms: device events around everything it launches, flag
read-backs included); (d) device events around all calls of the yardstick and the topk.  After one warm-up of each way,
every way is timed --rounds times (default 5); median, best and worst are printed.  The hits of (a) and (b) must equal
those of (d) after the same filter: per query the number of hits and their distances, best first (both are the device's
log of the same counts; which of several references at one distance is named is the rule's business, not the yardstick's).

    python tools/search_rate.py [--rounds R] [--top T] [--max-dist D] [--out FILE] [--shapes 1024x24x1000,...]
"""
import argparse
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
K = 21
PAIR_LIMIT = 2 ** 31 - 1

_rows = {}


def device_rows(n, s, seed):
    """[n][stride] rows on the device, kept: the two 100 000-reference shapes share theirs"""
    import numpy as np
    import torch

    from triangle_rate import make_rows

    if (n, s, seed) not in _rows:
        rows, lens = make_rows(n, s, seed)
        _rows[(n, s, seed)] = (torch.from_numpy(rows.view(np.int64)).to("cuda:0"), torch.from_numpy(lens.view(np.int32)).to("cuda:0"), rows.shape[1])
    return _rows[(n, s, seed)]


def measure(nq, nr, s, top, max_dist, rounds, say):
    import torch

    from auriclass_amd import engine

    L = engine.load()
    dev = "cuda:0"
    q_rows, q_len, stride = device_rows(nq, s, 7 + nq + s)
    r_rows, r_len, _ = device_rows(nr, s, nr + s)
    hit = [torch.zeros((nq, top), dtype=torch.int32, device=dev) for _ in range(3)]
    hit_dist = torch.zeros((nq, top), dtype=torch.float64, device=dev)
    n_hits = torch.zeros(nq, dtype=torch.int32, device=dev)
    chunk = max(1, min(nq, PAIR_LIMIT // nr))
    full = [torch.zeros((chunk, nr), dtype=torch.int32, device=dev), torch.zeros((chunk, nr), dtype=torch.int32, device=dev),
            torch.zeros((chunk, nr), dtype=torch.float64, device=dev)]
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def search(geometry):
        if geometry:
            os.environ["MHX_SEARCH_GEOMETRY"] = geometry
        ms = engine.dist_search_device(q_rows.data_ptr(), q_len.data_ptr(), nq, r_rows.data_ptr(), r_len.data_ptr(), nr, stride, K, s, top, max_dist,
                                       hit[0].data_ptr(), hit[1].data_ptr(), hit[2].data_ptr(), hit_dist.data_ptr(), n_hits.data_ptr())
        os.environ.pop("MHX_SEARCH_GEOMETRY", None)
        return ms, L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()

    yard = {}

    def yardstick():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        vals, counts = [], []
        t0.record()
        for q0 in range(0, nq, chunk):
            n = min(chunk, nq - q0)
            engine.dist_batch_device(q_rows[q0:].data_ptr(), q_len[q0:].data_ptr(), n, r_rows.data_ptr(), r_len.data_ptr(), nr, stride, K, s,
                                     full[0].data_ptr(), full[1].data_ptr(), full[2].data_ptr())
            ranges, fallbacks = L.mhx_last_dist_ranges(), L.mhx_last_dist_fallback_blocks()
            d = full[2][:n]
            keep = d <= max_dist
            vals.append(torch.topk(torch.where(keep, d, inf), min(top, nr), dim=1, largest=False).values)
            counts.append(keep.sum(dim=1).clamp(max=top))
        t1.record()
        torch.cuda.synchronize()
        yard["vals"], yard["n"] = torch.cat(vals), torch.cat(counts)
        return t0.elapsed_time(t1), ranges, fallbacks

    def agrees():
        n = n_hits.to(torch.int64)
        live = torch.arange(top, device=dev)[None, :] < n[:, None]
        want = yard["vals"]
        if want.shape[1] < top:
            want = torch.cat([want, inf.expand(nq, top - want.shape[1])], dim=1)
        return bool(torch.equal(n, yard["n"].to(torch.int64)) and torch.equal(hit_dist[live], want[live]))

    ways = {"search": lambda: search(None), "dist-geo": lambda: search("dist"), "yardstick": yardstick}
    info, times, same = {}, {w: [] for w in ways}, {}
    for w in ("yardstick", "search", "dist-geo"):   # warm-up: code objects, the workspace, the outputs' pages
        _, ranges, fallbacks = ways[w]()
        info[w] = (ranges, fallbacks)
        if w != "yardstick":
            same[w] = agrees()
    for _ in range(rounds):
        for w, call in ways.items():
            times[w].append(call()[0])
    say(f"{nq} queries x {nr} references, s = {s}, k = {K}, top = {top}, max_dist = {max_dist:g}: {nq * nr} pairs; hit counts and distances of "
        f"(a) and (b) equal the yardstick's: {same['search']} / {same['dist-geo']}")
    med = {w: statistics.median(v) for w, v in times.items()}
    for w, label in (("search", "(a) mhx_dist_search, triangle geometry"), ("dist-geo", "(b) mhx_dist_search, MHX_SEARCH_GEOMETRY=dist"),
                     ("yardstick", "(d) mhx_dist_batch + torch.topk")):
        v = times[w]
        say(f"  {label:46s} R = {info[w][0]:5d}  fallback blocks {info[w][1]}  ms: median {med[w]:10.3f}  best {min(v):10.3f}  worst {max(v):10.3f}   "
            f"{nq * nr / med[w] / 1e3:9.1f} M pairs/s   rounds " + " ".join(f"{x:.3f}" for x in v))
    say(f"  (a) / (d) = {med['search'] / med['yardstick']:.3f}   (b) / (d) = {med['dist-geo'] / med['yardstick']:.3f}   (a) / (b) = "
        f"{med['search'] / med['dist-geo']:.3f}   (medians)")
    if not all(same.values()):
        raise SystemExit("the search and the yardstick disagree")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top", type=int, default=5)
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1024x24x1000,1x100000x1000,1024x100000x1000,64x4096x10000")
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

    say(f"tools/search_rate.py on {engine.device_name()}: {args.rounds} interleaved rounds after a warm-up of each way; (a), (b): kernel time of "
        "the call (mhx_last_dist_kernel_ms), (d): device events around the yardstick's calls and its topk")
    for shape in args.shapes.split(","):
        nq, nr, s = (int(x) for x in shape.split("x"))
        measure(nq, nr, s, args.top, args.max_dist, args.rounds, say)


if __name__ == "__main__":
    main()

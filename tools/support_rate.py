"""What the jackknife support of search hits costs on the device (mhx_dist_support, device form) at R = 100 replicates, against
the path a user had before it, unchanged code: per query R times (mhx_resample_rows in device form over the query and its
candidates, then mhx_dist_batch in device form over the replicate's lists), which gives the same (common, denom).  Synthetic
sketches made on the device, k = 21 (27 at s = 50 000), keep = 0.5, seed = 42.

Shapes (queries x references x sketch size):

    1x24x50000        AuriClass's own: one sample against 24 references, all of them candidates
    1024x24x1000      a run of samples against 24 references, all of them candidates
    64x100000x1000    64 queries against a large reference set, the candidates the top 5 of mhx_dist_search (device form)

Ways, each timed with a host clock around calls that are complete when they return (a device synchronise before the clock stops):

    (a) fused      engine.dist_support_device: ONE call for all queries and replicates
    (b) yardstick  per query a row matrix [query, candidates] (gathered before the clock starts), then per replicate
                   mhx_resample_rows and mhx_dist_batch, both in device form.  Beyond --yard-queries queries the yardstick runs
                   on the first --yard-queries of them and its time is scaled by the number of queries, and said so

Before anything is timed the two ways must agree on every (common, denom) and s_r of the queries the yardstick runs.  Interleaved
rounds after a warm-up of each way, medians, and the spread between rounds.

    python tools/support_rate.py [--replicates 100] [--rounds 5] [--shapes 1x24x50000,1024x24x1000,64x100000x1000] [--out FILE]
"""
import argparse
import ctypes
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
KEEP, SEED = 0.5, 42


def make_rows(torch, n, s, gen, dev):
    """n ascending lists of s hashes below 2^62 (duplicates within a list: one chance in 10^13 per list)"""
    out = torch.empty((n, s), dtype=torch.int64, device=dev)
    for i0 in range(0, n, 8192):
        i1 = min(n, i0 + 8192)
        out[i0:i1] = torch.sort(torch.randint(0, 2 ** 62, (i1 - i0, s), dtype=torch.int64, device=dev, generator=gen), dim=1).values
    return out


def mutate(torch, rows, share, gen, dev):
    """every list with `share` of its hashes replaced by fresh ones"""
    fresh = torch.randint(0, 2 ** 62, rows.shape, dtype=torch.int64, device=dev, generator=gen)
    pick = torch.rand(rows.shape, device=dev, generator=gen) < share
    return torch.sort(torch.where(pick, fresh, rows), dim=1).values


def measure(shape, args, say):
    import torch

    from auriclass_amd import engine

    nq, nr, s = (int(x) for x in shape.split("x"))
    k = 27 if s >= 50000 else 21
    R = args.replicates
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(nq * 1000003 + nr * 101 + s)
    lib = engine.load()
    v = ctypes.c_void_p
    if nr <= 64:   # the references: copies of one base 2 % .. 30 % away; the queries: copies of the base 10 % away; all are candidates
        base = make_rows(torch, 1, s, gen, dev)
        refs = torch.cat([mutate(torch, base, 0.02 + 0.28 * i / max(nr - 1, 1), gen, dev) for i in range(nr)])
        q = mutate(torch, base.expand(nq, s).contiguous(), 0.10, gen, dev)
        top = nr
        cand = n_cand = None
    else:          # independent references; query i is a copy of reference 1000 i + 7, 20 % away; candidates: the search's top 5
        refs = make_rows(torch, nr, s, gen, dev)
        q = mutate(torch, refs[7::1000][:nq].contiguous(), 0.20, gen, dev)
        top = 5
    q_len = torch.full((nq,), s, dtype=torch.int32, device=dev)
    r_len = torch.full((nr,), s, dtype=torch.int32, device=dev)
    if nr > 64:
        cand = torch.zeros((nq, top), dtype=torch.int32, device=dev)
        hc, hd = torch.zeros_like(cand), torch.zeros_like(cand)
        n_cand = torch.zeros(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        engine.dist_search_device(q.data_ptr(), q_len.data_ptr(), nq, refs.data_ptr(), r_len.data_ptr(), nr, s, k, s, top, 1.0, cand.data_ptr(), hc.data_ptr(),
                                  hd.data_ptr(), 0, n_cand.data_ptr())
    first = torch.zeros((nq, top), dtype=torch.int32, device=dev)
    best, rep_s = (torch.zeros((nq, R), dtype=torch.int32, device=dev) for _ in range(2))
    rep_c, rep_d = (torch.zeros((nq, top, R), dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()

    def fused():
        t0 = time.perf_counter()
        ms = engine.dist_support_device(q.data_ptr(), q_len.data_ptr(), nq, refs.data_ptr(), r_len.data_ptr(), nr, s, s, top, R, KEEP, SEED,
                                        0 if cand is None else cand.data_ptr(), 0 if cand is None else n_cand.data_ptr(), first.data_ptr(), best.data_ptr(),
                                        rep_s.data_ptr(), rep_c.data_ptr(), rep_d.data_ptr())
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ms

    ny = min(nq, args.yard_queries)
    sets = []   # per query of the yardstick [query, candidates] and its lengths, gathered before the clock starts
    for i in range(ny):
        idx = torch.arange(nr, device=dev) if cand is None else cand[i].long()
        sets.append((torch.cat([q[i:i + 1], refs[idx]]).contiguous(), torch.full((top + 1,), s, dtype=torch.int32, device=dev)))
    o_rows = torch.zeros((top + 1, s), dtype=torch.int64, device=dev)
    o_len = torch.zeros(top + 1, dtype=torch.int32, device=dev)
    y_c, y_d = (torch.zeros((ny, R, top), dtype=torch.int32, device=dev) for _ in range(2))
    y_s = [[0] * R for _ in range(ny)]
    torch.cuda.synchronize()

    def yardstick():
        t0 = time.perf_counter()
        s_r = ctypes.c_uint32(0)
        for i, (rows, lens) in enumerate(sets):
            for r in range(R):
                engine._check(lib.mhx_resample_rows(v(rows.data_ptr()), v(lens.data_ptr()), top + 1, s, s, SEED, r, KEEP, v(o_rows.data_ptr()), v(o_len.data_ptr()),
                                                    ctypes.byref(s_r), 1))
                y_s[i][r] = s_r.value
                engine.dist_batch_device(o_rows.data_ptr(), o_len.data_ptr(), 1, o_rows[1:].data_ptr(), o_len[1:].data_ptr(), top, s, k, s_r.value,
                                         y_c[i, r].data_ptr(), y_d[i, r].data_ptr(), 0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    warm_a, _ = fused()
    warm_b = yardstick()
    same = (torch.equal(rep_c[:ny].permute(0, 2, 1), y_c) and torch.equal(rep_d[:ny].permute(0, 2, 1), y_d) and rep_s[:ny].cpu().tolist() == y_s)
    f = first.cpu()
    say(f"tools/support_rate.py on {engine.device_name()}: {nq} queries x {nr} references, s = {s}, k = {k}, top = {top}, R = {R}, keep = {KEEP}, seed = {SEED}; "
        f"s_r {int(rep_s.min())} .. {int(rep_s.max())}; first: {int((f == R).sum())} candidates best in every replicate, {int(((f > 0) & (f < R)).sum())} in some; "
        f"(common, denom) and s_r of the two ways the same for the {ny} queries the yardstick runs: {same}")
    if not same:
        raise SystemExit("the two ways disagree")
    wall = {"a": [], "k": [], "b": []}
    for _ in range(args.rounds):
        t, ms = fused()
        wall["a"].append(t)
        wall["k"].append(ms / 1e3)
        wall["b"].append(yardstick() * (nq / ny))
    say(f"{args.rounds} interleaved rounds after a warm-up of each way (warm-up: fused {warm_a * 1e3:.3f} ms, yardstick {warm_b * 1e3:.3f} ms for {ny} queries)"
        + (f"; the yardstick ran {ny} of {nq} queries, its time is scaled by {nq / ny:g}" if ny < nq else ""))

    def row(label, x):
        x = [t * 1e3 for t in x]
        say(f"  {label:58s} median {statistics.median(x):11.3f} ms  best {min(x):11.3f}  worst {max(x):11.3f}   rounds " + " ".join(f"{t:.3f}" for t in x))
        return statistics.median(x), (max(x) - min(x))
    ta, sa = row("(a) dist_support_device, all queries and replicates, wall", wall["a"])
    row("    of which mhx_last_dist_kernel_ms (stream time)", wall["k"])
    tb, sb = row("(b) R x (resample_rows + dist_batch) per query, wall", wall["b"])
    say(f"  (b) / (a) = {tb / ta:.1f}; spread between rounds: (a) {sa:.3f} ms, (b) {sb:.3f} ms; (a) not slower than (b) beyond the spread: {ta <= tb + sa + sb}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1x24x50000,1024x24x1000,64x100000x1000")
    ap.add_argument("--yard-queries", type=int, default=16, help="queries the yardstick runs at most; its time is scaled to all of them")
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
    for shape in args.shapes.split(","):
        measure(shape, args, say)


if __name__ == "__main__":
    main()

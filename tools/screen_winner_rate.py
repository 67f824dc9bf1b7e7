"""Cost of the winner-take-all finish of the containment screen (Screener.finish(winner=True)) next to the plain finish(),
on the same table and counts, and -- with --parent-lib -- next to the plain finish() of another libmhx build (the parent
commit's) on the same input:

    24 x 50 000 entries   k = 27, a clade of 24 mutated copies of one genome, sketched on the device
    4096 x 1000 entries   k = 21, 64 clades of 64 references drawn from the bottom hashes of the genome the reads cover,
                          each with a quarter of foreign hashes (a RefSeq-sized row count with heavy sharing inside a clade)

The reads (30x of the first genome) are pushed once; finish() is then timed call by call, host clock around the call (it
ends with the copy of shared / median and a stream synchronisation): first the plain finish() alone ("plain", the figure
to compare between libraries), then winner and plain alternating ("winner", and "between": the plain finish() that follows
a winner finish, whose working set is another).  Each library runs in
its own process (MHX_LIB), the processes interleaved round by round; the figures are medians per process and their range
over the rounds, which is the run-to-run spread to read a difference against.

    python tools/screen_winner_rate.py [--parent-lib PATH] [--rounds R] [--reps N]
    python tools/screen_winner_rate.py --child --once      (one table, one plain and one winner finish: for a kernel trace)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ("24x50000", "4096x1000")


def tables(shape):
    import numpy as np

    from auriclass_amd import engine, synth

    def gpu_sketch(genome, k, s):
        sk = engine.Sketcher(k, s, 1, expected_bytes=genome.size + 1)
        sk.push_host(genome.tobytes() + b"\n", engine.FMT_SEQ)
        h, _ = sk.finish()
        sk.close()
        return h

    g = synth.make_genome(1_000_000, 42)
    if shape == "24x50000":
        k, s = 27, 50_000
        refs = [gpu_sketch(g, k, s)] + [gpu_sketch(synth.mutate(g, 0.0005 * (1 + i % 6), 100 + i), k, s) for i in range(23)]
    else:
        k, s = 21, 1000
        rng = np.random.default_rng(5)
        pool = gpu_sketch(g, k, 200_000)
        refs = []
        for clade in range(64):
            own = rng.choice(pool, size=3000, replace=False)
            for _ in range(64):
                refs.append(np.unique(np.concatenate([rng.choice(own, size=750, replace=False),
                                                      rng.integers(0, 1 << 63, size=250, dtype=np.uint64)])))
    stride = max(len(r) for r in refs)
    rows = np.zeros((len(refs), stride), dtype=np.uint64)
    for i, r in enumerate(refs):
        rows[i, :len(r)] = r
    lens = np.array([len(r) for r in refs], dtype=np.uint32)
    lengths = np.full(len(refs), 1_000_000, dtype=np.uint64)
    fq = synth.make_fastq(g, 200_000, 150, 43)
    return k, s, rows, lens, lengths, fq.numpy()


def child(args):
    sys.path.insert(0, str(ROOT))
    from auriclass_amd import engine

    engine.init(0)
    has_winner = hasattr(engine.load(), "mhx_screener_finish_winner")
    out = {}
    for shape in SHAPES[:1] if args.once else SHAPES:
        k, s, rows, lens, lengths, fq = tables(shape)
        sc = engine.Screener(k, rows, lens, s, with_set_size=False)
        sc.push_host(fq, engine.FMT_FASTQ4)
        sc.sync()

        def timed(fn):
            t0 = time.perf_counter()
            r = fn()
            return (time.perf_counter() - t0) * 1e3, r

        # block A: plain finish() alone -- the comparison between libraries; block B: plain and winner alternating
        plain, between, winner = [], [], []
        shared_p = shared_w = None
        for i in range(1 if args.once else args.reps + 3):
            t, r = timed(lambda: sc.finish())
            shared_p = r[0]
            if i >= 3:
                plain.append(t)
        for i in range(0 if not has_winner else 1 if args.once else args.reps + 3):
            t, r = timed(lambda: sc.finish(winner=True, ref_length=lengths))
            shared_w = r[0]
            if i >= 3:
                winner.append(t)
            t, r = timed(lambda: sc.finish())
            assert (r[0] == shared_p).all()
            if i >= 3:
                between.append(t)
        sc.close()
        if args.once:
            continue
        out[shape] = {"plain_ms": statistics.median(plain), "plain_min": min(plain), "plain_max": max(plain),
                      "shared_plain": int(shared_p.sum())}
        if has_winner:
            out[shape].update({"winner_ms": statistics.median(winner), "winner_min": min(winner), "winner_max": max(winner),
                               "between_ms": statistics.median(between), "shared_winner": int(shared_w.sum())})
    print("WRESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = [("branch", ROOT / "auriclass_amd" / "lib" / "libmhx.so")]
    if args.parent_lib:
        libs.insert(0, ("parent", Path(args.parent_lib).resolve()))
    res = {name: [] for name, _ in libs}
    for rd in range(args.rounds):
        for name, lib in libs:
            env = dict(os.environ, MHX_LIB=str(lib))
            cmd = [sys.executable, __file__, "--child", "--reps", str(args.reps)]
            # nothing more is started on a GPU that a run may have faulted or hung: the failure is looked into first
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{name} hung in round {rd}: stopped")
            line = [x for x in p.stdout.splitlines() if x.startswith("WRESULT ")]
            if p.returncode != 0 or not line:
                print(f"{name}: FAILED rc={p.returncode}\n{p.stdout[-500:]}\n{p.stderr[-1500:]}", flush=True)
                raise SystemExit(f"{name} failed in round {rd}: stopped")
            r = json.loads(line[0][8:])
            res[name].append(r)
            for shape in SHAPES:
                x = r[shape]
                print(f"round {rd} {name:7s} {shape:10s} plain {x['plain_ms']:.3f} ms [{x['plain_min']:.3f}, {x['plain_max']:.3f}]" +
                      (f"  winner {x['winner_ms']:.3f} ms [{x['winner_min']:.3f}, {x['winner_max']:.3f}]  sum shared {x['shared_plain']} -> "
                       f"{x['shared_winner']}" if "winner_ms" in x else f"  sum shared {x['shared_plain']}"), flush=True)
    print(f"---- medians over {args.rounds} processes of {args.reps} calls each [lowest, highest process median] ----")
    for shape in SHAPES:
        for name, _ in libs:
            for what in ("plain_ms", "between_ms", "winner_ms"):
                v = [r[shape][what] for r in res[name] if what in r[shape]]
                if v:
                    med = statistics.median(v)
                    print(f"{shape:10s} {name:7s} {what[:-3]:7s} finish {med:8.3f} ms  [{min(v):.3f}, {max(v):.3f}]  "
                          f"spread {100 * (max(v) - min(v)) / med:.1f} %")


if __name__ == "__main__":
    main()

"""`python -m auriclass_amd.search [-n TOP | --all] [-d MAX_DIST] [-v MAX_P] [-p N] [--support R [--keep F] [--seed N] [--clades FILE]]
REF.msh QUERY.msh [QUERY.msh ...]`: for every
query sketch its TOP closest references of REF.msh within MAX_DIST, best first, as `mash dist` rows (engine.search_files).
--support R adds a column "c/R": in how many of R jackknife replicates of the sketches (each keeps the share --keep of the
hashes, drawn from --seed) the row's reference is the best of the query's hits; --clades FILE (AuriClass's clade_config.csv)
adds the clade of the row's reference and "g/R", the replicates whose best hit has that clade.
--all -d MAX_DIST prints EVERY reference within MAX_DIST of each query, best first, with no cap on the hits of a query
(engine.within_files); it needs an explicit -d and goes with none of -n, --support, --keep, --seed and --clades.
Ranking and filtering happen on the device, so REF.msh may hold a reference set far too large to print in full.  Inputs are
sketch files: a sequence file is refused with the hint to sketch it first.  Exit status 1 with the engine's message when
the call fails.  -p (threads) is accepted and ignored: the engine has its own."""
from __future__ import annotations

import argparse
import sys
from typing import List

from auriclass_amd import engine


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m auriclass_amd.search", description="closest references of a sketch set, per query sketch")
    ap.add_argument("-n", dest="top", type=int, default=None, help="hits per query, 1 .. 64 [5]")
    ap.add_argument("--all", dest="all_hits", action="store_true", help="every hit within -d, best first, no cap; needs -d")
    ap.add_argument("-d", dest="max_dist", type=float, default=None, help="maximum distance to report [1]")
    ap.add_argument("-v", dest="max_p_value", type=float, default=1.0, help="maximum p-value to report (drops rows, promotes none) [1]")
    ap.add_argument("-p", dest="threads", type=int, default=1, help="ignored")
    ap.add_argument("--support", dest="replicates", type=int, default=None, metavar="R", help="jackknife replicates, 0 .. 10000: a support column c/R [none]")
    ap.add_argument("--keep", type=float, default=None, metavar="F", help="share of the hashes a replicate keeps, (0, 1] [0.5]; needs --support")
    ap.add_argument("--seed", type=int, default=None, metavar="N", help="seed of the replicates [42]; needs --support")
    ap.add_argument("--clades", default=None, metavar="FILE", help="clade table (filename,clade): clade and g/R columns; needs --support")
    ap.add_argument("reference", metavar="REF.msh")
    ap.add_argument("queries", metavar="QUERY.msh", nargs="+")
    try:
        args = ap.parse_args(argv)
    except SystemExit as exc:
        return 0 if exc.code == 0 else 1
    for path in [args.reference] + args.queries:
        if not str(path).endswith(".msh"):
            sys.stderr.write(f"ERROR: the search takes sketch files only; sketch {path} first (mash sketch [-i] -o <out> ...) and pass the .msh\n")
            return 1
    if args.all_hits:
        if args.max_dist is None:
            sys.stderr.write("ERROR: --all needs an explicit -d MAX_DIST\n")
            return 1
        for flag, given in (("-n", args.top), ("--support", args.replicates), ("--keep", args.keep), ("--seed", args.seed), ("--clades", args.clades)):
            if given is not None:
                sys.stderr.write(f"ERROR: --all cannot be combined with {flag}\n")
                return 1
        try:
            sys.stdout.write(engine.within_files(args.reference, args.queries, args.max_dist, args.max_p_value, order=1))
        except engine.EngineError as exc:
            sys.stderr.write(exc.message + "\n")
            return 1
        return 0
    if args.replicates is None and (args.keep is not None or args.seed is not None or args.clades is not None):
        sys.stderr.write("ERROR: --keep, --seed and --clades need --support R\n")
        return 1
    if args.replicates is not None and not 0 <= args.replicates <= 10000:
        sys.stderr.write("ERROR: --support takes 0 .. 10000 replicates\n")
        return 1
    if args.seed is not None and not 0 <= args.seed < 1 << 64:
        sys.stderr.write("ERROR: --seed takes 0 .. 2^64 - 1\n")
        return 1
    args.top = 5 if args.top is None else args.top
    args.max_dist = 1.0 if args.max_dist is None else args.max_dist
    try:
        text = engine.search_files(args.reference, args.queries, top=args.top, max_dist=args.max_dist, max_p_value=args.max_p_value,
                                   replicates=args.replicates or 0, keep=0.5 if args.keep is None else args.keep,
                                   seed=42 if args.seed is None else args.seed, clades=args.clades)
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

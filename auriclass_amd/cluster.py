"""`python -m auriclass_amd.cluster -d MAX_DIST [--linkage single|complete|average] [--rep first|longest|medoid] [--dist] [-C] [-o REPS.msh]
[-p N] SET.msh [SET.msh ...]`: the references of all sketch files are one set; those within MAX_DIST of each other are joined (single linkage) on the device,
and every reference gets a row "cluster\\tsize\\trepresentative\\tmember\\tdegree" (engine.cluster_files).  -o writes the
representatives, unchanged, as a sketch file: the dereplicated set, which the search, `mash dist` and `mash screen` read.
--linkage complete|average cuts the complete- or average-linkage merges at MAX_DIST instead (engine.linkage_files): with complete
linkage every two members of a cluster are within MAX_DIST of each other; the rows have no degree column.
--rep medoid makes the representative of a cluster its medoid -- the member with the smallest sum of distances to the others,
ties to the lower index --, and --dist prints how far every member lies from its representative; either one, for every
--linkage, gives the rows "cluster\\tsize\\trepresentative\\tmember\\tdist\\tp\\tcommon/denom" (engine.cluster_reps_files), the last
three fields as `mash triangle -E` prints them for the pair (member, representative).  Without both the output is as before.
Inputs are sketch files: a sequence file is refused with the hint to sketch it first.  -d is required: no bound is a sensible
default for "the same thing".  Exit status 1 with the engine's message when the call fails.  -p (threads) is accepted and
ignored: the engine has its own."""
from __future__ import annotations

import argparse
import sys
from typing import List

from auriclass_amd import engine


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m auriclass_amd.cluster", description="single-linkage clusters of a sketch set and one representative of each")
    ap.add_argument("-d", dest="max_dist", type=float, required=True, help="references within this distance are neighbours (required)")
    ap.add_argument("--linkage", choices=["single", "complete", "average"], default="single", help="how clusters are compared [single]")
    ap.add_argument("--rep", choices=sorted(engine.CLUSTER_REPS_REPS), default="first",
                    help="representative of a cluster: its first member, its longest, or its medoid (the smallest sum of distances to the others) [first]")
    ap.add_argument("--dist", dest="dist", action="store_true", help="print the distance of every member to its representative (dist, p, common/denom)")
    ap.add_argument("-C", dest="comment", action="store_true", help="print comments in place of names")
    ap.add_argument("-o", dest="out", default=None, metavar="REPS.msh", help="write the representatives as a sketch file")
    ap.add_argument("-p", dest="threads", type=int, default=1, help="ignored")
    ap.add_argument("sets", metavar="SET.msh", nargs="+")
    try:
        args = ap.parse_args(argv)
    except SystemExit as exc:
        return 0 if exc.code == 0 else 1
    for path in args.sets:
        if not str(path).endswith(".msh"):
            sys.stderr.write(f"ERROR: the clustering takes sketch files only; sketch {path} first (mash sketch [-i] -o <out> ...) and pass the .msh\n")
            return 1
    try:
        if args.dist or args.rep == "medoid":
            text = engine.cluster_reps_files(args.sets, args.max_dist, linkage=args.linkage, rep=args.rep, comment=args.comment, out=args.out)
        elif args.linkage == "single":
            text = engine.cluster_files(args.sets, args.max_dist, comment=args.comment, rep=args.rep, out=args.out)
        else:
            text = engine.linkage_files(args.sets, args.linkage, mode="cut", comment=args.comment, max_dist=args.max_dist, rep=args.rep, out=args.out)
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`python -m auriclass_amd.tree [-C] [--newick] [--linkage single|complete|average] [--nj [--support R [--keep F] [--seed N]]]
[-p N] SET.msh [SET.msh ...]`: the references of all sketch files are one set;
its single-linkage tree -- the minimum spanning tree of all pairwise distances, computed on the device -- is printed as one
row per merge in merge order, "name_i\\tname_j\\tdist\\tp\\tcommon/denom\\tclusters" (engine.tree_files): the gaps in the dist
column are the distances at which `python -m auriclass_amd.cluster -d D` changes its answer.  --newick prints the dendrogram
instead (node height = merge distance).  --linkage complete|average agglomerates by complete or average linkage instead
(engine.linkage_files): rows "name_a\\tname_b\\tdist\\tsize\\tclusters", or the dendrogram under --newick.  --nj builds the
unrooted neighbour-joining tree instead (engine.nj_files): rows "name_a\\tname_b\\tlen_a\\tlen_b\\tdist\\tnodes", or the tree
under --newick; it is no linkage, so --nj with --linkage complete|average is refused.  --nj --support R adds jackknife support
from R replicates, each keeping the share --keep [0.5] of the sketch hashes chosen by --seed [42]: a seventh column "c/R" in the
table, the label floor(100 c / R) on every inner node but the root under --newick; --support 0 is the plain tree, --support
without --nj is refused.  Inputs are sketch files: a sequence file
is refused with the hint to sketch it first.  Exit status 1 with the engine's message when the call fails.  -p (threads) is
accepted and ignored: the engine has its own."""
from __future__ import annotations

import argparse
import sys
from typing import List

from auriclass_amd import engine


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m auriclass_amd.tree", description="single-linkage tree of a sketch set: its merges, or a Newick dendrogram")
    ap.add_argument("-C", dest="comment", action="store_true", help="print comments in place of names")
    ap.add_argument("--newick", action="store_true", help="print the dendrogram in Newick format in place of the merge table")
    ap.add_argument("--linkage", choices=["single", "complete", "average"], default="single", help="how clusters are compared [single]")
    ap.add_argument("--nj", action="store_true", help="neighbour joining: the unrooted tree in place of a dendrogram")
    ap.add_argument("--support", type=int, default=None, metavar="R", help="with --nj: jackknife support of every join from R replicates")
    ap.add_argument("--keep", type=float, default=0.5, metavar="F", help="the share of the sketch hashes a replicate keeps, (0, 1] [0.5]")
    ap.add_argument("--seed", type=int, default=42, metavar="N", help="the seed of the replicates [42]")
    ap.add_argument("-p", dest="threads", type=int, default=1, help="ignored")
    ap.add_argument("sets", metavar="SET.msh", nargs="+")
    try:
        args = ap.parse_args(argv)
    except SystemExit as exc:
        return 0 if exc.code == 0 else 1
    if args.nj and args.linkage != "single":
        sys.stderr.write("ERROR: --nj is no linkage: it does not go with --linkage complete|average\n")
        return 1
    if args.support is not None and not args.nj:
        sys.stderr.write("ERROR: --support counts the splits of the neighbour-joining tree: it goes with --nj only\n")
        return 1
    if args.support is not None and args.support < 0:
        sys.stderr.write("ERROR: --support takes a number of replicates, 0 or more\n")
        return 1
    if args.seed < 0 or args.seed >= 1 << 64:
        sys.stderr.write("ERROR: --seed takes a number in 0 .. 2^64 - 1\n")
        return 1
    for path in args.sets:
        if not str(path).endswith(".msh"):
            sys.stderr.write(f"ERROR: the tree takes sketch files only; sketch {path} first (mash sketch [-i] -o <out> ...) and pass the .msh\n")
            return 1
    try:
        if args.nj:
            text = engine.nj_files(args.sets, comment=args.comment, newick=args.newick, replicates=args.support or 0, keep=args.keep, seed=args.seed)
        elif args.linkage == "single":
            text = engine.tree_files(args.sets, comment=args.comment, newick=args.newick)
        else:
            text = engine.linkage_files(args.sets, args.linkage, mode="newick" if args.newick else "merges", comment=args.comment)
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`python -m auriclass_amd.contain [-w | -n TOP [-c MIN_SHARED] | --all [-c MIN_SHARED] [--order best|ref]] [-i MIN_IDENTITY] [-v MAX_P] [-C] [-p N]
REF.msh QUERY.msh [QUERY.msh ...]`: which share of
each reference sketch of REF.msh every query sketch holds, from the sketch files alone (engine.contain_files).  One row per
(query, reference): reference, query, identity, p-value, shared/n_ref, shared/n_qry -- within the window in which both
sketches are complete, n_ref hashes of the reference and n_qry of the query lie, `shared` of them in both.  A sample that
holds the reference next to anything else keeps identity 1 where `mash dist` moves away.  REF.msh may have another sketch
size than the queries.  -i and -v drop rows, -C prints the comment fields in place of the names.  Inputs are sketch files: a
sequence file is refused with the hint to sketch it first.  Exit status 1 with the engine's message when the call fails.
-p (threads) is accepted and ignored: the engine has its own.
-w: winner-take-all.  Every hash a query shares with the reference set is credited to one reference -- the one with the
greatest shared/n_ref for that query, then the greatest genome length, then the first in the file -- and the rows show what
each reference won in the place of `shared`, in all four columns; -i and -v filter on those values.  The members of a clade
then no longer repeat one another's row.
-n TOP (1 .. 64): per query only the TOP references it holds the largest share of, ranked on the device -- by shared/n_ref
exactly, then the larger `shared`, then the order in REF.msh -- best first; a query without hits prints nothing.  -i and -c
(a hit shares at least MIN_SHARED hashes, default 1: a one-hash reference inside a tiny window reaches 1/1) say what a hit
is and act before the cut; -v drops rows from the result already chosen and promotes none.  Not with -w, whose ranking is
per hash, not per pair; -c needs -n or --all.
--all: per query EVERY reference that is a hit by -i and -c, with no cap, taken out on the device as CSR
(engine.dist_contain_within): what -n cannot give when one mixed culture or one clade of near-identical references passes 64
rows.  --order best (the default) prints a query's hits in the order of -n, --order ref in the order of REF.msh; -v drops
rows; a query without hits prints nothing.  Not with -n or -w; --order needs --all."""
from __future__ import annotations

import argparse
import sys
from typing import List

from auriclass_amd import engine


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m auriclass_amd.contain", description="share of each reference sketch inside a query sketch")
    ap.add_argument("-i", dest="min_identity", type=float, default=0.0, help="minimum identity to report [0]")
    ap.add_argument("-v", dest="max_p_value", type=float, default=1.0, help="maximum p-value to report [1]")
    ap.add_argument("-w", dest="winner", action="store_true", help="winner-take-all: credit each shared hash to its best reference")
    ap.add_argument("-n", dest="top", type=int, default=None, help="per query only the TOP (1 .. 64) best references, ranked by shared/n_ref")
    ap.add_argument("-c", dest="min_shared", type=int, default=None, help="with -n or --all: a hit shares at least this many hashes [1]")
    ap.add_argument("--all", dest="all_hits", action="store_true", help="per query every reference that is a hit by -i and -c, with no cap")
    ap.add_argument("--order", dest="order", choices=("best", "ref"), default=None, help="with --all: a query's hits best first or in reference order [best]")
    ap.add_argument("-C", dest="comment", action="store_true", help="show comment fields in place of the names")
    ap.add_argument("-p", dest="threads", type=int, default=1, help="ignored")
    ap.add_argument("reference", metavar="REF.msh")
    ap.add_argument("queries", metavar="QUERY.msh", nargs="+")
    try:
        args = ap.parse_args(argv)
    except SystemExit as exc:
        return 0 if exc.code == 0 else 1
    for path in [args.reference] + args.queries:
        if not str(path).endswith(".msh"):
            sys.stderr.write(f"ERROR: contain takes sketch files only; sketch {path} first (mash sketch [-i] -o <out> ...) and pass the .msh\n")
            return 1
    if args.top is not None and args.winner:
        sys.stderr.write("ERROR: contain -n ranks pairs and -w credits every hash to one reference: not both\n")
        return 1
    if args.all_hits and (args.top is not None or args.winner):
        sys.stderr.write("ERROR: contain --all lists every hit; -n cuts the list and -w credits every hash to one reference: not together\n")
        return 1
    if args.order is not None and not args.all_hits:
        sys.stderr.write("ERROR: contain --order (the order of a query's hits) needs --all\n")
        return 1
    if args.min_shared is not None and args.top is None and not args.all_hits:
        sys.stderr.write("ERROR: contain -c (minimum shared hashes of a hit) needs -n\n")
        return 1
    if args.top is not None and not 1 <= args.top <= 64:
        sys.stderr.write("ERROR: contain -n: top must be 1 .. 64\n")
        return 1
    if args.min_shared is not None and args.min_shared < 1:
        sys.stderr.write("ERROR: contain -c: a hit shares at least 1 hash\n")
        return 1
    more = {"winner": True} if args.winner else {}
    if args.top is not None:
        more = {"top": args.top, "min_shared": 1 if args.min_shared is None else args.min_shared}
    if args.all_hits:
        more = {"all_hits": True, "order": 0 if args.order == "ref" else 1, "min_shared": 1 if args.min_shared is None else args.min_shared}
    try:
        text = engine.contain_files(args.reference, args.queries, min_identity=args.min_identity, max_p_value=args.max_p_value, comment=args.comment, **more)
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

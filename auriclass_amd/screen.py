"""`python -m auriclass_amd.screen [-w] [-i X] [-v P] [-p N] REF.msh reads...`: the containment screen (`mash screen`) with
the flags the `mash` shim does not serve -- -w winner-take-all, -i minimum identity, -v maximum p-value.  Prints the rows
of engine.screen_files; exit status 1 with the engine's message when it fails.  Without -i every row is printed (-i -1;
mash's own default is -i 0, rows with identity > 0).  -p (threads) is accepted and ignored: the engine has its own."""
from __future__ import annotations

import argparse
import sys
from typing import List

from auriclass_amd import engine


def main(argv: List[str] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m auriclass_amd.screen", description="containment of reference sketches in a read set")
    ap.add_argument("-w", dest="winner", action="store_true", help="winner-take-all: a hash counts for the best reference that holds it")
    ap.add_argument("-i", dest="min_identity", type=float, default=-1.0, help="minimum identity to report (0: above zero only, -1: all) [-1]")
    ap.add_argument("-v", dest="max_p_value", type=float, default=1.0, help="maximum p-value to report [1]")
    ap.add_argument("-p", dest="threads", type=int, default=1, help="ignored")
    ap.add_argument("reference", metavar="REF.msh")
    ap.add_argument("reads", nargs="+")
    try:
        args = ap.parse_args(argv)
    except SystemExit as exc:
        return 0 if exc.code == 0 else 1
    try:
        text, _ = engine.screen_files(args.reference, args.reads, winner=args.winner, min_identity=args.min_identity,
                                      max_p_value=args.max_p_value)
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

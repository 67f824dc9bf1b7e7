"""A `mash`-named command for an UNMODIFIED AuriClass checkout: put the directory holding the
`mash` launcher (auriclass_amd/bin) first on PATH and the reference's five subprocess call sites
(/root/reference/auriclass/general.py:198-205 `mash -h`; classes.py:576-596 and 696-706
`mash sketch`; classes.py:92-97 `mash dist`; classes.py:305-312 `mash bounds`) run on the GPU
engine.  `mash dist` also takes several queries and the filters -d / -v (every reference within a distance of each query:
engine.within_files); without a filter its calls and its bytes are those of the two-argument form.  `mash screen REF.msh reads...` (containment) and `mash sketch -i` (one sketch per sequence of a file: how a
reference set is made from one multi-FASTA) are served too, and `mash triangle SET.msh ...` (all pairs within a sketch
set: matrix or, with -E / -d / -v, edge list); AuriClass itself calls none of them.  Only the argv subsets AuriClass uses are understood; stdout/stderr text and exit
codes follow mash (sketch: exit 1 with 'ERROR: Did not find fasta records in ...')."""
from __future__ import annotations

import sys
from typing import List

from auriclass_amd import engine

USAGE = """
Mash version 2.3 (mhx GPU engine)

Type 'mash --license' for license and copyright information.

Usage:

  mash <command> [options] [arguments ...]

Commands:

  bounds    Print a table of Mash error bounds.

  dist      Estimate the distance of query sequences to references.

  screen    Determine whether query sequences are within a larger pool of sequences.

  sketch    Create sketches (reduced representations for fast operations).

  triangle  Estimate the distance of each sequence to every other sequence.

"""


def _take(args: List[str], flag: str, default=None, cast=str):
    if flag in args:
        i = args.index(flag)
        value = cast(args[i + 1])
        del args[i:i + 2]
        return value
    return default


def main(argv: List[str] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        sys.stdout.write(USAGE)
        return 0
    cmd, args = argv[0], argv[1:]
    try:
        if cmd == "sketch":
            reads = "-r" in args
            if reads:
                args.remove("-r")
            individual = "-i" in args
            if individual:
                args.remove("-i")
            if individual and reads:
                sys.stderr.write("ERROR: mash sketch -i (one sketch per sequence) cannot be combined with -r in the mhx shim\n")
                return 1
            m = _take(args, "-m", 1, int)
            out = _take(args, "-o", None)
            k = _take(args, "-k", 21, int)
            s = _take(args, "-s", 1000, int)
            if out is None or not args:
                sys.stderr.write("ERROR: mash sketch needs -o <out> and at least one input\n")
                return 1
            if not out.endswith(".msh"):
                out += ".msh"
            try:
                text, _ = engine.sketch_files(args, k, s, out, reads=reads, min_mult=m if reads else 1, individual=individual)
            except engine.NoRecordsError as exc:
                sys.stderr.write("\n" + exc.message + "\n")
                return 1
            sys.stderr.write(text)
            return 0
        if cmd == "dist":
            for flag in ("-t", "-l", "-C", "-i", "-k", "-s", "-r", "-m", "-a", "-z", "-S", "-w", "-b", "-g", "-c", "-n", "-Z", "-M", "-I"):
                if flag in args:
                    sys.stderr.write(f"ERROR: mash dist {flag} is not supported by the mhx shim\n")
                    return 1
            _take(args, "-p", 1, int)   # threads: the engine has its own
            max_dist = _take(args, "-d", None, float)
            max_p = _take(args, "-v", None, float)
            if len(args) < 2:
                sys.stderr.write("ERROR: mash dist [-d <max distance>] [-v <max p-value>] <reference> <query> [<query> ...]\n")
                return 1
            if max_dist is not None or max_p is not None:   # mash prints a pair iff distance <= -d && p <= -v, in reference order
                sys.stdout.write(engine.within_files(args[0], args[1:], 1.0 if max_dist is None else max_dist,
                                                     1.0 if max_p is None else max_p, order=0))
            elif len(args) == 2:
                sys.stdout.write(engine.dist_files(args[0], args[1]))
            else:
                sys.stdout.write(engine.dist_files_multi(args[0], args[1:]))
            return 0
        if cmd == "screen":
            for flag in ("-w", "-i", "-v", "-a"):
                if flag in args:
                    sys.stderr.write(f"ERROR: mash screen {flag} is not supported by the mhx shim\n")
                    return 1
            _take(args, "-p", 1, int)   # threads: the engine has its own
            if len(args) < 2:
                sys.stderr.write("ERROR: mash screen <reference.msh> <reads> [<reads> ...]\n")
                return 1
            text, _ = engine.screen_files(args[0], args[1:])
            sys.stdout.write(text)
            return 0
        if cmd == "triangle":
            for flag in ("-i", "-k", "-s", "-r", "-m", "-l", "-a", "-z", "-S", "-w", "-b", "-g", "-c", "-n", "-Z", "-M", "-I"):
                if flag in args:
                    sys.stderr.write(f"ERROR: mash triangle {flag} is not supported by the mhx shim (inputs are sketch files)\n")
                    return 1
            _take(args, "-p", 1, int)   # threads: the engine has its own
            edge = "-E" in args
            if edge:
                args.remove("-E")
            comment = "-C" in args
            if comment:
                args.remove("-C")
            max_dist = _take(args, "-d", 1.0, float)
            max_p = _take(args, "-v", 1.0, float)
            if not args:
                sys.stderr.write("ERROR: mash triangle <sketches.msh> [<sketches.msh> ...]\n")
                return 1
            for path in args:
                if not str(path).endswith(".msh"):
                    sys.stderr.write(f"ERROR: mash triangle in the mhx shim takes sketch files only; sketch {path} first "
                                     "(mash sketch [-i] -o <out> ...) and pass the .msh\n")
                    return 1
            sys.stdout.write(engine.triangle_files(args, edge=edge, comment=comment, max_dist=max_dist, max_p_value=max_p))
            return 0
        if cmd == "bounds":
            k = _take(args, "-k", 21, int)
            p = _take(args, "-p", 0.99, float)
            sys.stdout.write(engine.bounds(k, p))
            return 0
    except engine.EngineError as exc:
        sys.stderr.write(exc.message + "\n")
        return 1
    sys.stderr.write(f"ERROR: unsupported mash command for the mhx shim: {cmd}\n")
    return 1


if __name__ == "__main__":
    sys.exit(main())

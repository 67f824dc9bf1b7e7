"""The FASTA files the device parser is pinned with (tests/test_fasta_emulation.py on the CPU emulator,
tests/test_gpu_fasta_stream.py on the GPU; expectation: tests/fasta_rule.py).  Every case is the smallest file at which one
particular slip would show: a byte dropped or doubled at the edge of a 64-byte chunk or a 16 KiB tile, a start state
carried wrongly over tiles without a line start, a wrong share of tiles per thread in the offsets pass, a record list that
outgrows its inline copy or its capacity.  All of them are generated from seeds; none is stored."""
from typing import Callable, Dict, List, Tuple

import numpy as np

CHUNK, TILE = 64, 16384
SEPS_INLINE, SEPS_CAP = 4096, 65536      # kFastaSepsInline, the first capacity of the record list (mhx_files.cpp)
ACGT = np.frombuffer(b"ACGT", np.uint8)
EDGES = (63, 64, 65, 16383, 16384, 16385, 32767, 32768)

Case = Tuple[str, bytes]


def acgt(rng, n: int) -> bytes:
    return rng.choice(ACGT, size=n).tobytes()


def fill_lines(rng, length: int, width: int = 70) -> bytes:
    """exactly `length` bytes of ACGT lines of up to `width` columns, the last byte a newline"""
    assert length >= 1
    a = rng.choice(ACGT, size=length)
    a[length - 1::-(width + 1)] = 0x0A
    return a.tobytes()


# ---- tiny files: every n mod 16 and mod 64, files that end inside, at and one past a chunk ---------------------------
def tiny() -> List[Case]:
    rng = np.random.default_rng(101)
    body = acgt(rng, 40000)
    out = []
    for n in list(range(1, 131)) + [16383, 16384, 16385, 32768]:
        out.append((f"gt*{n}", b">" * n))
        out.append((f"gt-nl*{n}", (b">\n" * (n // 2 + 1))[:n]))
        out.append((f"gt-a*{n}", (b">" + b"a" * n)[:n]))
        out.append((f"rec[{n}]", (b">a\n" + body)[:n]))
        out.append((f"rec-nl[{n}]", (b">a\n" + body)[:n - 1] + b"\n"))
    return out


# ---- line structure against the two grids ----------------------------------------------------------------------------
def edges() -> List[Case]:
    rng = np.random.default_rng(102)
    out = []
    for p in EDGES:
        head = b">first\n" + fill_lines(rng, p - 7)            # the next line starts at file offset p
        for name, nxt in (("seq", b"ACGTTGCA\n"), ("hdr", b">again\nAC\n"), ("end", b"")):
            out.append((f"gt@{p}+{name}", head + b">x y\n" + acgt(rng, 9) + b"\n" + nxt))
        hdr = b">" + b"h" * (p - 13) + b"\n"                   # its newline sits at file offset p
        for name, nxt in (("seq", b"ACGTTGCA\nAC\n"), ("hdr", b">again\nAC\n"), ("blank", b"\n\nAC\n"), ("end", b"")):
            out.append((f"hdr-nl@{p}+{name}", b">first\nACGT\n" + hdr + nxt))
        out.append((f"seq-nl@{p}", b">s\n" + acgt(rng, p - 3) + b"\n" + acgt(rng, 5) + b"\n>t\n" + acgt(rng, 3)))
    return out


# ---- tiles with no line start: kPass travels over two whole tiles ----------------------------------------------------
def long_lines() -> List[Case]:
    rng = np.random.default_rng(103)
    start, span = 9000, 5 * TILE // 2   # the long line covers tiles 1 and 2; the line behind it starts in chunk 12 of tile 3
    assert start < TILE and (start + span + 1) // TILE == 3 and (start + span + 1) % TILE >= CHUNK
    head = b">p\n" + fill_lines(rng, start - 3)
    seq, hdr = acgt(rng, span), b">" + rng.choice(np.frombuffer(b"hdr >ACGT\t", np.uint8), size=span - 1).tobytes()
    tails = (b"\n" + acgt(rng, 30) + b"\n>n\n" + acgt(rng, 10) + b"\n", b"\n>n\n" + acgt(rng, 10) + b"\n", b"\n", b"")
    out = []
    for i, tail in enumerate(tails):
        out.append((f"long-seq+{i}", head + seq + tail))
        out.append((f"long-hdr+{i}", head + hdr + tail))
    out.append(("long-both", head + seq + b"\n" + hdr + b"\n" + acgt(rng, 3 * TILE) + b"\n" + hdr + b"\n" + seq))
    out.append(("one-header-only", hdr))
    out.append(("one-line-record", b">r\n" + seq + seq))
    return out


# ---- dense chunks --------------------------------------------------------------------------------------------------
def dense() -> List[Case]:
    return [
        ("64-newlines-in-a-chunk", b">d\n" + b"A" * 61 + b"\n" * 64 + b"ACGT\n"),
        ("64-newlines-then-header", b">d\n" + b"A" * 61 + b"\n" * 64 + b">h\nACGT\n"),
        ("newlines-across-chunks", b">d\n" + b"\n" * 300 + b"AC" + b"\n" * 77 + b">e" + b"\n" * 130),
        ("nl-gt-patterns", b">\n" + b"\n>\n>\nA\n>\n" * 60),
        ("gt-gt-nl", b">>\n>>>\nA>\n>A>\n" * 40),
        ("empty-records", b">\n" * 200),
        ("empty-records-named", b">a b\n" * 70 + b"ACGT\n"),
        ("blank-lines", b">a\n\n\nAC\n\nGT\n\n>b\n\n" * 30 + b">c\n\n\n"),
        ("one-base-lines", b">a\n" + b"A\nC\nG\nT\n" * 100),
    ]


# ---- the byte alphabet ---------------------------------------------------------------------------------------------
def alphabet() -> List[Case]:
    every = bytes(b for b in range(256) if b != 0x0A)
    rev = every[::-1]                               # (starts with 0xFF: no '@', '+' or '>' in first position)
    return [
        ("all-bytes-in-a-sequence-line", b">all\nA" + every + b"\n" + rev + b"\nACGT\n"),
        ("all-bytes-in-a-header-line", b">" + every + b"\n" + b"ACGT\n>" + rev + b"\nAC\n"),
        ("all-bytes-unaligned", b">u\n" + b"".join(b"A" * i + every + b"\n" for i in range(1, 18))),
        ("gt-in-mid-line", b">x\nAC>GT\n>y>z\nA>\n"),
        ("gt-after-cr", b">x\nAC\r>GT\n\r>AC\n>y\r\n\r>\r\n"),
        ("crlf", (b">r one\r\n" + b"ACGTACGTAC\r\n" * 7 + b"\r\n") * 40),
        ("lone-cr", b">x\r\nAC\rGT\r\n\r\n>y\r\n\r\r\nA\r"),
        ("blanks-tabs-del-nul-high", b">b\nAC GT\tAC\x7fGT\x00AC\x80GT\xffAC\x1f\x20\x21\n" * 9),
    ]


# ---- file ends -----------------------------------------------------------------------------------------------------
def ends() -> List[Case]:
    rng = np.random.default_rng(106)
    body = b">a x\n" + fill_lines(rng, 500) + b">b\n" + fill_lines(rng, 300)
    return [
        ("ends-in-sequence-without-newline", body + acgt(rng, 33)),
        ("ends-in-header-without-newline", body + b">dangling header"),
        ("ends-in-lone-gt", body + b">"),
        ("ends-in-three-newlines", body + b"\n\n\n"),
        ("ends-in-header-and-newlines", body + b">last\n\n\n"),
    ]


# ---- many tiles: per = 1, 2, 3 tiles per thread of the offsets pass -----------------------------------------------
def tiled_file(seed: int, n: int) -> bytes:
    """n bytes: records of 60-to-80-column lines under headers of random length, some of them longer than a tile, so that
    the state a tile starts in varies and several tiles start inside a header"""
    rng = np.random.default_rng(seed)
    a = rng.choice(ACGT, size=n)
    widths = rng.integers(60, 81, size=n // 60 + 2)
    nl = np.cumsum(widths + 1) - 1
    nl = nl[nl < n - 1]
    a[nl] = 0x0A
    starts = np.concatenate(([0], nl + 1))                      # first byte of every line
    hdr = starts[rng.random(starts.size) < 0.01]
    hdr[0] = 0                                                  # the file starts with a header
    a[hdr] = 0x3E
    text = np.frombuffer(b"contig_ >@+\tx", np.uint8)
    for h in hdr[1::7]:                                         # some headers with text in them ...
        e = min(n, int(h) + 1 + int(rng.integers(1, 60)))
        seg = a[h + 1:e]
        seg[seg != 0x0A] = rng.choice(text, size=int((seg != 0x0A).sum()))
    for h in hdr[3::11]:                                        # ... and some that swallow the lines behind them
        e = min(n - 1, int(h) + int(rng.integers(100, 3 * TILE)))
        seg = a[h + 1:e]
        seg[seg == 0x0A] = 0x68
    if n % TILE == 1:                                           # the last tile's one byte: a base on a line of its own
        a[n - 2:] = (0x0A, 0x41)
    else:
        a[n - 1] = 0x0A
    return a.tobytes()


MANY_TILES = {1024: 1024 * TILE, 1025: 1024 * TILE + 1, 2049: 2048 * TILE + 777}   # tiles: bytes


def many_tiles(ntiles: int) -> List[Case]:
    n = MANY_TILES[ntiles]
    assert (n + TILE - 1) // TILE == ntiles
    return [(f"{ntiles}-tiles", tiled_file(ntiles, n))]


# ---- many records: the inline copy of the record list (4 096) and its first capacity (65 536) ---------------------------
def record_file(seed: int, nrec: int, lo: int = 0, hi: int = 3) -> bytes:
    """nrec records `>\\nSEQ\\n` with sequences of lo..hi bases (an empty one has no line at all)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=nrec)
    seq = acgt(rng, int(lens.sum()))
    out, p = [], 0
    for L in lens.tolist():
        out.append(b">\n" + seq[p:p + L] + b"\n" if L else b">\n")
        p += L
    return b"".join(out)


MANY_RECORDS = (SEPS_INLINE - 1, SEPS_INLINE, SEPS_INLINE + 1, SEPS_CAP, SEPS_CAP + 1, 200_000)


def many_records(nrec: int) -> List[Case]:
    return [(f"{nrec}-records", record_file(nrec, nrec))]


# ---- FASTQ syntax: '@' or '+' first on a line is not for the device; anywhere else it is a byte like any other -----------
def fastq() -> List[Case]:
    rng = np.random.default_rng(109)
    out = []
    for c in (b"@", b"+"):
        for p in (CHUNK, TILE):
            out.append((f"{c.decode()}-line@{p}", b">f\n" + fill_lines(rng, p - 3) + c + b"x\nACGT\n"))
            out.append((f"{c.decode()}-mid-line@{p}", b">f\n" + acgt(rng, p - 3) + c + b"ACGT\n>g" + c + b"\nAC\n"))
        out.append((f"{c.decode()}-line@n-1", b">f\n" + fill_lines(rng, 200) + c))
        out.append((f"{c.decode()}-mid-line@n-1", b">f\n" + acgt(rng, 200) + c))
        out.append((f"{c.decode()}-after-header", b">f\n" + c + b"\nACGT\n"))
        out.append((f"{c.decode()}-first-byte", c + b"f\nACGT\n"))
    out.append(("both-mid-line", b">f\nAC@GT+AC\n>h@+\nAC\n \t@\n\r+\n"))
    out.append(("four-line-fastq", b">r\nACGT\n+\nIIII\n"))
    out.append(("starts-with-newline", b"\n>a\nACGT\n"))
    out.append(("starts-with-sequence", b"ACGT\n>a\nACGT\n"))
    return out


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------
STRUCTURAL = np.frombuffer(b"\n\n\n>\r \t\x7f\x00\x80ACGTacgtN", np.uint8)


def fuzz(count: int = 300) -> List[Case]:
    """files of up to three tiles that begin with '>': bytes of the structural alphabet, thinned with plain bases in
    three files of four so that lines longer than a chunk and chunks without any structure occur as well"""
    rng = np.random.default_rng(110)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 3 * TILE + 1)) if i % 3 else int(rng.integers(1, 400))
        a = rng.choice(STRUCTURAL, size=n)
        share = (1.0, 0.3, 0.05, 0.01)[i % 4]
        if share < 1.0:
            plain = rng.random(n) >= share
            a[plain] = rng.choice(ACGT, size=int(plain.sum()))
        a[0] = 0x3E
        out.append((f"fuzz-{i}", a.tobytes()))
    return out


def foreign(n: int = 8 * TILE) -> bytes:
    """line structure and nothing else: what a buffer should hold before the small cases reuse it (itself a plain FASTA of
    header lines `>@+`)"""
    return (b">@+\n" * (n // 4 + 1))[:n]


# Every group of the list, in an order that keeps the large files behind the small ones.  The emulator runs all of them;
# the GPU tests leave 2049 tiles to the emulator when it alone would take longer than all the others together.
GROUPS: Dict[str, Callable[[], List[Case]]] = {
    "tiny": tiny, "edges": edges, "long_lines": long_lines, "dense": dense, "alphabet": alphabet, "ends": ends,
    "fastq": fastq, "fuzz": fuzz,
    **{f"records_{r}": (lambda r=r: many_records(r)) for r in MANY_RECORDS},
    **{f"tiles_{t}": (lambda t=t: many_tiles(t)) for t in MANY_TILES},
}

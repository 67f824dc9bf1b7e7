"""CPU emulation of the FASTQ record check (auriclass_amd/csrc/mhx_fqcheck.h, the very functions mhx_fqcheck.hip
runs): its verdict against a plain statement of the rule on seeded damaged files, and end to end with the sketch
kernel's tile emulator: whatever the check and the layout check let through is sketched as the oracle sketches it."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import synth
from oracle import mash_oracle as mo
from tests import emul_build
from tests.test_tile_emulation import MAXT, run_emul

BLANKS = bytes(range(0x21)) + b"\x7f"   # what the kseq reader drops
SPECIAL = np.frombuffer(b"\n\n\n@+>\r ANacgt" + b" \t\r\x7f\x00", np.uint8)


@pytest.fixture(scope="module")
def tile_emul():
    L = emul_build.load("tile_emul")
    L.emul_sketch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                              ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def fq():
    L = emul_build.load("fqcheck_emul")
    L.emul_fqcheck.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    L.emul_fqcheck.restype = ctypes.c_int
    return L


def check_flags(L, data: bytes, lead: int = 0) -> bool:
    """True when the emulated device check raises kFlagBadFastq on `data`, placed `lead` bytes into a 16-byte aligned
    buffer that is readable up to the next 16-byte boundary (and no further: the rest is foreign bytes)."""
    raw = np.zeros(lead + len(data) + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    buf = raw[off:]
    buf[:lead] = np.frombuffer((b"@+\nAC \r" * (lead // 7 + 1))[:lead], np.uint8)
    buf[lead:lead + len(data)] = np.frombuffer(data, np.uint8)
    buf[lead + len(data):lead + len(data) + 32] = np.frombuffer(b"\n @+ACGT" * 4, np.uint8)
    return bool(L.emul_fqcheck(buf.ctypes.data, lead, lead + len(data)))


def rule_flags(data: bytes) -> bool:
    """The rule, read off oracle/mashcore.c:mo_sketch_add_fastx, over the lines in fours (line 0 = a header): a record
    fails when (a) its sequence line holds a blank other than one '\\r' at its end, (b) its sequence line begins with
    '>', '@' or '+', or (c) its quality line holds another count of non-blank bytes than its sequence line.  A record
    cut short counts its missing lines as empty (the device check flags a span that ends with unbalanced bases)."""
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    for r in range(0, len(lines), 4):
        rec = lines[r:r + 4] + [b""] * 4
        seq, qual = rec[1], rec[3]
        body = seq[:-1] if seq.endswith(b"\r") else seq
        if len(body.translate(None, BLANKS)) != len(body):
            return True
        if seq[:1] in (b">", b"@", b"+"):
            return True
        if len(seq.translate(None, BLANKS)) != len(qual.translate(None, BLANKS)):
            return True
    return False


def damage(rng, base: bytes, nops: int) -> bytes:
    """tools' old damage generator: replace a byte, delete 1..40 bytes, or insert 1..5 bytes of a set that holds line
    structure, blanks and non-ACGT bytes"""
    b = bytearray(base)
    for _ in range(nops):
        pos = int(rng.integers(0, len(b)))
        op = int(rng.integers(0, 3))
        if op == 0:
            b[pos] = int(rng.choice(SPECIAL))
        elif op == 1:
            del b[pos:pos + int(rng.integers(1, 40))]
        else:
            b[pos:pos] = bytes(rng.choice(SPECIAL, size=int(rng.integers(1, 6))))
    return bytes(b)


def oracle_outcome(data: bytes, k: int):
    sk = mo.Sketcher(k, 1 << 24)
    try:
        sk.add_fastx(data)
    except ValueError:
        return None
    return sk.finish()[0]


@pytest.fixture(scope="module")
def base_fastq():
    genome = synth.make_genome(20000, seed=5)
    return synth.make_fastq(genome, 300, 80, seed=6, device="cpu").numpy().tobytes()


def test_rule_statement_on_damaged_files(fq, base_fastq):
    """Device check == the rule, exactly (neither more nor less), on 3000 seeded damaged files, at unaligned starts."""
    rng = np.random.default_rng(11)
    flagged = 0
    for trial in range(3000):
        data = damage(rng, base_fastq, int(rng.integers(1, 5)))
        lead = int(rng.integers(0, 16)) if trial % 3 else 0
        want = rule_flags(data)
        assert check_flags(fq, data, lead) == want, (trial, lead)
        flagged += want
    assert 300 < flagged < 2900
    assert not check_flags(fq, base_fastq)


def test_passed_files_sketch_as_the_oracle_does(fq, tile_emul, base_fastq):
    """End to end on the CPU: a damaged file that passes the record check and the sketch kernel's layout check is
    accepted by the oracle, and the tile emulator's window hashes are the oracle's."""
    rng = np.random.default_rng(12)
    passed = 0
    for trial in range(1500):
        data = damage(rng, base_fastq, int(rng.integers(1, 5)))
        if check_flags(fq, data):
            continue
        got, stats = run_emul(tile_emul, data, 21, fmt=1, T=MAXT)
        if int(stats[3]) & 2:   # kFlagBadFastq of the layout check
            continue
        want = oracle_outcome(data, 21)
        assert want is not None, trial
        assert np.array_equal(np.unique(got), want), trial
        passed += 1
    assert passed > 60


def record(i, seq, qual, eol=b"\n", plus=b"+"):
    return b"@r%d x" % i + eol + seq + eol + plus + eol + qual + eol


def reads_file(rng, n, lo, hi, eol=b"\n"):
    out = []
    for i in range(n):
        s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(lo, hi + 1))))
        out.append(record(i, s, b"I" * len(s), eol))
    return b"".join(out)


def test_six_reads_blank_inside_a_sequence_is_flagged(fq, tile_emul):
    """Strict 4-line file, one sequence line with a space after base 30, its quality as long as its bases: the
    oracle joins the bases on either side (240 windows), the tile code breaks the run (220): the check must flag it."""
    rng = np.random.default_rng(21)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=60)) for _ in range(6)]
    recs = [record(i, s, b"I" * 60) for i, s in enumerate(seqs)]
    for blank in (b" ", b"\t", b"\x7f", b"\x00", b"\r"):
        bad = seqs[3][:30] + blank + seqs[3][30:]
        data = b"".join(recs[:3]) + record(3, bad, b"I" * 60) + b"".join(recs[4:])
        assert check_flags(fq, data), blank
        assert oracle_outcome(data, 21) is not None       # the oracle sketches it ...
        got, stats = run_emul(tile_emul, data, 21, fmt=1)
        assert int(stats[3]) & 2 == 0                    # ... the layout check has nothing to say ...
        assert len(got) < 6 * 40                         # ... and the device would sketch it differently
    assert not check_flags(fq, b"".join(recs))


KINDS = ("short", "long", "qual_blank", "seq_blank", "seq_gt", "seq_at", "seq_plus")


def damaged_record(kind, i, s):
    q = b"I" * len(s)
    return {
        "short": record(i, s, q[:-1]), "long": record(i, s, q + b"I"), "qual_blank": record(i, s, q[:5] + b" " + q[6:]),
        "seq_blank": record(i, s[:7] + b"\t" + s[7:], q), "seq_gt": record(i, b">" + s[1:], q),
        "seq_at": record(i, b"@" + s[1:], q), "seq_plus": record(i, b"+" + s[1:], q),
    }[kind]


@pytest.mark.parametrize("border", [16384, 32768, 131072, 262144])
def test_damage_at_tile_and_block_borders(fq, border):
    """Damage a record that straddles (or starts or ends at) a 16 KiB tile, 32 KiB step or 128 KiB workgroup border."""
    rng = np.random.default_rng(border)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(50, 200)))) for _ in range(4000)]
    clean = [record(i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    starts = np.cumsum([0] + [len(r) for r in clean])
    assert not check_flags(fq, b"".join(clean))
    j = int(np.searchsorted(starts, border, side="right")) - 1   # the record that holds the border byte
    for shift in (-1, 0, 1):
        for kind in KINDS:
            recs = list(clean)
            recs[j + shift] = damaged_record(kind, j + shift, seqs[j + shift])
            data = b"".join(recs)
            assert check_flags(fq, data), (kind, shift)
            assert rule_flags(data)


def test_long_reads_crlf_empty_reads_no_final_newline(fq):
    rng = np.random.default_rng(31)
    long_reads = reads_file(rng, 6, 30000, 70000)            # lines longer than a step and a workgroup's tile
    assert not check_flags(fq, long_reads) and not check_flags(fq, long_reads[:-1], lead=5)
    lines = long_reads.split(b"\n")
    lines[11] = lines[11][:-1]                               # one quality line a byte short, far from any border
    assert check_flags(fq, b"\n".join(lines))
    lines = long_reads.split(b"\n")
    lines[9] = lines[9][:20000] + b" " + lines[9][20000:]     # a blank deep inside a 30-70 kb sequence line
    lines[11] += b"I"
    assert check_flags(fq, b"\n".join(lines))
    crlf = reads_file(rng, 500, 1, 300, eol=b"\r\n")
    assert not check_flags(fq, crlf) and not check_flags(fq, crlf[:-1]) and not check_flags(fq, crlf[:-2], lead=9)
    assert check_flags(fq, crlf.replace(b"\r\n+", b"\r\r\n+", 1))      # two CRs end a sequence line
    empty = b"".join(record(i, b"", b"") for i in range(100)) + reads_file(rng, 50, 0, 3)
    assert not check_flags(fq, empty) and not check_flags(fq, empty[:-1])
    assert check_flags(fq, empty.replace(b"+\n\n", b"+\nI\n", 1))     # an empty read with a quality byte
    assert not check_flags(fq, empty.replace(b"+\n\n", b"+\n \t\n", 1))  # ... blanks only: kseq counts none
    # a span cut inside a record: the bases it holds are not balanced
    assert check_flags(fq, crlf[:len(crlf) // 2]) == rule_flags(crlf[:len(crlf) // 2])
    for lead in (0, 1, 7, 15, 16, 33, 4099):
        assert not check_flags(fq, long_reads, lead=lead)
        assert check_flags(fq, crlf.replace(b"I\r\n@", b"\r\n@", 1), lead=lead)


def test_span_beyond_one_summary_per_lane_of_the_final_join(fq):
    """A 72 MiB span: more workgroup summaries (256 KiB each) than the final kernel has lanes, so each lane joins a run
    of them; damage late in the span, inside a lane's run and at its end, is still found."""
    L = 150
    rb = synth.record_bytes(L)
    n = (72 << 20) // rb
    genome = synth.make_genome(2_000_000, seed=13)
    clean = synth.make_fastq(genome, n, L, seed=14, device="cpu").numpy().tobytes()
    assert len(clean) > 256 * (256 << 10)
    assert not check_flags(fq, clean) and not check_flags(fq, clean, lead=9)
    for rec in (n - 1, n - 2000, (n * 7) // 8 + 3):
        q = rec * rb + 14 + L
        x = rec * rb + 40                        # inside the sequence line
        for data in (clean[:q] + clean[q + 1:], clean[:x] + b" " + clean[x:]):   # a quality byte short; a blank
            assert check_flags(fq, data), rec

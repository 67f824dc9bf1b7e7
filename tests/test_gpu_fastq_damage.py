"""Damaged FASTQ through every file-level route: the engine (`mash sketch -r`) and the oracle give the same outcome --
both refuse, or the same hashes, comment, length and `Estimated genome size` line.  A file whose records the kseq
reader reads differently from the device parser must be caught by the record check (mhx_fqcheck.hip) and go to the
host record parser; a clean file must keep the device path (engine.last_fastq_route)."""
import gzip

import numpy as np
import pytest

from auriclass_amd import engine, synth
from oracle import mash_oracle as mo

pytestmark = pytest.mark.gpu

SPECIAL = np.frombuffer(b"\n\n\n@+>\r ANacgt" + b" \t\r\x7f\x00", np.uint8)
DEVICE = ("device-streamed", "device-whole")


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.build()
    engine.init(0)


def outcomes(paths, tmp_path, k=21, s=200, m=1):
    """(engine outcome, oracle outcome, route the engine took)"""
    out = tmp_path / "e.msh"
    try:
        err, _ = engine.sketch_files(paths, k, s, out, reads=True, min_mult=m)
        r = mo.read_msh(out).references[0]
        size = [x for x in err.splitlines() if x.startswith("Estimated genome size")]
        e = ("ok", r.hashes.tobytes(), r.comment, r.length, size)
    except engine.EngineError:
        e = ("refuse",)
    route = engine.last_fastq_route()
    try:
        sk, err = mo.sketch_files(paths, k, s, reads=True, m=m)
        r = sk.references[0]
        size = [x for x in err.splitlines() if x.startswith("Estimated genome size")]
        o = ("ok", r.hashes.tobytes(), r.comment, r.length, size)
    except ValueError:
        o = ("refuse",)
    return e, o, route


def same(paths, tmp_path, **kw):
    e, o, route = outcomes(paths, tmp_path, **kw)
    assert e[0] == o[0], (e[0], o[0], route)
    assert e == o, route
    return o[0] == "ok", route


def damage(rng, base: bytes) -> bytes:
    b = bytearray(base)
    for _ in range(int(rng.integers(1, 5))):
        pos = int(rng.integers(0, len(b)))
        op = int(rng.integers(0, 3))
        if op == 0:
            b[pos] = int(rng.choice(SPECIAL))
        elif op == 1:
            del b[pos:pos + int(rng.integers(1, 40))]
        else:
            b[pos:pos] = bytes(rng.choice(SPECIAL, size=int(rng.integers(1, 6))))
    return bytes(b)


def write(path, data: bytes):
    path.write_bytes(gzip.compress(data, compresslevel=1) if path.name.endswith(".gz") else data)
    return path


@pytest.fixture(scope="module")
def base_fastq():
    genome = synth.make_genome(20000, seed=5)
    return synth.make_fastq(genome, 300, 80, seed=6, device="cpu").numpy().tobytes()


@pytest.mark.parametrize("suffix,trials", [(".fq", 200), (".fq.gz", 50)])
def test_seeded_differential_fuzz(tmp_path, base_fastq, suffix, trials):
    rng = np.random.default_rng(41 if suffix == ".fq" else 42)
    p = tmp_path / ("f" + suffix)
    kinds = {"ok": 0, "refuse": 0}
    for trial in range(trials):
        ok, _ = same([write(p, damage(rng, base_fastq))], tmp_path)
        kinds["ok" if ok else "refuse"] += 1
    assert kinds["ok"] > 0 and kinds["refuse"] > 0, kinds


def test_seeded_fuzz_large_sketch_with_multiplicity(tmp_path):
    genome = synth.make_genome(20000, seed=7)
    base = synth.make_fastq(genome, 2000, 100, seed=8, device="cpu").numpy().tobytes()
    rng = np.random.default_rng(43)
    p = tmp_path / "f.fq"
    for trial in range(8):
        same([write(p, damage(rng, base))], tmp_path, k=27, s=50000, m=3)


def record(i, seq, qual):
    return b"@r%d x\n" % i + seq + b"\n+\n" + qual + b"\n"


KINDS = ("short", "long", "qual_blank", "seq_blank", "seq_gt", "seq_at", "seq_plus")


def damaged_record(kind, i, s):
    q = b"I" * len(s)
    return {
        "short": record(i, s, q[:-1]), "long": record(i, s, q + b"I"), "qual_blank": record(i, s, q[:5] + b" " + q[6:]),
        "seq_blank": record(i, s[:30] + b" " + s[30:], q), "seq_gt": record(i, b">" + s[1:], q),
        "seq_at": record(i, b"@" + s[1:], q), "seq_plus": record(i, b"+" + s[1:], q),
    }[kind]


def reads(rng, n, lo, hi):
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(lo, hi + 1)))) for _ in range(n)]


def test_targeted_damage_first_middle_last_record(tmp_path):
    rng = np.random.default_rng(44)
    seqs = reads(rng, 400, 60, 160)
    clean = [record(i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    p = tmp_path / "t.fq"
    ok, route = same([write(p, b"".join(clean))], tmp_path)
    assert ok and route in DEVICE
    for kind in KINDS:
        for j in (0, 200, 399):
            recs = list(clean)
            recs[j] = damaged_record(kind, j, seqs[j])
            ok, route = same([write(p, b"".join(recs))], tmp_path)
            assert route == "record-parser", (kind, j, route)


ROUTES = {
    "bulk": ({}, ".fq"), "chunked": ({"MHX_NO_BULK": "1"}, ".fq"), "gz_own": ({}, ".fq.gz"),
    "gz_zlib": ({"MHX_ZLIB_INFLATE": "1"}, ".fq.gz"), "whole_file": ({"MHX_NO_STREAMING": "1"}, ".fq"),
    "whole_file_gz": ({"MHX_NO_STREAMING": "1"}, ".fq.gz"),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_file_level_route(tmp_path, monkeypatch, route):
    env, suffix = ROUTES[route]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    want_clean = "device-whole" if "MHX_NO_STREAMING" in env else "device-streamed"
    rng = np.random.default_rng(45)
    seqs = reads(rng, 300, 60, 160)
    clean = [record(i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    p1, p2 = tmp_path / ("a" + suffix), tmp_path / ("b" + suffix)
    write(p1, b"".join(clean[:150]))
    ok, r = same([write(p2, b"".join(clean[150:]))], tmp_path)
    assert ok and r == want_clean
    ok, r = same([p1, p2], tmp_path)                         # a clean pair
    assert ok and r == want_clean
    for kind in KINDS:
        recs = list(clean)
        recs[220] = damaged_record(kind, 220, seqs[220])     # in the second file of the pair
        write(p2, b"".join(recs[150:]))
        ok, r = same([p1, p2], tmp_path)
        assert r == "record-parser", (kind, r)
        ok, r = same([write(p1, b"".join(recs[100:]))], tmp_path)
        assert r == "record-parser", (kind, r)
        write(p1, b"".join(clean[:150]))


def test_gz_larger_than_a_chunk_damage_in_the_second_chunk(tmp_path):
    """A .fq.gz of ~42 MB inflated: the ingest cuts its first 32 MiB chunk in front of the last record whose '+' line
    starts inside it (j below), which makes that record the first of the second chunk.  Records j - 1, j and j + 1 lose
    one quality byte in turn, so the first record of the second chunk is among the damaged ones even if the cut moves
    by a record."""
    L = 150
    rb = synth.record_bytes(L)
    n = (40 << 20) // rb
    genome = synth.make_genome(2_000_000, seed=9)
    clean = synth.make_fastq(genome, n, L, seed=10, device="cpu").numpy().tobytes()
    p = tmp_path / "big.fq.gz"
    ok, route = same([write(p, clean)], tmp_path)
    assert ok and route == "device-streamed"
    j = ((32 << 20) - 13 - L) // rb              # the last record with its '+' line inside the first chunk
    assert j * rb < (32 << 20) <= (j + 1) * rb + 12 + L
    for rec in (j - 1, j, j + 1):
        q = rec * rb + 14 + L                    # its quality line
        data = bytearray(clean)
        assert data[q - 2] == ord("+") and data[q + L] == ord("\n")
        del data[q]
        ok, route = same([write(p, bytes(data))], tmp_path)
        assert route == "record-parser" and not ok, rec


def test_long_reads_one_quality_line_short(tmp_path):
    """Reads of 3-60 kb (tiles that take the look-back repair pass): one quality line a byte short."""
    rng = np.random.default_rng(46)
    seqs = reads(rng, 60, 3000, 60000)
    clean = [record(i, s, b"I" * len(s)) for i, s in enumerate(seqs)]
    p = tmp_path / "long.fq"
    ok, route = same([write(p, b"".join(clean))], tmp_path)
    assert ok and route == "device-streamed"
    recs = list(clean)
    recs[31] = damaged_record("short", 31, seqs[31])
    ok, route = same([write(p, b"".join(recs))], tmp_path)
    assert route == "record-parser" and not ok

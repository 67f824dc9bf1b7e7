"""CPU emulation of the device FASTA parser (auriclass_amd/csrc/mhx_fasta.h, the very functions mhx_fasta.hip runs, in
the kernels' order: tests/emul/fasta_emul.cpp) against the plain rule (tests/fasta_rule.py) on the shared case list
(tests/fasta_cases.py): the stream byte for byte, the separator positions, the total and the FASTQ flag."""
import ctypes

import numpy as np
import pytest

from tests import emul_build, fasta_cases
from tests.fasta_rule import has_fastq_line, rule

FOREIGN = np.frombuffer(b"\n>@+" * 16, np.uint8)


@pytest.fixture(scope="module")
def fa():
    L = emul_build.load("fasta_emul")
    L.emul_fasta.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_fasta.restype = ctypes.c_int
    return L


def run_emul(L, data: bytes, want_total: int, want_seps: int):
    """(stream, total, seps as the device leaves them, separator count, FASTQ flag) of `data`, placed in a 16-byte aligned
    buffer that is readable up to the next 16-byte boundary, with foreign line structure directly behind its end"""
    n = len(data)
    raw = np.zeros(n + 64 + 16, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:]
    buf[:n] = np.frombuffer(data, np.uint8)
    buf[n:n + 64] = FOREIGN
    out = np.full(want_total + 64, 0xEE, dtype=np.uint8)          # a stream that is too long runs into the guard, not out
    seps = np.zeros(want_seps + 64, dtype=np.uint64)
    total, nseps, flag = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = L.emul_fasta(buf.ctypes.data, n, out.ctypes.data, out.size, ctypes.byref(total), seps.ctypes.data, seps.size, ctypes.byref(nseps),
                      ctypes.byref(flag))
    assert rc == 0, "kept bytes beyond the room of the rule's stream"
    return out, total.value, seps, nseps.value, bool(flag.value)


def check(L, name: str, data: bytes):
    stream, seps = rule(data)
    out, total, got_seps, nseps, flag = run_emul(L, data, len(stream), len(seps))
    assert total == len(stream), name
    assert out[:total].tobytes() == stream, name
    assert bool(np.all(out[total:] == 0xEE)), name                # nothing written behind the stream
    assert nseps == len(seps) and np.array_equal(np.sort(got_seps[:nseps]), np.array(seps, dtype=np.uint64)), name
    assert flag == has_fastq_line(data), name


@pytest.mark.parametrize("group", list(fasta_cases.GROUPS))
def test_emulated_parser_equals_the_rule(fa, group):
    cases = fasta_cases.GROUPS[group]()
    assert cases
    for name, data in cases:
        check(fa, name, data)


def test_the_case_list_covers_what_it_says():
    """the shapes the list is there for, checked on the list itself"""
    T = fasta_cases.TILE
    sizes = {t: len(fasta_cases.many_tiles(t)[0][1]) for t in (1024, 1025)}
    assert [(n + T - 1) // T for n in sizes.values()] == [1024, 1025]
    assert (fasta_cases.MANY_TILES[2049] + T - 1) // T == 2049 and fasta_cases.MANY_TILES[2049] > 33_500_000
    data = fasta_cases.many_tiles(1025)[0][1]
    a = np.frombuffer(data, np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(a[:-1] == 0x0A) + 1))
    hdr = starts[a[starts] == 0x3E]
    # some tiles start inside a header line, some inside a sequence line, and some hold no line start at all
    line_of_tile = np.searchsorted(starts, np.arange(1, 1025) * T, side="right") - 1
    in_header = a[starts[line_of_tile]] == 0x3E
    assert 20 < int(in_header.sum()) < 1000 and hdr.size > 1000
    no_start = np.diff(np.searchsorted(starts, np.arange(0, 1026) * T)) == 0
    assert int(no_start.sum()) >= 5
    for nrec in fasta_cases.MANY_RECORDS:
        assert fasta_cases.many_records(nrec)[0][1].count(b">") == nrec
    assert not has_fastq_line(fasta_cases.foreign()) and fasta_cases.foreign()[:1] == b">"
    assert all(d[:1] == b">" and not has_fastq_line(d) for _, d in fasta_cases.fuzz(40))

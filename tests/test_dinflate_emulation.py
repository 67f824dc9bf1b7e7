"""CPU emulation of the device gzip decoder (auriclass_amd/csrc/mhx_dinflate.h, the very functions and round driver the
HIP kernels run) against Python's zlib: search, symbolic decode, chain check and redo, resolution and CRC-32, lane by lane."""
import ctypes
import gzip
import zlib

import numpy as np
import pytest

from auriclass_amd import synth
from tests import emul_build


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("dinflate_emul", libs=("-lz",))
    L.emul_gunzip.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                              ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    return L


def run(L, gz: bytes, seg: int, round_segs: int = 1 << 20, cap: int = 0):
    cap = cap or 64 * len(gz) + (1 << 20)
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64(0)
    stats = np.zeros(8, dtype=np.uint64)
    rc = L.emul_gunzip(gz, len(gz), seg, round_segs, out, cap, ctypes.byref(n), stats.ctypes.data)
    return rc, out.raw[:min(n.value, cap)], n.value, stats


def gz_member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    parts = []
    for i in range(0, len(data), flush_every):
        parts.append(c.compress(data[i:i + flush_every]))
        parts.append(c.flush(zlib.Z_SYNC_FLUSH if (i // flush_every) % 2 == 0 else zlib.Z_FULL_FLUSH))
    parts.append(c.flush())
    return b"".join(parts)


@pytest.fixture(scope="module")
def fastq():
    genome = synth.make_genome(400_000, seed=5)
    return synth.make_fastq(genome, 12_000, 150, seed=6, device="cpu").numpy().tobytes()


def check(L, data, gz, seg, **kw):
    rc, got, n, stats = run(L, gz, seg, cap=len(data) + 16, **kw)
    assert rc == 0, f"device path failed on a valid stream (stats {stats})"
    assert n == len(data) and got == data
    return stats


@pytest.mark.parametrize("level", [1, 6, 9])
def test_fastq_levels(emul, fastq, level):
    gz = gz_member(fastq, level)
    stats = check(emul, fastq, gz, 16 << 10)
    assert stats[0] == 1 and stats[1] > 4


@pytest.mark.parametrize("strategy", [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
def test_strategies(emul, fastq, strategy):
    check(emul, fastq, gz_member(fastq, 6, strategy), 16 << 10)


def test_sync_flushes_and_stored_blocks(emul, fastq):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    data = fastq[:500_000] + noise + fastq[500_000:]
    check(emul, data, gz_member(data, 6, flush_every=37_000), 8 << 10)
    check(emul, data, gz_member(data, 0), 8 << 10)  # level 0: stored blocks only


def test_all_n_reads(emul):
    recs = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"N" * 150, b"#" * 150) for i in range(20_000))
    stats = check(emul, recs, gz_member(recs, 6), 1 << 10)
    assert stats[1] > 1


def test_random_binary(emul):
    data = np.random.default_rng(9).integers(0, 256, 600_000, dtype=np.uint8).tobytes()
    check(emul, data, gz_member(data, 9), 16 << 10)


def test_tiny_segments_force_redo(emul, fastq):
    """Targets a few hundred bytes apart: many land in blocks (false candidates, or none at all); the chain check redoes them."""
    for level, seg in ((1, 300), (6, 512), (9, 1000)):
        check(emul, fastq, gz_member(fastq, level), seg)
    # stored blocks whose payload is itself a DEFLATE stream: valid dynamic headers inside blocks, false starts for sure
    inner = b"".join(zlib.compress(fastq[i:i + 40_000], 6)[2:] for i in range(0, 600_000, 40_000))
    data = inner + fastq[:300_000]
    st = check(emul, data, gz_member(data, 0) , 2000)
    assert st[2] > 0
    mixed = gz_member(data, 6, flush_every=50_000)
    check(emul, data, mixed, 700)


def test_rounds(emul, fastq):
    """Few segments per round: every round starts where the previous one verifiably stopped, markers read its output."""
    for rs in (1, 2, 3, 7):
        check(emul, fastq, gz_member(fastq, 6), 4 << 10, round_segs=rs)


def test_small_slabs_grow(emul):
    """Highly compressible data: the symbol slabs overflow, the counts stay exact and the round is decoded again."""
    data = b"A" * 3_000_000 + b"C" * 10
    check(emul, data, gz_member(data, 9), 1 << 10)


def test_members_and_trailing_garbage(emul, fastq):
    a, b = fastq[:700_000], fastq[700_000:]
    both = gz_member(a, 6) + gz_member(b, 1)
    st = check(emul, fastq, both, 16 << 10)
    assert st[0] == 2
    check(emul, fastq, both + b"trailing garbage that is not gzip", 16 << 10)
    check(emul, fastq, gzip.compress(fastq, mtime=0), 16 << 10)  # gzip module header (FNAME absent, mtime 0)


def test_empty_member(emul):
    check(emul, b"", gz_member(b"", 6), 16 << 10)


def test_truncated_and_flipped_never_succeed_with_other_bytes(emul, fastq):
    gz = gz_member(fastq, 6)
    rng = np.random.default_rng(11)
    for cut in (len(gz) - 1, len(gz) - 5, len(gz) - 9, len(gz) // 2, 30):
        rc, got, n, _ = run(emul, gz[:cut], 8 << 10)
        assert rc != 0
    for _ in range(25):
        b = bytearray(gz)
        pos = int(rng.integers(20, len(gz) - 8))
        b[pos] ^= 1 << int(rng.integers(0, 8))
        rc, got, n, _ = run(emul, bytes(b), 8 << 10)
        if rc == 0:  # a flip that leaves the stream valid must decode to what zlib says
            assert got == zlib.decompress(bytes(b), 31)

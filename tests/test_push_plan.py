"""The schedule of a sketcher push on the CPU: tests/emul/push_plan_emul.cpp steps through auriclass_amd/csrc/mhx_push_plan.h
-- the header push_span itself steps through -- and returns every launch as a row.  Against the independent statement of
tests/push_rule.py over a grid, and against the invariants that the comments of the schedule claim."""
import ctypes
import itertools
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import emul_build
from tests import push_rule as pr

TILE = pr.TILE
COLS = ("push", "tile0", "ntiles", "split", "queue", "cap_before", "next_cap", "verify", "bytes", "chunk", "push_tiles")
S = (64, 1000, 8192, 50000)
M = (1, 2, 3, 4, 5, 9)
NSLOTS = (1 << 16, 1 << 21, 1 << 24, 1 << 30)
HASH_MAX = (0xFFFFFFFF, 2 ** 64 - 1)             # k <= 16, k > 16
FORMS = ((0, 0), (1, 0), (2, 0), (1, 1))          # (kernel format, repair): a repair pass runs format 1, the only form settle() and finish() start one in
CUS = (1, 256)
SPAN_TILES = (1, 31, 32, 33, 64, 65, 70)
GB3 = 3_000_000_000


@pytest.fixture(scope="module")
def emul():
    L = emul_build.load("push_plan_emul")
    u32, u64, vp, i = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int
    L.emul_push_constant.argtypes = [i]
    L.emul_push_constant.restype = u64
    L.emul_first_chunk.argtypes = [u32, u32, u64]
    L.emul_first_chunk.restype = u64
    L.emul_queue_form.argtypes = [i, u32, u64, u64, i]
    L.emul_queue_form.restype = u32
    L.emul_push_rows.argtypes = [u32, u32, u64, u64, u64, i, vp, vp, vp, vp, u64, i, u32, vp, vp, u64]
    L.emul_push_rows.restype = ctypes.c_int64
    assert L.emul_push_constant(5) == len(COLS)
    return L


def span_bytes(tiles, begin):
    """a span that ends inside tile number `tiles`, counted from the aligned base"""
    return tiles * TILE - 100 - begin


def planned(L, sk, pushes, cu, counters=None, force_queue=None, force_split=0):
    """rows (one per launch, COLS) of the pushes [(kfmt, repair, begin, n)] on a sketcher (s, m, nslots, hash_max, scale);
    counters: [bytes, chunk, repair_bytes, repair_chunk], updated in place (default: a fresh sketcher's)"""
    s, m, nslots, hash_max, scale = sk
    if counters is None:
        counters = np.array([0, L.emul_first_chunk(s, m, nslots)] * 2, np.uint64)
    kfmt = np.array([p[0] for p in pushes], np.int32)
    rep = np.array([p[1] for p in pushes], np.int32)
    begin = np.array([p[2] for p in pushes], np.uint64)
    n = np.array([p[3] for p in pushes], np.uint64)
    cap_rows = len(pushes) + 64 * min(len(pushes), 64) + 64
    rows = np.zeros((cap_rows, len(COLS)), np.uint64)
    got = L.emul_push_rows(s, m, nslots, hash_max, scale, cu, kfmt.ctypes.data, rep.ctypes.data, begin.ctypes.data, n.ctypes.data, len(pushes),
                           -1 if force_queue is None else force_queue, force_split, counters.ctypes.data, rows.ctypes.data, cap_rows)
    assert got >= 0
    return rows[:got]


def ruled(sk, pushes, cu, force_queue=None, force_split=0):
    s, m, nslots = sk[:3]
    counters = pr.fresh_counters(s, m, nslots)
    out = []
    for i, (kfmt, rep, begin, n) in enumerate(pushes):
        for st in pr.push(sk, counters, kfmt, rep, begin, n, cu, force_queue, force_split):
            out.append([i, st["tile0"], st["ntiles"], st["split"], st["queue"], st["cap_before"], st["next_cap"], st["verify"], st["bytes"],
                        st["chunk"], pr.tiles_of(begin, n)])
    return np.array(out, np.uint64).reshape(-1, len(COLS))


def sequences(kfmt, rep, spans=SPAN_TILES):
    """(name, pushes): every span whole and in two parts, at begin 0 and off the 16-byte grid"""
    for tiles, begin in itertools.product(spans, (0, 7)):
        n = span_bytes(tiles, begin)
        yield (tiles, begin, "whole"), [(kfmt, rep, begin, n)]
        first = (n * 3 // 5) & ~15          # (the second part begins on the grid again)
        if first:
            yield (tiles, begin, "two"), [(kfmt, rep, begin, first), (kfmt, rep, 0, n - first)]
    yield ("3GB", 15, "whole"), [(kfmt, rep, 15, GB3)]
    yield ("3GB", 0, "two"), [(kfmt, rep, 0, GB3 // 3), (kfmt, rep, 0, GB3 - GB3 // 3)]


def growth(s, nslots):
    return min(max(nslots // (16 * s), int(pr.GROWTH)), 256)


def cap_of(s, m, hash_max, scale, after):
    """the cap as the schedule's comment states it, in exact integer and extended arithmetic of its own"""
    if m <= 1 or after <= (1 << 20):
        return 0
    ld = np.longdouble
    frac = ld(48) * (ld(s) + ld(8) * np.sqrt(ld(s)) + ld(16)) * ld(scale) / ld(after)
    return 0 if frac >= 1 else max(1, int(frac * ld(hash_max)))


def check_invariants(L, rows, sk, pushes, cu, force_queue=None, force_split=0):
    """the pushes of a fresh sketcher"""
    s, m, nslots, hash_max, scale = sk
    ld = np.longdouble
    G = growth(s, nslots)
    chunk_before = {0: L.emul_first_chunk(s, m, nslots), 1: L.emul_first_chunk(s, m, nslots)}      # main, repair
    seen = {0: 0, 1: 0}
    for i, (kfmt, rep, begin, n) in enumerate(pushes):
        r = rows[rows[:, 0] == i].tolist()
        ntiles = pr.tiles_of(begin, n)
        before_push = seen[rep]
        # every tile exactly once, in order, in at most 64 launches; the last takes the rest
        assert 1 <= len(r) <= pr.MAX_LAUNCHES
        assert r[0][1] == 0 and all(r[j][1] == r[j - 1][1] + r[j - 1][2] for j in range(1, len(r)))
        assert r[-1][1] + r[-1][2] == ntiles and all(x[2] >= 1 for x in r)
        for j, x in enumerate(r):
            _, tile0, take, split, queue, cap_before, next_cap, verify, after, chunk, _ = x
            last = j == len(r) - 1
            before = seen[rep]
            assert after == before_push + min(n, (tile0 + take) * TILE)    # real bytes, not whole tiles
            own_cap = cap_before if j == 0 else r[j - 1][6]                # a later launch's cap rides with the pass in front of it
            assert j == 0 or cap_before == 0
            assert not last or next_cap == 0
            if m == 1:
                assert own_cap == 0
                if i == 0 and j == 0:
                    assert take * TILE <= max(nslots // 4, TILE)           # the first launch of a fresh sketcher: a quarter of the table
                if j != pr.MAX_LAUNCHES - 1:
                    assert take == min(ntiles - tile0, max(1, chunk_before[rep] // TILE))
                assert chunk == (chunk_before[rep] * G if chunk_before[rep] < 1 << 40 else chunk_before[rep])
            else:
                assert chunk == chunk_before[rep]
                assert own_cap == cap_of(s, m, hash_max, scale, after)      # floor(48 s' scale / after x hash_max), absent at >= 1, never 0
                if after <= 1 << 20:
                    assert own_cap == 0                                    # the first MiB is admitted whole
                if j != pr.MAX_LAUNCHES - 1:
                    assert after <= max(1 << 20, (8 if m <= 3 else 4) * before) + TILE     # growth of the bytes seen, to a tile
            if force_queue is not None:
                assert queue == force_queue
            elif kfmt == 0:
                assert queue == 0
            else:
                rate = min(ld(1), ld(s) / (ld("0.4") * ld(before))) if before else ld(1)
                if own_cap:
                    rate = max(rate, ld(own_cap) / ld(hash_max))
                assert queue == int(rate <= ld("0.1") and (s >= 8192 or rate > ld("3e-4")))
            may_split = before == 0 and j == 0 and kfmt != 1 and not rep and not own_cap and not queue
            if not may_split:
                assert split == 1
            elif force_split:
                assert split == force_split
            else:
                assert split in (1, 2, 4, 8) and (take * split >= cu or split == 8) and (split == 1 or take * (split // 2) < cu)
            # chain check: exactly once, on the last pass, for format 2 or repair with two tiles or more
            assert verify == int(last and (kfmt == 2 or bool(rep)) and ntiles >= 2)
            seen[rep], chunk_before[rep] = after, chunk
        assert seen[rep] == before_push + n


def test_constants_and_first_chunk(emul):
    assert [emul.emul_push_constant(i) for i in range(5)] == [pr.MAX_LAUNCHES, pr.GROWTH, pr.UNCAPPED, pr.DEVICE_ORDER_MIN_SKETCH, TILE]
    for s, m, nslots in itertools.product(S + (1, 16384, 16385, 1_000_000), M, NSLOTS):
        c0 = emul.emul_first_chunk(s, m, nslots)
        assert c0 == pr.first_chunk(s, m, nslots)
        assert c0 <= nslots // 4 and (m == 1 or c0 == min(1 << 20, nslots // 4))


def test_grid_equals_rule_and_keeps_the_invariants(emul):
    launches = 0
    for s, m, nslots, hash_max, cu in itertools.product(S, M, NSLOTS, HASH_MAX, CUS):
        sk = (s, m, nslots, hash_max, 1)
        for kfmt, rep in FORMS:
            for name, pushes in sequences(kfmt, rep):
                rows = planned(emul, sk, pushes, cu)
                assert np.array_equal(rows, ruled(sk, pushes, cu)), (sk, cu, kfmt, rep, name)
                check_invariants(emul, rows, sk, pushes, cu)
                launches += len(rows)
    assert launches > 50_000


def test_overrides_and_retry_budget(emul):
    """a forced kernel form wins everywhere; a forced split only where a split may be; admit_scale (the retry's 16x) scales the cap"""
    for s, m, hash_max, scale in itertools.product((1000, 8192), (1, 3, 5), HASH_MAX, (1, 16)):
        sk = (s, m, 1 << 21, hash_max, scale)
        for (kfmt, rep), (fq, fs) in itertools.product(FORMS, ((0, 0), (1, 0), (None, 1), (None, 2), (None, 4), (None, 8), (0, 8), (1, 8))):
            for name, pushes in sequences(kfmt, rep, (1, 33, 65)):
                rows = planned(emul, sk, pushes, 256, force_queue=fq, force_split=fs)
                assert np.array_equal(rows, ruled(sk, pushes, 256, fq, fs)), (sk, kfmt, rep, fq, fs, name)
                check_invariants(emul, rows, sk, pushes, 256, force_queue=fq, force_split=fs)


TEN_BYTE = [(((1000, m, 1 << 21, 2 ** 64 - 1, 1), 256, (2, 0)), tiles) for m in (1, 3) for tiles in SPAN_TILES] + \
           [(((64, 5, 1 << 16, 0xFFFFFFFF, 1), 1, (0, 0)), 20), (((8192, 2, 1 << 24, 2 ** 64 - 1, 1), 256, (1, 1)), 3)]


@pytest.mark.parametrize("config,tiles", TEN_BYTE, ids=[f"s{c[0][0]}_m{c[0][1]}_fmt{c[2][0]}_{t}tiles" for c, t in TEN_BYTE])
def test_ten_byte_pushes(emul, config, tiles):
    """thousands of tiny pushes: one launch each, the counters advance by real bytes, the stages of m > 1 are defined on them;
    every span of the grid for m = 1 and m = 3 at s = 1000, and two other sketchers (32-bit hashes, a repair pass)"""
    sk, cu, (kfmt, rep) = config
    total = span_bytes(tiles, 0)
    pushes = [(kfmt, rep, off & 15, min(10, total - off)) for off in range(0, total, 10)]
    rows = planned(emul, sk, pushes, cu)
    assert len(rows) == len(pushes) and np.array_equal(rows[:, 0], np.arange(len(pushes), dtype=np.uint64))
    assert np.array_equal(rows, ruled(sk, pushes, cu)), (sk, tiles)
    assert rows[-1, 8] == total
    assert np.all(rows[1:, 3] == 1) and np.all(rows[:, 7] == 0)          # only the very first launch may split; one tile has no chain
    s, m, _, hash_max, scale = sk
    caps = rows[:, 5].astype(object)
    after = rows[:, 8].astype(object)
    assert all(c == cap_of(s, m, hash_max, scale, a) for c, a in zip(caps[::997], after[::997]))
    assert np.all(rows[:, 6] == 0)                                      # one launch per push: every cap is a launch of its own


def test_repair_counters_advance_on_their_own(emul):
    sk = (1000, 3, 1 << 21, 2 ** 64 - 1, 1)
    n = span_bytes(70, 0)
    pushes = [(2, 0, 0, n), (1, 1, 0, n), (2, 0, 0, n), (1, 1, 0, n)]
    rows = planned(emul, sk, pushes, 256)
    assert np.array_equal(rows, ruled(sk, pushes, 256))
    main, rep = rows[np.isin(rows[:, 0], (0, 2))], rows[np.isin(rows[:, 0], (1, 3))]
    assert main[-1, 8] == 2 * n and rep[-1, 8] == 2 * n
    # the repair pass of a span is scheduled as the span was: on counters that have seen what the main ones had
    assert np.array_equal(main[:, 1:3], rep[:, 1:3]) and np.array_equal(main[:, 5:7], rep[:, 5:7])
    assert np.all(rep[:, 3] == 1) and rep[rep[:, 0] == 1][-1, 7] == 1


def test_queue_form_rule(emul):
    """the one rule, as the screen-mode push calls it with T_screen / hash_max"""
    for kfmt, s, (num, den), forced in itertools.product((0, 1, 2), (1000, 8191, 8192), ((0, 1), (1, 10000), (3, 10000), (4, 10000), (1, 10), (1001, 10000), (1, 1)),
                                                         (-1, 0, 1)):
        rate = np.longdouble(num) / np.longdouble(den)
        want = pr.queue_form(kfmt, s, rate, None if forced < 0 else forced)
        assert emul.emul_queue_form(kfmt, s, num, den, forced) == want
        if forced < 0:   # against the rule in exact fractions, away from the two bounds themselves (there the rounding of the quotient decides)
            assert want == int(kfmt != 0 and num * 10 <= den and (s >= 8192 or num * 10000 > 3 * den)) or (num, den) in ((3, 10000), (1, 10))


def test_stepper_under_address_sanitizer(tmp_path):
    """CPU ASan/UBSan build of tests/emul/push_plan_emul.cpp as a program of its own: the 3 GB span and a span in 10-byte pushes"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "push_plan_emul"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-DPUSH_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           str(root / "tests" / "emul" / "push_plan_emul.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime on this host")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=0"), timeout=120)
    assert r.returncode == 0 and r.stdout == "ok 24\n", (r.stdout[-500:], r.stderr[-3000:])

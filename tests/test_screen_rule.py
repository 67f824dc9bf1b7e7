"""CPU-side checks of the containment screen (`mash screen`): the new entry points are exported and declared, refuse to
compute without a GPU engine, and the scalar columns -- identity and the binomial tail -- follow the rule stated in
tests/screen_rule.py (Mash's CommandScreen restated; no mash output is recorded for it)."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from auriclass_amd import engine
from tests import screen_rule as rule

ROOT = Path(__file__).resolve().parent.parent
NEW = ["mhx_screen_files", "mhx_screener_create", "mhx_screener_destroy", "mhx_screener_reset", "mhx_screener_push_device",
       "mhx_screener_push_host", "mhx_screener_sync", "mhx_screener_finish", "mhx_screen_identity", "mhx_screen_p_value"]


@pytest.fixture(scope="module")
def lib():
    engine.build()
    return engine.load()


def test_screen_symbols_are_declared_and_exported(lib):
    declared = engine.declared_symbols()
    for name in NEW:
        assert name in declared, f"include/mhx.h does not declare {name}"
        assert hasattr(lib, name), f"libmhx.so does not export {name}"
    assert callable(engine.screen_files) and hasattr(engine, "Screener")


NO_ENGINE = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
c = ctypes
L.mhx_last_error.restype = c.c_char_p
rows = (c.c_uint64 * 4)(1, 2, 3, 4)
lens = (c.c_uint32 * 1)(4)
h = c.c_void_p()
need = c.c_size_t(0)
size = c.c_double(0)
paths = (c.c_char_p * 1)(b"reads.fq")
out = (c.c_uint32 * 4)()
got = {
    "screen_files": L.mhx_screen_files(b"ref.msh", paths, 1, None, c.c_size_t(0), c.byref(need), c.byref(size)),
    "create": L.mhx_screener_create(21, rows, lens, c.c_uint32(1), c.c_uint32(4), c.c_uint32(4), 1, 0, c.byref(h)),
    "reset": L.mhx_screener_reset(None),
    "push_device": L.mhx_screener_push_device(None, None, c.c_uint64(0), 0),
    "push_host": L.mhx_screener_push_host(None, None, c.c_uint64(0), 0),
    "sync": L.mhx_screener_sync(None),
    "finish": L.mhx_screener_finish(None, out, out, c.byref(size), None),
}
bad = {k: v for k, v in got.items() if v != -1}
assert not bad, bad
assert b"no GPU engine" in L.mhx_last_error()
L.mhx_screener_destroy(None)
print("ok")
"""


def test_screen_entry_points_answer_no_device_without_an_engine(lib):
    # a fresh process that never calls mhx_init: no engine, whatever the machine holds
    r = subprocess.run([sys.executable, "-c", NO_ENGINE, str(engine.LIB_PATH)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_identity_equals_the_definition_bit_for_bit(lib):
    rng = np.random.default_rng(5)
    cases = [(0, 0, 21), (0, 1, 1), (1, 1, 32), (0, 50000, 27), (50000, 50000, 27), (48466, 48476, 27), (1, 1000000, 5)]
    for k in (1, 5, 11, 16, 17, 21, 27, 32):
        for n in (1, 2, 1000, 48476, 50000, 10 ** 6):
            for s in {0, 1, n // 2, max(n - 1, 0), n} | {int(x) for x in rng.integers(0, n + 1, size=6)}:
                cases.append((s, n, k))
    for s, n, k in cases:
        got, want = engine.screen_identity(s, n, k), rule.identity(s, n, k)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (s, n, k, got, want)


def p_grid():
    pts = []
    for k in (11, 16, 21, 27, 32):
        for n in (1, 1000, 50_000, 10 ** 6):
            for size in (1e3, 1e4, 1e5 + 0.75, 1e6, 1e7, 154153.32037587647, 1e8, 1e9, 1e10):
                r = 1.0 / (1.0 + 4.0 ** k / math.floor(size))
                shared = {1, 2, 3, n}
                shared |= {int(n * f) for f in (1e-4, 1e-3, 1e-2, 0.1, 0.25, 0.5, 0.9)}
                for mult in (0.5, 1.0, 2.0, 5.0):
                    for off in (-1, 0, 1, 3):
                        shared.add(int(n * r * mult) + off)
                pts += [(s, n, size, k) for s in sorted(shared) if 1 <= s <= n]
    return pts


def test_p_value_against_binomial_survival_function_on_the_grid(lib):
    """k x n x set size x shared (see p_grid): mhx_screen_p_value against scipy's binom.sf -- at most one apart in the sixth
    significant digit, two values below 1e-300 equal; at least half of the points must carry a value >= 1e-300 on both
    sides."""
    pytest.importorskip("scipy")
    pts = p_grid()
    assert len(pts) > 1500
    informative, worst, misses = 0, 0.0, []
    for s, n, size, k in pts:
        got, want = engine.screen_p_value(s, n, size, k), rule.p_value(s, n, size, k)
        if got >= 1e-300 and want >= 1e-300:
            informative += 1
            worst = max(worst, abs(got - want) / want)
        if not rule.same_to_the_sixth_digit(got, want):
            misses.append((s, n, size, k, got, want))
    print(f"{len(pts)} grid points, {informative} with both values >= 1e-300, worst relative difference {worst:.3g}")
    assert not misses, misses[:10]
    assert 2 * informative >= len(pts)


def test_p_value_special_cases(lib):
    assert engine.screen_p_value(0, 50000, 1e6, 27) == 1.0
    assert engine.screen_p_value(0, 50000, 0.0, 27) == 1.0
    assert engine.screen_p_value(5, 50000, 0.0, 27) == 0.0          # an empty read set cannot share anything
    # the set size enters through its floor (mash keeps it in a uint64_t)
    assert engine.screen_p_value(3, 1000, 123456.99, 11) == engine.screen_p_value(3, 1000, 123456.0, 11)
    assert engine.screen_p_value(3, 1000, 123456.99, 11) != engine.screen_p_value(3, 1000, 123457.0, 11)

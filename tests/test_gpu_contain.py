"""The containment from sketches on the GPU (mhx_dist_contain) against the rule of tests/contain_rule.py, every integer exact:
the pair kernel on the crafted edge cases, the range route at 16, 64 and 1024 value ranges (no block may fall back there, so
the pair kernel alone cannot pass), flagged blocks redone by the pair kernel, a pair without a geometry, MHX_DIST_GENERIC in
a child process, the device-pointer form, and the argument checks."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from tests import contain_cases as cc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(name):
    Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows() if name == "crafted" else cc.rows_of(name)
    return engine.dist_contain(Q, q_len, R, r_len, s_q, s_r)


def check(got, want, what=""):
    for name, a, b in zip(("shared", "n_qry", "n_ref"), got, want):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def test_pair_kernel_on_the_crafted_edge_cases(lib):
    """6 x 5 at s_q = 16, s_r = 8 (tests/contain_cases.py: crafted_rows): empty, short, full, identical and disjoint lists, tau on
    a value both hold, on a value one holds, between values, lists ending in 2^64 - 1, padding and lengths above the sketch size"""
    got = run("crafted")
    assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1   # 30 pairs: the pair kernel alone
    check(got, cc.expected("crafted"))


@pytest.mark.parametrize("name,env,ranges", [("small", {}, 16), ("mixed", {}, 64), ("mixed", {"MHX_SEARCH_QBATCH": "13"}, 64), ("set200", {}, 64),
                                             ("mixed", {"MHX_SEARCH_GEOMETRY": "dist"}, 1024), ("extreme", {}, 64), ("extreme_mirrored", {}, 64),
                                             ("extreme", {"MHX_SEARCH_GEOMETRY": "dist"}, 1024)])
def test_range_route(lib, monkeypatch, name, env, ranges):
    """mixed: 40 queries at s_q = 1000 against 33 references at s_r = 200 -- two slices, the second of one reference, the
    slice-per-wave range pass; set200: 150 x 200 at s = 1000, the one-query-per-lane range pass, seven slices; extreme: short
    lists whose tau is 2^64 - 1 and lies in the top range, next to 2^64 - 1 itself as a hash.  No block falls back."""
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    got = run(name)
    assert lib.mhx_last_dist_ranges() == ranges and lib.mhx_last_dist_fallback_blocks() == 0
    check(got, cc.expected(name), name)
    if name == "mixed":   # the property the mode is for: the first ten queries hold genome i and a contaminant as large or larger
        shared, n_qry, n_ref = got
        for i in range(9):   # (reference 9 is the empty list)
            assert shared[i, i] == n_ref[i, i] > 0 and n_qry[i, i] > n_ref[i, i]
        assert n_ref[9, 9] == 0 and n_qry[9, 9] == 1000


@pytest.mark.parametrize("name", ["crowded", "plasmids", "plasmids_swapped"])
def test_flagged_blocks_go_to_the_pair_kernel(lib, name):
    """crowded: nearly every value in one range; plasmids: a short list spans the hash space, so the full list of a 240 000-hash
    genome lies in the lowest range and its slice passes 255 entries"""
    got = run(name)
    assert lib.mhx_last_dist_fallback_blocks() > 0
    check(got, cc.expected(name), name)
    if name == "plasmids":   # references 0, 3 and 4 lie inside the genomes of queries 0, 1 and 1; 3 also inside query 5's
        shared, n_qry, n_ref = got
        for q, r in ((0, 0), (1, 3), (1, 4), (5, 3)):   # (the window of a 1000-hash sketch of 240 000 hashes holds few plasmid hashes, or none)
            assert shared[q, r] == n_ref[q, r] and n_qry[q, r] == 1000


def test_more_blocks_than_one_group_of_flag_words(lib, monkeypatch):
    """The flag words of the blocks come back per group of 4096 blocks.  One query per block, 140 queries against 960 references
    (30 slices) of 64 hashes: 4200 blocks, the last 104 in a second group, whose flag words are cleared and used again
    (tests/contain_cases.py: two_groups).  Queries 136 to 139 derive from references of slices 21, 28 and 29: their blocks lie
    in the second group and hold counts that are not zero.  No range is crowded, so no block falls back."""
    monkeypatch.setenv("MHX_SEARCH_QBATCH", "1")
    Q, q_len, R, r_len, s_q, s_r = cc.rows_of("two_groups")
    nq, nr = len(q_len), len(r_len)
    nblocks = nq * ((nr + 31) // 32)
    assert nblocks > 4096 and 136 * 30 + 21 >= 4096   # query 136's block with slice 21 lies in the second group
    got = engine.dist_contain(Q, q_len, R, r_len, s_q, s_r)
    assert lib.mhx_last_dist_ranges() == 16 and lib.mhx_last_dist_fallback_blocks() == 0
    want = cc.expected("two_groups")
    check(got, want, "two_groups")
    for q, r in ((136, 700), (137, 900), (138, 930), (139, 959)):
        assert want[0][q, r] > 0 and got[0][q, r] == want[0][q, r]
    assert want[0][137, 900] == want[2][137, 900] == 64   # a reference that is its query


def test_a_pair_without_a_geometry(lib):
    """70 000 entries: above the base form of the range route"""
    got = run("long_pair")
    assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1
    check(got, cc.expected("long_pair"))


CHILD = """
import sys
import numpy as np
from auriclass_amd import engine
from tests import contain_cases as cc
engine.init()
out = {}
for name in ("mixed", "extreme"):
    got = engine.dist_contain(*cc.rows_of(name))
    assert engine.load().mhx_last_dist_ranges() == 0 and engine.load().mhx_last_dist_fallback_blocks() == -1
    for what, a in zip(("shared", "n_qry", "n_ref"), got):
        out[name + "_" + what] = a
np.savez(sys.argv[1], **out)
"""


def test_generic_kernel_in_a_child_process_equals_the_range_route(lib, tmp_path):
    """MHX_DIST_GENERIC=1 is read per call, but a child process is how a user sets it"""
    path = tmp_path / "generic.npz"
    env = dict(os.environ, MHX_DIST_GENERIC="1")
    done = subprocess.run([sys.executable, "-c", CHILD, str(path)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    theirs = np.load(path)
    for name in ("mixed", "extreme"):
        got = run(name)
        assert lib.mhx_last_dist_ranges() == 64 and lib.mhx_last_dist_fallback_blocks() == 0
        for what, a in zip(("shared", "n_qry", "n_ref"), got):
            assert np.array_equal(a, theirs[name + "_" + what]), (name, what)


def test_device_pointers_twice_against_the_host_form(lib):
    """everything on the device, lengths above the sketch size and above the stride included (the kernels clip what the host
    form refuses); the same integers as the host form, and the same the second time"""
    dev = torch.device("cuda")
    for name in ("mixed", "crafted"):
        Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows() if name == "crafted" else cc.rows_of(name)
        host = engine.dist_contain(Q, q_len, R, r_len, s_q, s_r)
        lying_q, lying_r = q_len.copy(), r_len.copy()
        lying_q[q_len >= s_q] = 0xFFFFFFF0   # a full list whose length lies: the stride and s bound it
        lying_r[r_len >= s_r] = Q.shape[1] + 5
        d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, lying_q, R, lying_r)]
        nq, nr = len(q_len), len(r_len)
        for _ in range(2):
            out = [torch.full((nq, nr), 7, dtype=torch.int32, device=dev) for _ in range(3)]
            torch.cuda.synchronize()
            ms = engine.dist_contain_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, Q.shape[1],
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
            assert ms > 0
            check([o.cpu().numpy().view(np.uint32) for o in out], host, name)
        check(host, cc.expected(name), name)


def test_argument_checks(lib):
    Q, q_len, R, r_len, s_q, s_r = cc.crafted_rows()
    for bad_sq, bad_sr in ((0, s_r), (s_q, 0)):
        with pytest.raises(engine.EngineError) as e:
            engine.dist_contain(Q, q_len, R, r_len, bad_sq, bad_sr)
        assert e.value.code == engine.MHX_E_ARG
    too_long = q_len.copy()
    too_long[3] = Q.shape[1] + 1
    with pytest.raises(engine.EngineError) as e:
        engine.dist_contain(Q, too_long, R, r_len, s_q, s_r)
    assert e.value.code == engine.MHX_E_ARG and "q_len[3]" in e.value.message
    too_long = r_len.copy()
    too_long[1] = R.shape[1] + 1
    with pytest.raises(engine.EngineError) as e:
        engine.dist_contain(Q, q_len, R, too_long, s_q, s_r)
    assert e.value.code == engine.MHX_E_ARG and "r_len[1]" in e.value.message
    v = ctypes.c_void_p
    out = np.zeros((6, 5), np.uint32)
    assert lib.mhx_dist_contain(v(Q.ctypes.data), v(q_len.ctypes.data), 6, s_q, v(R.ctypes.data), v(r_len.ctypes.data), 5, s_r, 0, v(out.ctypes.data),
                                v(out.ctypes.data), v(out.ctypes.data), 0) == engine.MHX_E_ARG   # stride 0
    assert lib.mhx_dist_contain(v(Q.ctypes.data), v(q_len.ctypes.data), 6, s_q, v(R.ctypes.data), v(r_len.ctypes.data), 5, s_r, 24, None,
                                v(out.ctypes.data), v(out.ctypes.data), 0) == engine.MHX_E_ARG   # a null output
    # no queries or no references: a successful no-op that touches nothing
    out[:] = 9
    assert lib.mhx_dist_contain(None, None, 0, s_q, v(R.ctypes.data), v(r_len.ctypes.data), 5, s_r, 24, v(out.ctypes.data), v(out.ctypes.data), v(out.ctypes.data), 0) == 0
    assert lib.mhx_dist_contain(v(Q.ctypes.data), v(q_len.ctypes.data), 6, s_q, None, None, 0, s_r, 24, v(out.ctypes.data), v(out.ctypes.data), v(out.ctypes.data), 0) == 0
    assert (out == 9).all()

"""The winner-take-all containment on the GPU (mhx_dist_contain_winner) against the rule of tests/contain_winner_rule.py, every
integer exact: small calls on the pair-kernel route, the range route (whatever the query batch), flagged blocks, a pair
without a geometry, 2^64 - 1 as a hash that is won, the counter of the claim pass, the device-pointer form, and the argument
checks."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_screen.py: the two then share one device runtime

from auriclass_amd import engine
from tests import contain_rule as rule
from tests import contain_winner_cases as wc
from tests import contain_winner_rule as wrule

pytestmark = pytest.mark.gpu
COLS = ("won", "shared", "n_qry", "n_ref")


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def run(name):
    Q, q_len, R, r_len, s_q, s_r, lengths = wc.rows_of(name)
    return engine.dist_contain_winner(Q, q_len, R, r_len, s_q, s_r, lengths)


def check(got, want, what=""):
    for name, a, b in zip(COLS, got, want):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, bad[:5], a[tuple(bad[0])], b[tuple(bad[0])])


def check_case(lib, name):
    got = run(name)
    want = wc.expected(name)
    check(got, want[:4], name)
    wrule.check_consequences(*got, want[4], wc.rows_of(name)[6])
    assert lib.mhx_last_contain_winner_pairs() == int((want[1] > 0).sum())   # the claim pass walked the pairs that share something
    return got


@pytest.mark.parametrize("name", ["tau_and_ties", "tau_and_ties_lengths", "crafted"])
def test_small_calls_on_the_pair_kernel_route(lib, name):
    """tau_and_ties: a value held only behind a reference's bound is not found there, tau is inclusive, an exact tie goes to the
    lower index or, with lengths, to the longer genome; crafted: empty, short, full and disjoint lists, 2^64 - 1 won by reference 3"""
    got = check_case(lib, name)
    assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1
    if name == "tau_and_ties":
        assert got[0].tolist() == [[8, 2, 0, 0, 1]]
    if name == "tau_and_ties_lengths":
        assert got[0].tolist() == [[0, 2, 8, 0, 1]]
    if name == "crafted":
        assert got[0].tolist() == [[0, 0, 0, 0, 0], [0, 3, 0, 0, 0], [0, 3, 5, 0, 0], [0, 0, 0, 0, 0], [0, 3, 0, 3, 0], [0, 1, 1, 3, 0]]


@pytest.mark.parametrize("name,env", [("clades", {}), ("mixed", {}), ("mixed", {"MHX_SEARCH_QBATCH": "13"})])
def test_range_route(lib, monkeypatch, name, env):
    """clades: 7 x 14, what the mode exists for; mixed: 40 x 33, two reference slices -- a query's words see every reference of
    both --, and the same integers when the queries go in batches of 13.  No block falls back."""
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    won, shared, n_qry, n_ref = check_case(lib, name)
    assert lib.mhx_last_dist_ranges() == 64 and lib.mhx_last_dist_fallback_blocks() == 0
    if name == "clades":
        for c in range(3):
            assert won[c, 4 * c] == n_ref[c, 4 * c] == 200
        m = wc.CLADE_MIXED_QUERY
        assert won[m, 0] == 200 and won[m, 8] == 200
        assert (won[wc.CLADE_SHORT_QUERY, wc.CLADE_SHORT_REF], won[wc.CLADE_SHORT_QUERY, :4].sum()) == (17, 0)
    if name == "mixed":   # the mixed cultures: queries 33 + i hold genomes 2 i and 2 i + 1
        Q, q_len, R, r_len, s_q, s_r, _ = wc.rows_of(name)
        for i in range(7):
            qi, a, b = 33 + i, 2 * i, 2 * i + 1
            q = rule.the_list(Q[qi], q_len[qi], s_q)
            fa, fb = (wrule.found(q, rule.the_list(R[j], r_len[j], s_r), s_q, s_r) for j in (a, b))
            hi, lo, fhi, flo = (a, b, fa, fb) if wrule.best_ranked(shared[qi:qi + 1, a:b + 1], n_ref[qi:qi + 1, a:b + 1])[0] == 0 else (b, a, fb, fa)
            assert won[qi, hi] == len(fhi) and won[qi, lo] == len(flo - fhi), (qi, hi, lo)   # the lower-ranked one loses what both hold
            assert won[qi].sum() == won[qi, a] + won[qi, b] == len(fa | fb)


@pytest.mark.parametrize("name", ["plasmids", "plasmids_swapped", "crowded"])
def test_flagged_blocks(lib, name):
    """the plain pass of these goes to the pair kernel block by block; the claim pass behind it sees the same outputs"""
    check_case(lib, name)
    assert lib.mhx_last_dist_fallback_blocks() > 0


def test_a_pair_without_a_geometry(lib):
    """70 000 entries: 70 000 winner words of one query, one pair that wins everything it found"""
    won, shared, n_qry, n_ref = check_case(lib, "long_pair")
    assert lib.mhx_last_dist_ranges() == 0 and lib.mhx_last_dist_fallback_blocks() == -1
    assert won[0, 0] == shared[0, 0] > 50000


@pytest.mark.parametrize("name", ["extreme", "extreme_mirrored"])
def test_the_largest_hash_is_won(lib, name):
    """2^64 - 1 is a hash like any other: found at the last position of a query's list, credited to one reference"""
    check_case(lib, name)
    winners = wc.expected(name)[5]
    assert any(2 ** 64 - 1 in best for best in winners)   # the case holds what it is here for


def test_disjoint_sets_walk_no_pair(lib):
    rng = np.random.default_rng(99)
    Q = np.sort(rng.integers(0, 2 ** 62, size=(9, 64), dtype=np.uint64), axis=1)
    R = np.sort(rng.integers(2 ** 62, 2 ** 63, size=(11, 64), dtype=np.uint64), axis=1)
    lens = np.full(9, 64, np.uint32), np.full(11, 64, np.uint32)
    won, shared, n_qry, n_ref = engine.dist_contain_winner(Q, lens[0], R, lens[1], 64, 64)
    assert lib.mhx_last_contain_winner_pairs() == 0
    assert not won.any() and not shared.any()
    check((shared, n_qry, n_ref), rule.matrix_of_rows(Q, lens[0], R, lens[1], 64, 64))


def test_device_pointers_twice_against_the_host_form(lib):
    """everything on the device, ref_length too, lengths above the sketch size and above the stride included; the same integers
    as the host form, the same the second time, and shared / n_qry / n_ref are dist_contain's"""
    dev = torch.device("cuda")
    for name in ("mixed", "crafted"):
        Q, q_len, R, r_len, s_q, s_r, _ = wc.rows_of(name)
        nq, nr = len(q_len), len(r_len)
        lengths = (1000 + (np.arange(nr, dtype=np.uint64) * 7) % 5).astype(np.uint64)   # ties in the length too
        host = engine.dist_contain_winner(Q, q_len, R, r_len, s_q, s_r, lengths)
        check(host, wrule.matrix_of_rows(Q, q_len, R, r_len, s_q, s_r, lengths)[:4], name)
        check(host[1:], engine.dist_contain(Q, q_len, R, r_len, s_q, s_r), name)
        lying_q, lying_r = q_len.copy(), r_len.copy()
        lying_q[q_len >= s_q] = 0xFFFFFFF0   # a full list whose length lies: the stride and s bound it
        lying_r[r_len >= s_r] = Q.shape[1] + 5
        d = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in (Q, lying_q, R, lying_r, lengths)]
        for _ in range(2):
            out = [torch.full((nq, nr), 7, dtype=torch.int32, device=dev) for _ in range(4)]
            torch.cuda.synchronize()
            ms = engine.dist_contain_winner_device(d[0].data_ptr(), d[1].data_ptr(), nq, s_q, d[2].data_ptr(), d[3].data_ptr(), nr, s_r, Q.shape[1],
                                                   d[4].data_ptr(), *(o.data_ptr() for o in out))
            assert ms > 0
            check([o.cpu().numpy().view(np.uint32) for o in out], host, name)


def test_argument_checks(lib):
    Q, q_len, R, r_len, s_q, s_r, _ = wc.rows_of("crafted")
    for bad_sq, bad_sr in ((0, s_r), (s_q, 0)):
        with pytest.raises(engine.EngineError) as e:
            engine.dist_contain_winner(Q, q_len, R, r_len, bad_sq, bad_sr)
        assert e.value.code == engine.MHX_E_ARG
    too_long = q_len.copy()
    too_long[3] = Q.shape[1] + 1
    with pytest.raises(engine.EngineError) as e:
        engine.dist_contain_winner(Q, too_long, R, r_len, s_q, s_r)
    assert e.value.code == engine.MHX_E_ARG and "q_len[3]" in e.value.message
    v = ctypes.c_void_p
    out = np.full((6, 5), 9, np.uint32)
    o = v(out.ctypes.data)
    args = (v(Q.ctypes.data), v(q_len.ctypes.data), 6, s_q, v(R.ctypes.data), v(r_len.ctypes.data), 5, s_r)
    call = lib.mhx_dist_contain_winner
    assert call(*args, 0, None, o, o, o, o, 0) == engine.MHX_E_ARG     # stride 0
    assert call(*args, 24, None, None, o, o, o, 0) == engine.MHX_E_ARG   # a null `won`
    assert call(*args, 24, None, o, None, o, o, 0) == engine.MHX_E_ARG   # a null output
    # no queries or no references: a successful no-op that touches nothing
    assert call(None, None, 0, s_q, v(R.ctypes.data), v(r_len.ctypes.data), 5, s_r, 24, None, o, o, o, o, 0) == 0
    assert call(v(Q.ctypes.data), v(q_len.ctypes.data), 6, s_q, None, None, 0, s_r, 24, None, o, o, o, o, 0) == 0
    assert (out == 9).all()

"""Jackknife support of search hits on the GPU (mhx_dist_support) against the rule of tests/support_rule.py on the cases of
tests/support_cases.py: first, rep_best, rep_s, rep_common and rep_denom byte for byte in both pointer forms, twice each, with
the caller's rows unchanged; the replicates' pair results once more through the device's own pinned path (mhx_resample_rows +
mhx_dist_batch); batches forced by MHX_SUPPORT_WORK_MB; the argument checks; a replicate that keeps nothing."""
import ctypes

import numpy as np
import pytest
import torch   # before the engine's library, as in tests/test_gpu_triangle.py: the two then share one device runtime

from auriclass_amd import engine
from tests import search_cases as sc
from tests import support_cases as cases
from tests import support_rule as rule
from tests import triangle_cases as tc

pytestmark = pytest.mark.gpu
K = cases.K
NAMES = ("first", "rep_best", "rep_s", "rep_common", "rep_denom")


@pytest.fixture(scope="module")
def lib():
    engine.init()
    return engine.load()


def dev():
    return f"cuda:{torch.cuda.current_device()}"


def cand_arrays(rows, top):
    """cand [nq, top] (7 behind a row's end: a valid index that must not be looked at) and n_cand [nq]"""
    cand = np.full((len(rows), top), 7, np.uint32)
    for i, row in enumerate(rows):
        cand[i, :len(row)] = row
    return cand, np.array([len(row) for row in rows], np.uint32)


def host_form(Mq, lq, Mr, lr, s, R, keep, seed, cand, n_cand):
    return engine.dist_support(Mq, lq, Mr, lr, s, R, keep, seed, cand, n_cand)


def device_form(Mq, lq, Mr, lr, s, R, keep, seed, cand, n_cand):
    """device pointers on copies, the outputs filled with something else before; the inputs must come back unchanged"""
    nq, nr = Mq.shape[0], Mr.shape[0]
    top = nr if cand is None else cand.shape[1]
    t64 = lambda a: torch.from_numpy(a.view(np.int64)).to(dev())   # noqa: E731
    t32 = lambda a: torch.from_numpy(a.view(np.int32)).to(dev())   # noqa: E731
    d_q, d_r, d_ql, d_rl = t64(Mq), t64(Mr), t32(lq), t32(lr)
    d_c, d_n = (None, None) if cand is None else (t32(cand), t32(n_cand))
    outs = [torch.full(shape, -3, dtype=torch.int32, device=dev()) for shape in ((nq, top), (nq, R), (nq, R), (nq, top, R), (nq, top, R))]
    torch.cuda.synchronize()
    ms = engine.dist_support_device(d_q.data_ptr(), d_ql.data_ptr(), nq, d_r.data_ptr(), d_rl.data_ptr(), nr, Mq.shape[1], s, top, R, keep, seed,
                                    0 if cand is None else d_c.data_ptr(), 0 if cand is None else d_n.data_ptr(), *(o.data_ptr() for o in outs))
    assert ms > 0
    assert d_q.cpu().numpy().view(np.uint64).tobytes() == Mq.tobytes() and d_r.cpu().numpy().view(np.uint64).tobytes() == Mr.tobytes()
    assert d_ql.cpu().numpy().view(np.uint32).tobytes() == lq.tobytes() and d_rl.cpu().numpy().view(np.uint32).tobytes() == lr.tobytes()
    return tuple(o.cpu().numpy().view(np.uint32) for o in outs)


def check_call(queries, references, rows, s, R, keep, seed, stride=None, top=None, null_cand=False, forms=(host_form, device_form), times=2):
    """both forms, twice each, against the rule; returns the rule's arrays"""
    if stride is None:
        stride = tc.pad_rows(list(queries) + list(references))[0].shape[1]
    Mq, lq = tc.pad_rows(queries, stride)
    Mr, lr = tc.pad_rows(references, stride)
    top = len(references) if null_cand else top
    cand, n_cand = (None, None) if null_cand else cand_arrays(rows, top)
    want = cases.expected_call(queries, references, rows, top, s, R, keep, seed)
    valid = want[5]
    for form in forms:
        for _ in range(times):
            got = form(Mq, lq, Mr, lr, s, R, keep, seed, cand, n_cand)
            for name, g, w in zip(NAMES, got, want):
                if g.ndim == 3:   # pair results: the cells of candidates that do not count are unspecified
                    g = np.where(valid[:, :, None], g, 0)
                assert g.tobytes() == w.tobytes(), (form.__name__, name)
            assert all(int(want[0][i].sum()) == (R if len(rows[i]) else 0) for i in range(len(queries)))
    return want


def all_refs(nq, nr):
    return tuple(tuple(range(nr)) for _ in range(nq))


@pytest.mark.parametrize("R", [1, 8, 63, 64, 65, 130])
def test_near_tie_counts_equal_the_rule(lib, R):
    """cand == NULL with nr = 8; the winner changes from replicate to replicate"""
    qs, refs = cases.near_tie()
    want = check_call(qs, refs, all_refs(1, 8), cases.S, R, 0.5, 42, null_cand=True)
    if R >= 8:   # on the rule's values: otherwise counting could not be told from a constant
        assert ((want[0] > 0) & (want[0] < R)).any(), want[0].tolist()
    if R == 8:
        assert want[0][0].tolist() == [0, 6, 0, 0, 1, 1, 0, 0] and 472 <= want[2].min() and want[2].max() <= 495
    if R == 64:
        assert int((want[0] > 0).sum()) == 5
    assert lib.mhx_last_dist_kernel_ms() > 0


@pytest.mark.parametrize("keep", [0.5, 1.0, 0.03])
@pytest.mark.parametrize("seed", [42, 2 ** 64 - 1])
def test_keep_rates_and_seeds(lib, keep, seed):
    qs, refs = cases.near_tie()
    check_call(qs, refs, all_refs(1, 8), cases.S, 5, keep, seed, null_cand=True, times=1)
    lad, rows = cases.ladder(), cases.ladder_cands()
    check_call(lad, lad, rows, cases.S, 5, keep, seed, stride=1008, top=16, times=1)


def test_ties_go_to_the_lower_reference(lib):
    qs, lists, rows = cases.ties()
    want = check_call(qs, lists, rows, cases.S, 8, 0.5, 42, top=8)
    assert (want[1][0] == 5).all() and (want[1][1] == 77).all()


@pytest.mark.parametrize("stride", [1000, 1008, 1024])
def test_short_lists_at_every_stride(lib, stride):
    """every list of the ladder as a query against the others: complete sets, unions below s_r, denom < s_r, 0/0"""
    lad, rows = cases.ladder(), cases.ladder_cands()
    want = check_call(lad, lad, rows, cases.S, 5, 0.5, 42, stride=stride, top=16)
    assert (want[4] < want[2][:, None, :])[want[5]].any()   # denom < s_r somewhere
    e0, e1 = [i for i, v in enumerate(lad) if len(v) == 0]
    cell = (e0, rows[e0].index(e1))
    assert want[3][cell].tolist() == [0] * 5 and want[4][cell].tolist() == [0] * 5   # the empty query against the empty reference: 0/0


def test_candidate_lists_that_differ(lib):
    """n_cand 1, 2, 33, 64 and 0 in one call, top = 64, candidates in no order"""
    lists, s = tc.set200()
    refs = lists[:70]
    qs = [sc.queries()[i] for i in (0, 1, 24, 26, 27)]
    rng = np.random.default_rng(3)
    rows = [tuple(int(x) for x in rng.permutation(70)[:n]) for n in (1, 2, 33, 64, 0)]
    rows[2] = (5,) + tuple(x for x in rows[2] if x != 5)[:32]   # the query that copies list 5 has it among its candidates
    want = check_call(qs, refs, rows, s, 3, 0.5, 42, top=64)
    assert (want[1][4] == rule.NONE).all() and int(want[0][4].sum()) == 0 and (want[1][2] == 5).all()


def test_batches_do_not_change_the_result(lib, monkeypatch):
    """14 queries at top = 64 and R = 130 need 99 KiB of workspace each: a bound of 1 MiB makes two batches"""
    lad, rows = cases.ladder(), cases.ladder_cands()
    monkeypatch.setenv("MHX_SUPPORT_WORK_MB", "1")
    check_call(lad, lad, rows, cases.S, 130, 0.5, 42, top=64, times=1)
    monkeypatch.delenv("MHX_SUPPORT_WORK_MB")
    check_call(lad, lad, rows, cases.S, 130, 0.5, 42, top=64, times=1, forms=(host_form,))


def test_auriclass_sketch_size(lib):
    """s = 50 000: a list is many times longer than one wave's share"""
    qs, refs, s = cases.long()
    check_call(qs, refs, all_refs(1, 3), s, 4, 0.5, 42, null_cand=True)


def test_pair_results_through_the_pinned_distance_path(lib):
    """three replicates of the near-tie set and of ladder queries: mhx_resample_rows + mhx_dist_batch give the same pairs"""
    (Q,), refs = cases.near_tie()
    lad, rows = cases.ladder(), cases.ladder_cands()
    for q, cands in ((Q, list(refs)), (lad[-1], [lad[j] for j in rows[-1]]), (lad[4], [lad[j] for j in rows[4]])):
        M, lens = tc.pad_rows([q] + cands)
        Mq, lq = M[:1], lens[:1]
        _, _, rep_s, rep_c, rep_d = engine.dist_support(Mq, lq, M[1:], lens[1:], cases.S, 3, 0.5, 42)
        for r in range(3):
            out, out_len, s_r = engine.resample_rows(M, lens, cases.S, 42, r, 0.5)
            common, denom, _ = engine.dist_batch(out[:1], out_len[:1], out[1:], out_len[1:], K, s_r)
            assert s_r == rep_s[0, r]
            assert common[0].tolist() == rep_c[0, :, r].tolist() and denom[0].tolist() == rep_d[0, :, r].tolist()


def test_bad_arguments_leave_the_sentinels(lib):
    qs, refs = cases.near_tie()
    Mq, lq = tc.pad_rows(qs, 1008)
    Mr, lr = tc.pad_rows(refs, 1008)
    cand, n_cand = cand_arrays([(0, 3, 5)], 4)
    o = np.full(4 * 8 * 8, 77, np.uint32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.ctypes.data)   # noqa: E731

    def call(q=Mq, ql=lq, nq=1, r=Mr, rl=lr, nr=8, stride=1008, s=cases.S, c=cand, n=n_cand, top=4, R=8, keep=0.5, first=o, best=o, rs=o, rc=o, rd=o):
        return lib.mhx_dist_support(p(q), p(ql), nq, p(r), p(rl), nr, stride, s, p(c), p(n), top, R, keep, 42, p(first), p(best), p(rs), p(rc), p(rd), 0)
    for kw in ({"q": None}, {"ql": None}, {"r": None}, {"rl": None}, {"first": None}, {"n": None}, {"rc": None}, {"rd": None}):
        assert call(**kw) == engine.MHX_E_ARG and b"null argument" in lib.mhx_last_error(), kw
    assert call(s=0) == engine.MHX_E_ARG and call(stride=0) == engine.MHX_E_ARG
    for top in (0, 65):
        assert call(top=top) == engine.MHX_E_ARG and b"top" in lib.mhx_last_error()
    assert call(n=np.array([5], np.uint32)) == engine.MHX_E_ARG and b"n_cand" in lib.mhx_last_error()
    assert call(c=np.array([0, 8, 5, 7], np.uint32)) == engine.MHX_E_ARG and b"no reference" in lib.mhx_last_error()
    assert call(c=np.array([0, 3, 3, 7], np.uint32)) == engine.MHX_E_ARG and b"twice" in lib.mhx_last_error()
    for lens_kw in ("ql", "rl"):
        bad = (lq if lens_kw == "ql" else lr).copy()
        bad[0] = 1009
        assert call(**{lens_kw: bad}) == engine.MHX_E_ARG and b"exceeds stride" in lib.mhx_last_error()
    for keep in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(keep=keep) == engine.MHX_E_ARG and b"keep" in lib.mhx_last_error()
    for R in (0, 10001):
        assert call(R=R) == engine.MHX_E_ARG and b"replicates" in lib.mhx_last_error()
    assert call(c=None, n=None) == engine.MHX_E_ARG and b"top must be nr" in lib.mhx_last_error()            # top 4, nr 8
    assert call(c=None, n=None, nr=65, top=65) == engine.MHX_E_ARG
    assert (o == 77).all()
    assert call(nq=0) == engine.MHX_OK and (o == 77).all()   # no query: nothing written
    # the same arguments in buffers of their own: accepted, and the optional outputs may be missing
    want = cases.expected(qs[0], [refs[j] for j in (0, 3, 5)], (0, 3, 5), cases.S, 8, 0.5, 42)
    for kw in ({}, {"best": None, "rs": None, "rc": None, "rd": None}, {"rs": None}, {"best": None}):
        first, best, rs, rc, rd = (np.full(n, 77, np.uint32) for n in (4, 8, 8, 32, 32))
        given = dict(first=first, best=best, rs=rs, rc=rc, rd=rd)
        given.update(kw)
        assert call(**given) == engine.MHX_OK and first.tolist() == want.first.tolist() + [0]
        assert (best.tolist() == want.rep_best.tolist()) == ("best" not in kw) and (rs.tolist() == want.rep_s.tolist()) == ("rs" not in kw)
        assert (rc[:24].reshape(3, 8).tolist() == want.rep_common.tolist()) == ("rc" not in kw)


def test_a_replicate_that_keeps_nothing_is_refused(lib):
    """keep 0.03 on a full list of one hash, s = 1"""
    one = np.array([[5]], np.uint64)
    ln = np.array([1], np.uint32)
    with pytest.raises(ValueError, match="replicate 0"):
        rule.support_fast(one[0], [one[0]], [0], 1, K, 4, 0.03, 42)
    with pytest.raises(engine.EngineError) as exc:
        engine.dist_support(one, ln, one, ln, 1, 4, 0.03, 42)
    assert exc.value.code == engine.MHX_E_ARG and "query 0" in exc.value.message and "replicate 0" in exc.value.message and "keep" in exc.value.message
    first, best, rep_s, _, _ = engine.dist_support(one, ln, one, ln, 1, 4, 1.0, 42)   # behind the refusal the engine works as before
    assert first.tolist() == [[4]] and best.tolist() == [[0] * 4] and rep_s.tolist() == [[1] * 4]

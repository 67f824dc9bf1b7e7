"""The unbounded containment call at file level (mhx_contain_files_within) and through `python -m auriclass_amd.contain --all`,
against the rows of the restated rule (tests/contain_within_rule.py): names and integers exact and in the rule's order, identity
and p-value to the sixth digit as the containment's file tests compare a %g column; the retry of a batch whose hits exceed its
first buffers, a list of query files, the refusals of the command line, and the bytes of every call that does not say --all."""
import numpy as np
import pytest

from auriclass_amd import contain, engine
from tests import contain_cases as cc
from tests import contain_rule
from tests import contain_within_cases as cwc
from tests import contain_within_rule as rule

pytestmark = pytest.mark.gpu
K = cc.K
CUTS = ((0, 3), (3, 41), (41, 70))


def write(path, prefix, lists, s, k=K):
    """one sketch file of the lists cut at s; returns (names, comments, lengths).  The lengths are those of large genomes: at
    800 000 bases the p-value of 64 shared hashes out of 64 lies below the smallest normal double, where six digits do not exist"""
    lists = [np.asarray(v[:s], np.uint64) for v in lists]
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [3_000_000_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    engine.msh_write(path, k, s, names, comments, lengths, lists)
    return names, comments, lengths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """crowd as files: a reference file at s = 64, three query files at s = 128"""
    engine.init()
    d = tmp_path_factory.mktemp("contain_within")
    qs, rs, s_q, s_r = cwc.crowd()
    R = write(d / "ref.msh", "ref", rs, s_r)
    Q = [write(d / ("q%d.msh" % i), "q%d" % i, qs[a:b], s_q) for i, (a, b) in enumerate(CUTS)]
    return d, R, Q


def want_rows(R, Q, which=0, first=0, **kw):
    """the rule's rows for the query files Q[first:]; which: 0 names, 1 comments"""
    shared, n_qry, n_ref = (m[CUTS[first][0]:] for m in cwc.matrix())
    names = [n for q in Q[first:] for n in q[which]]
    sizes = [l for q in Q[first:] for l in q[2]]
    return rule.text_rows(R[which], names, sizes, shared, n_qry, n_ref, K, **kw)


def same(text, want):
    rows = contain_rule.rows_of_text(text)
    assert len(rows) == len(want) and [(r[0], r[1]) + r[4:] for r in rows] == [(w[0], w[1]) + w[4:] for w in want]   # the order too
    assert contain_rule.same_rows(rows, want)


def test_text_equals_the_rules_rows_in_both_orders(files):
    d, R, Q = files
    paths = [d / "q0.msh", d / "q1.msh", d / "q2.msh"]
    for min_identity, min_shared in cwc.bounds()[2:6]:   # a main bound; the identity of a pair and its two neighbours
        for order, name in ((0, "ref"), (1, "best")):
            want = want_rows(R, Q, min_identity=min_identity, min_shared=min_shared, order=name)
            text = engine.contain_files(d / "ref.msh", paths, min_identity=min_identity, min_shared=min_shared, all_hits=True, order=order)
            same(text, want)
    text = engine.contain_files(d / "ref.msh", paths, min_identity=0.9, all_hits=True)   # best first is the default
    assert sum(line.split("\t")[1] == "q0/genome0.fasta" for line in text.splitlines()) > 64
    for line in text.splitlines()[:40]:
        cols = line.split("\t")
        assert len(cols) == 6 and cols[2] == "%g" % float(cols[2]) and cols[3] == "%g" % float(cols[3])
    assert engine.contain_files(d / "ref.msh", paths, min_identity=0.9, all_hits=True, order=0) != text
    # the p-value bound drops rows on the host; a bound between two p-values that occur, far from both
    full = want_rows(R, Q, min_identity=0.9, order="ref")
    ps = sorted({r[3] for r in full})
    gaps = [(b / a, a * (b / a) ** 0.5) for a, b in zip(ps, ps[1:]) if a > 0]
    bound = max(gaps[len(gaps) // 4: 3 * len(gaps) // 4])[1]
    for order, name in ((0, "ref"), (1, "best")):
        cut = want_rows(R, Q, min_identity=0.9, max_p_value=bound, order=name)
        assert 0 < len(cut) < len(full)
        same(engine.contain_files(d / "ref.msh", paths, min_identity=0.9, max_p_value=bound, all_hits=True, order=order), cut)
    # comments in place of the names; queries without hits print nothing
    same(engine.contain_files(d / "ref.msh", paths[1:], min_identity=0.95, min_shared=10, comment=True, all_hits=True),
         want_rows(R, Q, 1, 1, min_identity=0.95, min_shared=10))
    assert engine.contain_files(d / "ref.msh", [d / "q2.msh"], min_identity=0.99, min_shared=30, all_hits=True) == ""


def test_a_batch_with_more_hits_than_its_first_buffers(files):
    """crowd at (0, 1): 4581 hits in one batch of 70 sketches, which has room for 4096 at first -- the batch is repeated once
    with the size the device reported.  A list of two query files gives the text of the two, one after the other."""
    d, R, Q = files
    paths = [d / "q0.msh", d / "q1.msh", d / "q2.msh"]
    want = want_rows(R, Q, order="ref")
    assert len(want) > 4096
    text = engine.contain_files(d / "ref.msh", paths, all_hits=True, order=0)
    same(text, want)
    same(engine.contain_files(d / "ref.msh", paths, all_hits=True), want_rows(R, Q))
    one_by_one = [engine.contain_files(d / "ref.msh", [p], all_hits=True, order=0) for p in paths]
    assert "".join(one_by_one) == text and all(t for t in one_by_one)
    assert engine.contain_files(d / "ref.msh", [paths[2], paths[0]], all_hits=True, order=0) == one_by_one[2] + one_by_one[0]


def test_bad_options_and_mismatches(files, tmp_path):
    d, R, Q = files
    for bad in (dict(order=2), dict(min_shared=0), dict(min_identity=float("nan")), dict(max_p_value=float("nan")), dict(top=5), dict(winner=True)):
        with pytest.raises(engine.EngineError) as exc:
            engine.contain_files(d / "ref.msh", [d / "q0.msh"], all_hits=True, **bad)
        assert exc.value.code == engine.MHX_E_ARG, bad
    qs = cwc.crowd()[0]
    write(tmp_path / "k19.msh", "k19", qs[:3], cwc.S_Q, k=19)
    write(tmp_path / "s100.msh", "s100", qs[:3], 100)
    for other, words in ((tmp_path / "k19.msh", "different k-mer sizes"), (tmp_path / "s100.msh", "different sketch sizes")):
        with pytest.raises(engine.EngineError) as want:
            engine.contain_files(d / "ref.msh", [d / "q0.msh", other], top=5)
        with pytest.raises(engine.EngineError) as got:
            engine.contain_files(d / "ref.msh", [d / "q0.msh", other], all_hits=True)
        assert got.value.code == want.value.code == engine.MHX_E_MISMATCH and got.value.message == want.value.message and words in got.value.message
    (tmp_path / "garbage.msh").write_bytes(b"not a sketch file at all" * 10)
    for ref in (tmp_path / "missing.msh", tmp_path / "garbage.msh"):
        with pytest.raises(engine.EngineError) as want:
            engine.contain_files(ref, [d / "q0.msh"], top=5)
        with pytest.raises(engine.EngineError) as got:
            engine.contain_files(ref, [d / "q0.msh"], all_hits=True)
        assert (got.value.code, got.value.message) == (want.value.code, want.value.message)


def test_command_line(files, capsys):
    d, R, Q = files
    ref, q0, q1 = str(d / "ref.msh"), str(d / "q0.msh"), str(d / "q1.msh")
    assert contain.main(["--all", "-i", "0.9", ref, q0, q1]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q0, q1], min_identity=0.9, all_hits=True, order=1)
    assert contain.main(["--all", "--order", "ref", "-i", "0.95", "-c", "10", "-v", "1e-10", "-C", "-p", "8", ref, q1]) == 0
    out = capsys.readouterr().out
    assert out == engine.contain_files(ref, [q1], min_identity=0.95, min_shared=10, max_p_value=1e-10, comment=True, all_hits=True, order=0) and out
    assert contain.main(["--all", "--order", "best", "-c", "10", ref, q0]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q0], min_shared=10, all_hits=True)
    for argv, words in ((["--all", "-n", "5"], "--all"), (["--all", "-w"], "--all"), (["--order", "ref"], "--order"), (["--order", "best", "-n", "5"], "--order"),
                        (["--all", "-c", "0"], "-c")):
        assert contain.main(argv + [ref, q0]) == 1
        out = capsys.readouterr()
        assert out.out == "" and out.err.startswith("ERROR: contain") and words in out.err, argv
    assert contain.main(["--all", "--order", "sideways", ref, q0]) == 1
    assert capsys.readouterr().out == ""
    assert contain.main(["-c", "2", ref, q0]) == 1
    out = capsys.readouterr()
    assert out.out == "" and out.err == "ERROR: contain -c (minimum shared hashes of a hit) needs -n\n"   # today's message, byte for byte


def test_without_all_the_bytes_are_those_of_before(files, capsys):
    """every form of the command that does not say --all makes the call it made before: the full table, -w and -n"""
    d, R, Q = files
    ref, q0 = str(d / "ref.msh"), str(d / "q0.msh")
    shared, n_qry, n_ref = (m[:3] for m in cwc.matrix())
    table = engine.contain_files(ref, [q0])
    assert contain_rule.same_rows(contain_rule.rows_of_text(table), contain_rule.expected_rows(R[0], Q[0][0], Q[0][2], shared, n_qry, n_ref, K))
    for argv, kw in (([], {}), (["-i", "0.9"], dict(min_identity=0.9)), (["-w"], dict(winner=True)), (["-n", "5", "-c", "2"], dict(top=5, min_shared=2)),
                     (["-n", "64", "-i", "0.9"], dict(top=64, min_identity=0.9))):
        assert contain.main(argv + [ref, q0]) == 0
        assert capsys.readouterr().out == engine.contain_files(ref, [q0], **kw)
    top = contain_rule.rows_of_text(engine.contain_files(ref, [q0], top=64, min_identity=0.9))
    everything = contain_rule.rows_of_text(engine.contain_files(ref, [q0], min_identity=0.9, all_hits=True))
    assert sum(r[1] == Q[0][0][0] for r in top) == 64 < sum(r[1] == Q[0][0][0] for r in everything)
    assert [r for r in everything if r[1] == Q[0][0][0]][:64] == [r for r in top if r[1] == Q[0][0][0]]

"""The containment search at file level (mhx_contain_files_search) and through `python -m auriclass_amd.contain -n`, against the
text of the restated rule (tests/contain_search_rule.py): names and integers exact, identity and p-value to the sixth digit as
the containment's file tests compare them.  Small sketch files written by the engine's own writer from synthetic lists, the
reference file at another sketch size than the queries."""
import functools

import numpy as np
import pytest

from auriclass_amd import contain, engine
from tests import contain_cases as cc
from tests import contain_rule as crule
from tests import contain_search_cases as csc
from tests import contain_search_rule as rule

pytestmark = pytest.mark.gpu
K = csc.K


@functools.lru_cache(maxsize=None)
def case():
    """the tie case and one more query, a genome that holds reference 3 whole, two hashes of reference 51 and one of reference
    50: rows whose p-value is far from 0 (one shared hash of 200 is chance), behind rows whose p-value is 0.
    (queries, references, s_q, s_r, (shared, n_qry, n_ref) by the rule)"""
    qs, rs, s_q, s_r = csc.ties()
    rng = np.random.default_rng(5150)
    more = (cc.union(cc.genome(rng, 20000), rs[3], rs[51][:2], rs[50][:1]),)
    counts = tuple(np.concatenate([a, b]) for a, b in zip(csc.expected(), crule.matrix(more, rs, s_q, s_r)))
    return qs + more, rs, s_q, s_r, counts


def write(path, prefix, lists, s):
    """one sketch file of the lists cut at s; returns (names, comments, lengths)"""
    lists = [np.asarray(v[:s], np.uint64) for v in lists]
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [800_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    engine.msh_write(path, K, s, names, comments, lengths, lists)
    return names, comments, lengths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a reference file at s = 200, three query files at s = 1000 (queries 0 .. 3, 4 .. 5 and 6)"""
    engine.init()
    d = tmp_path_factory.mktemp("contain_search")
    qs, rs, s_q, s_r, _ = case()
    R = write(d / "ref.msh", "ref", rs, s_r)
    Q = [write(d / ("q%d.msh" % i), "q%d" % i, qs[a:b], s_q) for i, (a, b) in enumerate(((0, 4), (4, 6), (6, 7)))]
    return d, R, Q, [d / "q0.msh", d / "q1.msh", d / "q2.msh"]


def want_rows(R, Q, top, which=0, **bounds):
    shared, n_qry, n_ref = case()[4]
    names = [n for q in Q for n in q[which]]
    sizes = [l for q in Q for l in q[2]]
    return rule.search_text(R[which], names, sizes, shared, n_qry, n_ref, K, top, **bounds)


def test_text_equals_the_rules_rows(files):
    d, R, Q, paths = files
    text = engine.contain_files(d / "ref.msh", paths, top=3)
    want = want_rows(R, Q, 3)
    assert 12 <= len(want) <= 18 and text.count("\n") == len(want)    # queries 0, 1, 2, 5 and 6 have three hits and more, query 4 none
    assert crule.same_rows(crule.rows_of_text(text), want)
    assert [r[0] for r in want[:3]] == [R[0][3], R[0][11], R[0][35]] and want[0][1] == Q[0][0][0]   # best first: the tie by index
    for line in text.splitlines():
        cols = line.split("\t")
        assert len(cols) == 6 and cols[2] == "%g" % float(cols[2]) and cols[3] == "%g" % float(cols[3])
    for top in (1, 64):
        assert crule.same_rows(crule.rows_of_text(engine.contain_files(d / "ref.msh", paths, top=top)), want_rows(R, Q, top))
    # one query file: the same rows for its queries
    assert engine.contain_files(d / "ref.msh", paths[1:2], top=3) == "".join(l + "\n" for l in text.splitlines() if l.split("\t")[1].startswith("q1/"))


def test_the_p_value_drops_rows_and_promotes_none(files):
    """-v acts on the result already chosen: what remains are rows of the unfiltered text, in their order, and no other"""
    d, R, Q, paths = files
    full = engine.contain_files(d / "ref.msh", paths, top=5).splitlines()
    mine = [r for r in crule.rows_of_text("\n".join(full)) if r[1] == Q[2][0][0]]
    assert [(r[4], r[5]) for r in mine] == [(200, 200)] * 3 + [(2, 200), (1, 200)] and mine[3][3] < 1e-6 < mine[4][3] < 1e-3
    cut = engine.contain_files(d / "ref.msh", paths, top=5, max_p_value=1e-6).splitlines()
    assert crule.same_rows(crule.rows_of_text("\n".join(cut)), want_rows(R, Q, 5, max_p_value=1e-6))
    assert 0 < len(cut) < len(full) and cut == [l for l in full if l in cut]
    assert sum(l.split("\t")[1] == Q[2][0][0] for l in cut) == 4    # the fifth row is gone, no sixth-ranked pair in its place


def test_the_identity_acts_before_the_cut(files):
    """-i and -c say what a hit is: with them the list is refilled from the hits that remain"""
    d, R, Q, paths = files
    for bounds in (dict(min_identity=1.0), dict(min_identity=0.9, min_shared=60), dict(min_shared=201), dict(min_identity=1.1)):
        got = crule.rows_of_text(engine.contain_files(d / "ref.msh", paths, top=3, **bounds))
        want = want_rows(R, Q, 3, **bounds)
        assert crule.same_rows(got, want), bounds
        assert (len(want) > 0) == (bounds.get("min_identity", 0) <= 1.0 and bounds.get("min_shared", 1) <= 200)
    # query 0 at min_shared = 60: the 50/50 of the short reference is no hit, and another reference has its row
    q0 = Q[0][0][0]
    rows = [r for r in crule.rows_of_text(engine.contain_files(d / "ref.msh", paths, top=5, min_shared=60)) if r[1] == q0]
    plain = [r for r in crule.rows_of_text(engine.contain_files(d / "ref.msh", paths, top=5)) if r[1] == q0]
    assert [r[0] for r in plain] == [R[0][i] for i in (3, 11, 35, 67, 10)] and plain[4][4:6] == (50, 50)
    assert [r[0] for r in rows[:4]] == [r[0] for r in plain[:4]] and R[0][10] not in [r[0] for r in rows] and all(r[4] >= 60 for r in rows)


def test_comments_in_place_of_names(files):
    d, R, Q, paths = files
    got = crule.rows_of_text(engine.contain_files(d / "ref.msh", paths, top=3, comment=True))
    want = want_rows(R, Q, 3, which=1)
    assert crule.same_rows(got, want) and want[0][:2] == ("ref record 3", "q0 record 0")


def test_bad_options_are_refused(files):
    d, R, Q, paths = files
    for bad in (dict(top=0), dict(top=65), dict(top=3, min_shared=0), dict(top=3, min_identity=float("nan")), dict(top=3, max_p_value=float("nan")),
                dict(top=3, winner=True), dict(top=-1), dict(top=3, min_shared=-1), dict(top=2 ** 32 + 3)):   # (no negative value wraps into a valid one)
        with pytest.raises(engine.EngineError) as exc:
            engine.contain_files(d / "ref.msh", paths, **bad)
        assert exc.value.code == engine.MHX_E_ARG, bad


def test_command_line(files, capsys, tmp_path):
    d, R, Q, paths = files
    ref, q0, q1 = str(d / "ref.msh"), str(paths[0]), str(paths[1])
    assert contain.main(["-n", "3", ref, q0, q1]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q0, q1], top=3)
    assert contain.main(["-n", "5", "-c", "60", "-i", "0.9", "-v", "1e-10", "-C", ref, q0]) == 0
    out = capsys.readouterr().out
    assert out == engine.contain_files(ref, [q0], top=5, min_shared=60, min_identity=0.9, max_p_value=1e-10, comment=True) and out != ""
    # without -n: the call of today, the same bytes
    assert contain.main([ref, q0, q1]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q0, q1])
    assert contain.main(["-i", "0.9", "-C", ref, q1]) == 0
    assert capsys.readouterr().out == engine.contain_files(ref, [q1], min_identity=0.9, comment=True)
    # the refusals: exit 1 and a message, nothing on stdout
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    for argv, word in ((["-n", "3", "-w", ref, q0], "-w"), (["-c", "2", ref, q0], "-n"), (["-n", "3", ref, str(fa)], "genome.fa"), (["-n", "65", ref, q0], "top"),
                       (["-n", "-1", ref, q0], "top"), (["-n", "0", ref, q0], "top"), (["-n", "3", "-c", "-1", ref, q0], "-c"), (["-n", "3", "-c", "0", ref, q0], "-c")):
        assert contain.main(argv) == 1, argv
        err = capsys.readouterr()
        assert err.out == "" and word in err.err, argv

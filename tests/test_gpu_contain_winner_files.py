"""The winner-take-all containment at file level (mhx_contain_files_winner) and through `python -m auriclass_amd.contain -w`,
against the rows of the restated rule (tests/contain_winner_rule.py): names and integers exact, identity and p-value to the
sixth digit.  The `clades` case as sketch files with distinct length fields: the winner rows point to one reference per genome
where the plain rows repeat a clade."""
import numpy as np
import pytest

from auriclass_amd import contain, engine
from oracle import mash_oracle as mo
from tests import contain_cases as cc
from tests import contain_rule as rule
from tests import contain_winner_cases as wc
from tests import contain_winner_rule as wrule

pytestmark = pytest.mark.gpu
K = cc.K


def write(path, prefix, lists, s, lengths, k=K, seed=42):
    lists = [np.asarray(v[:s], np.uint64) for v in lists]
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    if seed == 42:
        engine.msh_write(path, k, s, names, comments, lengths, lists)
    else:
        mo.write_msh(path, mo.SketchFile(kmer_size=k, sketch_size=s, hash_seed=seed,
                                         references=[mo.Reference(n, c, l, h) for n, c, l, h in zip(names, comments, lengths, lists)]))
    return names, comments, lengths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the clades as files: a reference file at s = 200 whose length fields fall with the index, two query files at s = 1000"""
    engine.init()
    d = tmp_path_factory.mktemp("contain_winner")
    qs, rs, s_q, s_r = wc.clades()
    R = write(d / "ref.msh", "ref", rs, s_r, wc.clade_lengths())
    sizes = [900_000 + 1234 * i for i in range(len(qs))]
    Q = [write(d / "q0.msh", "q0", qs[:4], s_q, sizes[:4]), write(d / "q1.msh", "q1", qs[4:], s_q, sizes[4:])]
    return d, R, Q


@pytest.fixture(scope="module")
def expected():
    Q, q_len, R, r_len, s_q, s_r, _ = wc.rows_of("clades")
    return wrule.matrix_of_rows(Q, q_len, R, r_len, s_q, s_r, wc.clade_lengths())


def want_rows(R, Q, expected, which=0, **bounds):
    won, shared, n_qry, n_ref = expected[:4]
    names = [n for q in Q for n in q[which]]
    sizes = [l for q in Q for l in q[2]]
    return wrule.expected_rows(R[which], names, sizes, won, n_qry, n_ref, K, **bounds)


def test_winner_rows_equal_the_rule(files, expected, capsys):
    d, R, Q = files
    ref, paths = d / "ref.msh", [d / "q0.msh", d / "q1.msh"]
    text = engine.contain_files(ref, paths, winner=True)
    want = want_rows(R, Q, expected)
    assert len(want) == 7 * 14 and text.count("\n") == len(want)
    assert rule.same_rows(rule.rows_of_text(text), want)
    assert contain.main(["-w", str(ref)] + [str(p) for p in paths]) == 0
    assert capsys.readouterr().out == text
    # the falling lengths send every tie where the index sends it: the same integers as without lengths
    assert np.array_equal(expected[0], wc.expected("clades")[0])
    # -i 0.9 leaves exactly the rule's rows: one per single-genome query, two for the mixed culture (the unrelated genome: none)
    cut = want_rows(R, Q, expected, min_identity=0.9)
    per_query = [sum(1 for r in cut if r[1] == n) for q in Q for n in q[0]]
    assert per_query == [1, 1, 1, 2, 1, 1, 0]
    assert contain.main(["-w", "-i", "0.9", str(ref)] + [str(p) for p in paths]) == 0
    out = capsys.readouterr().out
    assert out == engine.contain_files(ref, paths, winner=True, min_identity=0.9)
    assert rule.same_rows(rule.rows_of_text(out), cut)
    # -v filters on the winner values too, and -C prints the comments
    cut = want_rows(R, Q, expected, 1, max_p_value=1e-10)
    assert 0 < len(cut) < len(want)
    assert rule.same_rows(rule.rows_of_text(engine.contain_files(ref, paths, winner=True, max_p_value=1e-10, comment=True)), cut)


def test_without_w_the_bytes_are_the_plain_call(files, capsys):
    d, R, Q = files
    ref, paths = d / "ref.msh", [d / "q0.msh", d / "q1.msh"]
    plain = engine.contain_files(ref, paths)
    assert plain == engine.contain_files(ref, paths, winner=False)
    shared, n_qry, n_ref = wc.expected("clades")[1:4]
    names = [n for q in Q for n in q[0]]
    sizes = [l for q in Q for l in q[2]]
    assert rule.same_rows(rule.rows_of_text(plain), rule.expected_rows(R[0], names, sizes, shared, n_qry, n_ref, K))
    assert contain.main([str(ref)] + [str(p) for p in paths]) == 0
    assert capsys.readouterr().out == plain
    assert plain != engine.contain_files(ref, paths, winner=True)


def test_mismatch_is_refused(files, tmp_path):
    d, R, Q = files
    qs = wc.clades()[0]
    write(tmp_path / "k19.msh", "k19", qs[:3], 1000, [1, 2, 3], k=19)
    with pytest.raises(engine.EngineError) as exc:
        engine.contain_files(d / "ref.msh", [d / "q0.msh", tmp_path / "k19.msh"], winner=True)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    write(tmp_path / "seed7.msh", "seed7", qs[:3], 1000, [1, 2, 3], seed=7)
    with pytest.raises(engine.EngineError) as exc:
        engine.contain_files(d / "ref.msh", [tmp_path / "seed7.msh"], winner=True)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different hash seeds" in exc.value.message
    with pytest.raises(engine.EngineError) as exc:
        engine.contain_files(d / "ref.msh", [d / "q0.msh"], winner=True, min_identity=float("nan"))
    assert exc.value.code == engine.MHX_E_ARG

"""The reference-set search at file level (mhx_search_files) and through `python -m auriclass_amd.search`, against the rows
of the restated rule (tests/search_rule.py) byte for byte, formatted as the oracle's dist_text formats them."""
import numpy as np
import pytest

from auriclass_amd import engine, search
from oracle import mash_oracle as mo
from tests import search_cases as sc
from tests import search_rule as rule

pytestmark = pytest.mark.gpu
K, S = sc.K, 1000


def write(path, prefix, lists, k=K, s=S):
    """one sketch file through engine.msh_write, and the same as the oracle's SketchFile"""
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [800_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    engine.msh_write(path, k, s, names, comments, lengths, lists)
    return mo.SketchFile(k, s, [mo.Reference(n, c, l, np.asarray(h, np.uint64)) for n, c, l, h in zip(names, comments, lengths, lists)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("search")
    refs, _ = sc.references()
    qs = sc.queries()
    R = {"a": write(d / "ref_a.msh", "a", refs[:70]),                      # three slices, the last of 6; the empty reference 33
         "b": write(d / "ref_b.msh", "b", refs[100:200])}                  # the duplicates 141, 190, 191, 196
    Q = [write(d / "q0.msh", "q0", qs[0:9]), write(d / "q1.msh", "q1", qs[22:30]), write(d / "q2.msh", "q2", qs[9:12] + qs[40:43])]
    return d, R, Q


@pytest.mark.parametrize("which", ["a", "b"])
def test_text_equals_the_rules_rows(files, which):
    d, R, Q = files
    paths = [d / "q0.msh", d / "q1.msh", d / "q2.msh"]
    ref = d / ("ref_%s.msh" % which)
    for top, max_dist in ((5, 1.0), (3, 0.05), (64, 0.2), (1, 0.0)):
        want = rule.search_text(R[which], Q, top, max_dist)
        assert engine.search_files(ref, paths, top=top, max_dist=max_dist) == want
        assert (max_dist == 1.0) == (want.count("\n") == top * 23)   # below 1 some queries have short or empty lists
    assert engine.search_files(ref, paths[1:2]) == rule.search_text(R[which], Q[1:2])   # the defaults: top 5, everything
    # the p-value bound drops rows from the lists already chosen and promotes nothing
    full, cut = rule.search_text(R[which], Q, 5, 1.0), rule.search_text(R[which], Q, 5, 1.0, 1e-10)
    assert 0 < cut.count("\n") < full.count("\n") and set(cut.splitlines()) <= set(full.splitlines())
    assert engine.search_files(ref, paths, top=5, max_p_value=1e-10) == cut


def test_query_files_across_the_batch_of_4096_sketches(tmp_path):
    """query files of 3000, 1200 and 50 sketches at s = 16 (tests/search_cases.py: batch_boundary): the first batch goes to the
    device behind file 1 with 4200 sketches, the last holds file 2 alone.  The text is that of the three files one by one."""
    engine.init()
    refs, files = sc.batch_boundary()
    write(tmp_path / "ref.msh", "r", refs, s=16)
    paths = [tmp_path / ("q%d.msh" % i) for i in range(3)]
    for i, lists in enumerate(files):
        write(paths[i], "q%d" % i, lists, s=16)
    assert len(files[0]) < 4096 <= len(files[0]) + len(files[1])
    for top, max_dist in ((5, 1.0), (2, 0.05)):
        one_by_one = [engine.search_files(tmp_path / "ref.msh", [p], top=top, max_dist=max_dist) for p in paths]
        assert all(t.count("\n") > 0 for t in one_by_one)
        assert engine.search_files(tmp_path / "ref.msh", paths, top=top, max_dist=max_dist) == "".join(one_by_one)
    assert one_by_one[0].count("\n") < 2 * len(files[0])   # the bound leaves most lists empty


def test_mismatch_is_refused(files, tmp_path):
    d, R, Q = files
    write(tmp_path / "k19.msh", "k19", sc.queries()[:3], k=19)
    with pytest.raises(engine.EngineError) as exc:
        engine.search_files(d / "ref_a.msh", [d / "q0.msh", tmp_path / "k19.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    write(tmp_path / "s300.msh", "s300", [q[:300] for q in sc.queries()[:3]], s=300)
    with pytest.raises(engine.EngineError) as exc:
        engine.search_files(d / "ref_a.msh", [d / "q0.msh", tmp_path / "s300.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    for bad in (dict(top=0), dict(top=65), dict(max_dist=float("nan"))):
        with pytest.raises(engine.EngineError) as exc:
            engine.search_files(d / "ref_a.msh", [d / "q0.msh"], **bad)
        assert exc.value.code == engine.MHX_E_ARG


def test_a_reference_file_that_fails_fails_the_call_as_it_fails_dist_files(files, tmp_path):
    d, R, Q = files
    bad = mo.SketchFile(K, S, [mo.Reference("x", "", 1000, np.asarray(sc.queries()[0][::-1].copy()))])
    mo.write_msh(tmp_path / "descending.msh", bad)
    (tmp_path / "garbage.msh").write_bytes(b"not a sketch file at all" * 10)
    for ref in (tmp_path / "missing.msh", tmp_path / "descending.msh", tmp_path / "garbage.msh"):
        with pytest.raises(engine.EngineError) as want:
            engine.dist_files(ref, d / "q0.msh")
        with pytest.raises(engine.EngineError) as got:
            engine.search_files(ref, [d / "q0.msh"])
        assert got.value.code == want.value.code, ref


def test_command_line_prints_the_same_bytes(files, capsys, tmp_path):
    d, R, Q = files
    ref, q0, q1 = str(d / "ref_b.msh"), str(d / "q0.msh"), str(d / "q1.msh")
    assert search.main([ref, q0, q1]) == 0
    assert capsys.readouterr().out == rule.search_text(R["b"], Q[:2])
    assert search.main(["-n", "3", "-d", "0.05", "-v", "1e-10", "-p", "8", ref, q1]) == 0
    assert capsys.readouterr().out == rule.search_text(R["b"], Q[1:2], 3, 0.05, 1e-10)
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    assert search.main([ref, str(fa)]) == 1
    out = capsys.readouterr()
    assert out.out == "" and "sketch" in out.err and "genome.fa" in out.err
    assert search.main([ref, str(tmp_path / "missing.msh")]) == 1
    assert capsys.readouterr().out == ""

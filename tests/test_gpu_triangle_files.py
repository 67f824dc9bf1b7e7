"""`mash triangle` at file level (mhx_triangle_files) and through the shim, against the restated rule of
tests/triangle_rule.py byte for byte, and its edge rows against the `mash dist` rows of the same pairs from
mhx_dist_files_multi."""
import numpy as np
import pytest

from auriclass_amd import engine, mash_shim
from oracle import mash_oracle as mo
from tests import triangle_cases as tc
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu


def sketch_file(seed, n, k=21, s=400):
    rng = np.random.default_rng(seed)
    base = tc.sketch_like(rng, s)
    lists = [base if i == 0 else (tc.mutate(rng, base, 0.02 * i) if i % 3 else tc.sketch_like(rng, s)) for i in range(n)]
    if n > 4:
        lists[4] = lists[1].copy()
        lists[2] = lists[2][:57]
    refs = [mo.Reference("set%d/ref%d.fasta" % (seed, i), "genome %d of set %d" % (i, seed), 900_000 + 12_345 * i + seed, h)
            for i, h in enumerate(lists)]
    return mo.SketchFile(k, s, refs)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("triangle")
    A, B = sketch_file(12, 12), sketch_file(5, 5)
    # the second file holds near copies of the first one's base as well: pairs across the files are not all unrelated
    B.references[3].hashes = tc.mutate(np.random.default_rng(1), A.references[0].hashes, 0.05)
    mo.write_msh(d / "a.msh", A)
    mo.write_msh(d / "b.msh", B)
    F = tr.combine([A, B])
    mo.write_msh(d / "all.msh", F)
    return d, F


def test_matrix_and_edge_list_equal_the_rule(files):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    assert engine.triangle_files(paths) == tr.matrix_text(F)
    assert engine.triangle_files(paths, comment=True) == tr.matrix_text(F, comment=True)
    assert engine.triangle_files(paths, edge=True) == tr.edge_text(F)
    filtered = tr.edge_text(F, 0.1, 1e-5)
    assert 0 < filtered.count("\n") < 17 * 16 // 2
    assert engine.triangle_files(paths, edge=True, max_dist=0.1, max_p_value=1e-5) == filtered
    assert engine.triangle_files(paths, max_dist=0.1) == tr.edge_text(F, 0.1, 1.0)   # -d implies -E
    assert engine.triangle_files([d / "all.msh"]) == tr.matrix_text(F)


def test_edge_rows_are_the_dist_rows_of_the_same_pairs(files):
    d, F = files
    n = len(F.references)
    rows = engine.dist_files_multi(d / "all.msh", [d / "all.msh"]).splitlines(keepends=True)
    assert len(rows) == n * n
    want = "".join(rows[j * n + i] for i in range(n) for j in range(i))   # reference i, query j < i
    assert engine.triangle_files([d / "a.msh", d / "b.msh"], edge=True) == want


def test_mismatch_and_damage_are_refused(files, tmp_path):
    d, F = files
    other = sketch_file(3, 3, k=19)
    mo.write_msh(tmp_path / "k19.msh", other)
    with pytest.raises(engine.EngineError) as exc:
        engine.triangle_files([d / "a.msh", tmp_path / "k19.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    size = sketch_file(3, 3, s=300)
    mo.write_msh(tmp_path / "s300.msh", size)
    with pytest.raises(engine.EngineError) as exc:
        engine.triangle_files([d / "a.msh", tmp_path / "s300.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    bad = sketch_file(4, 4)
    bad.references[2].hashes = bad.references[2].hashes[::-1].copy()
    mo.write_msh(tmp_path / "descending.msh", bad)
    with pytest.raises(engine.EngineError) as exc:
        engine.triangle_files([d / "a.msh", tmp_path / "descending.msh"])
    assert exc.value.code == engine.MHX_E_FORMAT and "not ascending" in exc.value.message


def test_shim(files, capsys, tmp_path):
    d, F = files
    a, b = str(d / "a.msh"), str(d / "b.msh")
    assert mash_shim.main(["triangle", a, b]) == 0
    assert capsys.readouterr().out == tr.matrix_text(F)
    assert mash_shim.main(["triangle", "-p", "8", "-E", "-d", "0.1", "-v", "1e-5", a, b]) == 0
    assert capsys.readouterr().out == tr.edge_text(F, 0.1, 1e-5)
    assert mash_shim.main(["triangle", "-C", a, b]) == 0
    assert capsys.readouterr().out == tr.matrix_text(F, comment=True)
    assert mash_shim.main(["triangle", "-k", "21", a]) == 1
    out = capsys.readouterr()
    assert out.out == "" and "-k" in out.err
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    assert mash_shim.main(["triangle", a, str(fa)]) == 1
    out = capsys.readouterr()
    assert out.out == "" and "mash sketch" in out.err and "genome.fa" in out.err
    assert "triangle" in mash_shim.USAGE

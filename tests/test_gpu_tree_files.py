"""The single-linkage tree at file level (mhx_tree_files, python -m auriclass_amd.tree) against the restated rules of
tests/mst_rule.py and tests/tree_rule.py byte for byte: the merge table and the Newick dendrogram from sketch files written
by the test, with comments, one reference alone, refusals, and the command line."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import engine, tree
from oracle import mash_oracle as mo
from tests import tree_rule as tl
from tests import triangle_cases as tc
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu


def sketch_file(seed, n, k=21, s=400):
    """a base, near copies of it at many distances, independent lists, an exact duplicate and a short list; names that need
    quoting in Newick among them"""
    rng = np.random.default_rng(seed)
    base = tc.sketch_like(rng, s)
    lists = [base if i == 0 else (tc.mutate(rng, base, 0.02 * i) if i % 3 else tc.sketch_like(rng, s)) for i in range(n)]
    if n > 4:
        lists[4] = lists[1].copy()
        lists[2] = lists[2][:57]
    names = ["set%d/ref%d.fasta" % (seed, i) for i in range(n)]
    if n > 3:
        names[1] = "it's (a) name.fa"
        names[3] = "a,b:c;[d]"
    refs = [mo.Reference(names[i], "genome %d of set %d" % (i, seed), 900_000 + 12_345 * ((7 * i + 3) % 16) + seed, h) for i, h in enumerate(lists)]
    return mo.SketchFile(k, s, refs)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("tree")
    A, B = sketch_file(12, 12), sketch_file(5, 5)
    B.references[3].hashes = tc.mutate(np.random.default_rng(1), A.references[0].hashes, 0.05)
    B.references[0].hashes = A.references[6].hashes.copy()
    mo.write_msh(d / "a.msh", A)
    mo.write_msh(d / "b.msh", B)
    return d, tr.combine([A, B])


def test_merge_table_equals_the_rule(files):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    want = tl.table_text(F)
    rows = [r.split("\t") for r in want.splitlines()]
    assert len(rows) == len(F.references) - 1 and [int(r[5]) for r in rows] == list(range(len(rows), 0, -1))
    assert rows[0][2] == "0" and rows[-1][2] == "1"   # duplicates merge first, independent lists last
    assert engine.tree_files(paths) == want
    assert engine.tree_files(paths, comment=True) == tl.table_text(F, comment=True)
    assert engine.tree_files([d / "b.msh"]) == tl.table_text(mo.read_msh(d / "b.msh"))


def test_newick_equals_the_rule(files):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    want = tl.newick_text(F)
    assert want.endswith(");\n") and "'it''s (a) name.fa'" in want and "'a,b:c;[d]'" in want
    assert engine.tree_files(paths, newick=True) == want
    assert engine.tree_files(paths, newick=True, comment=True) == tl.newick_text(F, comment=True)


def test_one_reference_alone(files, tmp_path):
    one = sketch_file(9, 1)
    mo.write_msh(tmp_path / "one.msh", one)
    assert engine.tree_files([tmp_path / "one.msh"]) == ""
    assert engine.tree_files([tmp_path / "one.msh"], newick=True) == "set9/ref0.fasta;\n"
    two = sketch_file(9, 2)
    mo.write_msh(tmp_path / "two.msh", two)
    assert engine.tree_files([tmp_path / "two.msh"], newick=True) == tl.newick_text(two)
    assert engine.tree_files([tmp_path / "two.msh"]) == tl.table_text(two)


def test_mismatch_and_damage_are_refused(files, tmp_path):
    d, F = files
    mo.write_msh(tmp_path / "k19.msh", sketch_file(3, 3, k=19))
    with pytest.raises(engine.EngineError) as exc:
        engine.tree_files([d / "a.msh", tmp_path / "k19.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    other = sketch_file(3, 3)
    mo.write_msh(tmp_path / "seed7.msh", mo.SketchFile(kmer_size=other.kmer_size, sketch_size=other.sketch_size, references=other.references, hash_seed=7))
    for newick in (False, True):
        with pytest.raises(engine.EngineError) as exc:
            engine.tree_files([d / "a.msh", tmp_path / "seed7.msh"], newick=newick)
        assert exc.value.code == engine.MHX_E_MISMATCH and "different hash seeds" in exc.value.message
    mo.write_msh(tmp_path / "s300.msh", sketch_file(3, 3, s=300))
    with pytest.raises(engine.EngineError) as exc:
        engine.tree_files([d / "a.msh", tmp_path / "s300.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    bad = sketch_file(4, 4)
    bad.references[2].hashes = bad.references[2].hashes[::-1].copy()
    mo.write_msh(tmp_path / "descending.msh", bad)
    with pytest.raises(engine.EngineError) as exc:
        engine.tree_files([d / "a.msh", tmp_path / "descending.msh"], newick=True)
    assert exc.value.code == engine.MHX_E_FORMAT and "not ascending" in exc.value.message
    (tmp_path / "cut.msh").write_bytes((d / "a.msh").read_bytes()[:100])
    with pytest.raises(engine.EngineError) as exc:
        engine.tree_files([tmp_path / "cut.msh"])
    assert exc.value.code in (engine.MHX_E_FORMAT, engine.MHX_E_IO)
    opts = engine.TreeOpts(4, 0, 0)
    arr = (ctypes.c_char_p * 1)(str(d / "a.msh").encode())
    need = ctypes.c_size_t(0)
    assert engine.load().mhx_tree_files(arr, 1, ctypes.byref(opts), None, 0, ctypes.byref(need)) == engine.MHX_E_ARG


def test_command_line(files, capsys, tmp_path):
    d, F = files
    a, b = str(d / "a.msh"), str(d / "b.msh")
    assert tree.main([a, b]) == 0
    assert capsys.readouterr().out == tl.table_text(F)
    assert tree.main(["-p", "8", "-C", "--newick", a, b]) == 0
    assert capsys.readouterr().out == tl.newick_text(F, comment=True)
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    assert tree.main([a, str(fa)]) == 1
    res = capsys.readouterr()
    assert res.out == "" and "mash sketch" in res.err and "genome.fa" in res.err
    assert tree.main([str(tmp_path / "missing.msh")]) == 1
    assert capsys.readouterr().out == ""
    assert tree.main([]) == 1

"""Complete and average linkage at file level (mhx_linkage_files, python -m auriclass_amd.tree / auriclass_amd.cluster with
--linkage) against text built from the rule of tests/linkage_rule.py byte for byte: the merge table, the Newick dendrogram and
the cut with its representatives file, refusals, and both command lines -- where --linkage single prints what the call without
the flag prints."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import cluster, engine, tree
from oracle import mash_oracle as mo
from tests import linkage_rule as lr
from tests import triangle_cases as tc
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu
BOUND = 0.05
LINKAGES = [("complete", lr.COMPLETE), ("average", lr.AVERAGE)]


def sketch_file(seed, n, k=21, s=400):
    """as in tests/test_gpu_tree_files.py: a base, near copies of it at many distances, independent lists, an exact duplicate and
    a short list; names that need quoting in Newick among them; genome lengths NOT in index order"""
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
    d = tmp_path_factory.mktemp("linkage")
    A, B = sketch_file(12, 12), sketch_file(5, 5)
    B.references[3].hashes = tc.mutate(np.random.default_rng(1), A.references[0].hashes, 0.05)
    B.references[0].hashes = A.references[6].hashes.copy()
    mo.write_msh(d / "a.msh", A)
    mo.write_msh(d / "b.msh", B)
    return d, tr.combine([A, B])


@pytest.mark.parametrize("name,linkage", LINKAGES)
def test_merge_table_and_newick_equal_the_rule(files, name, linkage):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    want = lr.table_text(F, linkage)
    rows = [r.split("\t") for r in want.splitlines()]
    assert len(rows) == len(F.references) - 1 and [int(r[4]) for r in rows] == list(range(len(rows), 0, -1))
    assert rows[0][2] == "0" and int(rows[-1][3]) == len(F.references)
    assert engine.linkage_files(paths, name) == want
    assert engine.linkage_files(paths, name, comment=True) == lr.table_text(F, linkage, comment=True)
    newick = lr.newick_text(F, linkage)
    assert newick.endswith(");\n") and "'it''s (a) name.fa'" in newick
    assert engine.linkage_files(paths, name, mode="newick") == newick
    assert engine.linkage_files(paths, name, mode="newick", comment=True) == lr.newick_text(F, linkage, comment=True)


@pytest.mark.parametrize("name,linkage", LINKAGES)
def test_cut_and_representatives_equal_the_rule(files, tmp_path, name, linkage):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    first = lr.cut_text(F, linkage, BOUND)
    clusters = int(first.splitlines()[-1].split("\t")[0])
    assert 1 < clusters < len(F.references)
    assert engine.linkage_files(paths, name, mode="cut", max_dist=BOUND) == first
    assert engine.linkage_files(paths, name, mode="cut", max_dist=BOUND, rep="longest", comment=True) == lr.cut_text(F, linkage, BOUND, comment=True, rep="longest")
    for bound in (-1.0, 0.0, 0.2, 1.0):
        assert engine.linkage_files(paths, name, mode="cut", max_dist=bound) == lr.cut_text(F, linkage, bound)
    out = tmp_path / "reps.msh"
    assert engine.linkage_files(paths, name, mode="cut", max_dist=BOUND, rep="longest", out=out) == lr.cut_text(F, linkage, BOUND, rep="longest")
    reps = [r for _, r in lr.cut_clusters(F, linkage, BOUND, "longest")]
    assert out.read_bytes() == mo.msh_bytes(mo.SketchFile(F.kmer_size, F.sketch_size, [F.references[i] for i in reps]))


def test_one_reference_and_refusals(files, tmp_path):
    d, F = files
    one = sketch_file(9, 1)
    mo.write_msh(tmp_path / "one.msh", one)
    assert engine.linkage_files([tmp_path / "one.msh"], "average") == ""
    assert engine.linkage_files([tmp_path / "one.msh"], "average", mode="newick") == "set9/ref0.fasta;\n"
    assert engine.linkage_files([tmp_path / "one.msh"], "complete", mode="cut", max_dist=0.1) == "1\t1\tset9/ref0.fasta\tset9/ref0.fasta\n"
    mo.write_msh(tmp_path / "k19.msh", sketch_file(3, 3, k=19))
    with pytest.raises(engine.EngineError) as exc:
        engine.linkage_files([d / "a.msh", tmp_path / "k19.msh"], "complete")
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    with pytest.raises(engine.EngineError) as exc:
        engine.linkage_files([d / "a.msh"], "complete", mode="cut", max_dist=float("nan"))
    assert exc.value.code == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as exc:
        engine.linkage_files([d / "a.msh"], "complete", mode="merges", out=tmp_path / "never.msh")
    assert exc.value.code == engine.MHX_E_ARG and not (tmp_path / "never.msh").exists()
    for bad in ("single", "ward"):
        with pytest.raises(ValueError):
            engine.linkage_files([d / "a.msh"], bad)
    counted = sketch_file(6, 4)
    counted.references[1].counts = np.full(len(counted.references[1].hashes), 3, np.uint32)
    mo.write_msh(tmp_path / "counted.msh", counted)
    with pytest.raises(engine.EngineError) as exc:
        engine.linkage_files([tmp_path / "counted.msh"], "complete", mode="cut", max_dist=BOUND, out=tmp_path / "never.msh")
    assert exc.value.code == engine.MHX_E_ARG and "multiplicity counts" in exc.value.message and not (tmp_path / "never.msh").exists()
    arr = (ctypes.c_char_p * 1)(str(d / "a.msh").encode())
    need = ctypes.c_size_t(0)
    for opts in (engine.LinkageOpts(24, 0, 1, 0, 0, 1.0), engine.LinkageOpts(32, 0, 0, 0, 0, 1.0), engine.LinkageOpts(32, 0, 3, 0, 0, 1.0),
                 engine.LinkageOpts(32, 0, 1, 3, 0, 1.0), engine.LinkageOpts(32, 0, 1, 2, 2, 1.0)):
        assert engine.load().mhx_linkage_files(arr, 1, ctypes.byref(opts), None, None, 0, ctypes.byref(need)) == engine.MHX_E_ARG


def test_command_lines(files, capsys, tmp_path):
    d, F = files
    a, b = str(d / "a.msh"), str(d / "b.msh")
    for name, linkage in LINKAGES:
        assert tree.main(["--linkage", name, a, b]) == 0
        assert capsys.readouterr().out == lr.table_text(F, linkage)
        assert tree.main(["-C", "--newick", "--linkage", name, a, b]) == 0
        assert capsys.readouterr().out == lr.newick_text(F, linkage, comment=True)
        out = tmp_path / f"{name}.msh"
        assert cluster.main(["-d", str(BOUND), "--linkage", name, "--rep", "longest", "-o", str(out), a, b]) == 0
        assert capsys.readouterr().out == lr.cut_text(F, linkage, BOUND, rep="longest")
        assert out.exists()
    # the default is today's call, byte for byte
    for argv in ([a, b], ["--newick", "-C", a, b]):
        assert tree.main(argv) == 0
        plain = capsys.readouterr().out
        assert tree.main(["--linkage", "single"] + argv) == 0
        assert capsys.readouterr().out == plain and plain
    for argv in (["-d", str(BOUND), a, b], ["-d", "0.2", "--rep", "longest", "-C", a, b]):
        assert cluster.main(argv) == 0
        plain = capsys.readouterr().out
        assert cluster.main(["--linkage", "single"] + argv) == 0
        assert capsys.readouterr().out == plain and plain
    assert tree.main(["--linkage", "ward", a]) == 1
    capsys.readouterr()

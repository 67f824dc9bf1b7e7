"""Neighbour joining at file level (mhx_nj_files, python -m auriclass_amd.tree --nj) against text built from the rule of
tests/nj_rule.py byte for byte: the table of joins and the unrooted Newick tree of the `short` and tiny(33) sets written as
sketch files, with names and with comments, two files as one set, the refusal of --nj with a linkage, and the command line
without --nj, which prints what it printed before."""
import pytest

from auriclass_amd import engine, tree
from oracle import mash_oracle as mo
from tests import linkage_rule as lr
from tests import nj_cases as nc
from tests import nj_rule as nr
from tests import tree_rule as tl
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu


def sketch_file(name, args, tag):
    """a case set as a sketch file; names that need quoting in Newick among them"""
    lists, s = nc.lists_of(name, args)
    names = ["%s/ref%d.fasta" % (tag, i) for i in range(len(lists))]
    names[1] = "it's (a) name.fa"
    names[3] = "a,b:c;[d]"
    refs = [mo.Reference(names[i], "genome %d of %s" % (i, tag), 900_000 + 12_345 * ((7 * i + 3) % 16), h) for i, h in enumerate(lists)]
    return mo.SketchFile(nc.K, s, refs)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("nj")
    out = {}
    for tag, name, args in (("short", "short", ()), ("tiny33", "tiny", (33,))):
        F = sketch_file(name, args, tag)
        mo.write_msh(d / (tag + ".msh"), F)
        out[tag] = (d / (tag + ".msh"), F)
    return out


@pytest.mark.parametrize("tag", ["short", "tiny33"])
def test_table_and_newick_equal_the_rule(files, tag, capsys):
    path, F = files[tag]
    n = len(F.references)
    want = nr.table_text(F)
    rows = [r.split("\t") for r in want.splitlines()]
    assert len(rows) == n - 1 and [int(r[5]) for r in rows] == list(range(n - 1, 0, -1)) and rows[-1][3] == "0"
    assert engine.nj_files([path]) == want
    assert engine.nj_files([path], comment=True) == nr.table_text(F, comment=True)
    newick = nr.newick_text(F)
    assert newick.endswith(");\n") and "'it''s (a) name.fa'" in newick and newick.count("(") == n - 2 + 1   # one per join that is a node, and the one in the quoted name
    assert engine.nj_files([path], newick=True) == newick
    assert engine.nj_files([path], newick=True, comment=True) == nr.newick_text(F, comment=True)
    for argv, text in ((["--nj"], want), (["--nj", "-C"], nr.table_text(F, comment=True)), (["--nj", "--newick"], newick),
                       (["--newick", "-C", "--nj"], nr.newick_text(F, comment=True)), (["--nj", "--linkage", "single"], want)):
        assert tree.main(argv + [str(path)]) == 0
        assert capsys.readouterr().out == text


def test_two_files_form_one_set(files):
    (a, A), (b, B) = files["short"], files["tiny33"]
    F = tr.combine([A, B])
    assert engine.nj_files([a, b]) == nr.table_text(F)
    assert engine.nj_files([a, b], newick=True, comment=True) == nr.newick_text(F, comment=True)


def test_one_and_two_references(files, tmp_path):
    _, F = files["short"]
    for n, newick in ((1, "short/ref4.fasta;\n"), (2, None)):
        G = mo.SketchFile(F.kmer_size, F.sketch_size, F.references[4:4 + n])
        mo.write_msh(tmp_path / "few.msh", G)
        assert engine.nj_files([tmp_path / "few.msh"]) == nr.table_text(G)
        got = engine.nj_files([tmp_path / "few.msh"], newick=True)
        assert got == nr.newick_text(G) and (newick is None or got == newick)
        if n == 2:
            assert got.startswith("(short/ref4.fasta:0,short/ref5.fasta:") and nr.table_text(G).count("\n") == 1


def test_refusals_and_the_tree_without_the_flag(files, capsys, tmp_path):
    path, F = files["tiny33"]
    for linkage in ("average", "complete"):
        assert tree.main(["--nj", "--linkage", linkage, str(path)]) == 1
        out = capsys.readouterr()
        assert out.out == "" and "--nj" in out.err
    # without --nj: today's bytes
    assert tree.main([str(path)]) == 0
    assert capsys.readouterr().out == tl.table_text(F)
    assert tree.main(["--newick", "-C", str(path)]) == 0
    assert capsys.readouterr().out == tl.newick_text(F, comment=True)
    assert tree.main(["--linkage", "average", str(path)]) == 0
    assert capsys.readouterr().out == lr.table_text(F, lr.AVERAGE)
    mo.write_msh(tmp_path / "k19.msh", mo.SketchFile(19, F.sketch_size, F.references[:3]))
    with pytest.raises(engine.EngineError) as exc:
        engine.nj_files([path, tmp_path / "k19.msh"])
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    assert tree.main(["--nj", str(tmp_path / "missing.msh")]) == 1
    capsys.readouterr()

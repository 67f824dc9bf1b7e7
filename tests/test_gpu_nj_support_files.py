"""Jackknife support at file level (mhx_nj_files_opts, python -m auriclass_amd.tree --nj --support R) against the text of the
rule (tests/nj_support_rule.py) byte for byte: the table with its seventh column and the Newick tree with its labels, no
replicates printing what mhx_nj_files prints, and the command line's flags and refusals."""
import ctypes

import pytest

from auriclass_amd import engine, tree
from tests import nj_rule as nr
from tests import nj_support_rule as ns
from tests.test_gpu_nj_files import sketch_file
from tests.test_nj_support_rule import small_file
from oracle import mash_oracle as mo

pytestmark = pytest.mark.gpu
R = 5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("nj_support")
    out = {}
    for tag, F in (("small", small_file()), ("short", sketch_file("short", (), "short"))):
        mo.write_msh(d / (tag + ".msh"), F)
        out[tag] = (d / (tag + ".msh"), F)
    return out


@pytest.mark.parametrize("tag", ["small", "short"])
def test_table_and_newick_equal_the_rule(files, tag):
    path, F = files[tag]
    n = len(F.references)
    table = ns.table_text(F, R, 0.5, 42)
    assert table.count("\n") == n - 1 and all(row.endswith("/%d" % R) for row in table.splitlines())
    assert engine.nj_files([path], replicates=R) == table
    assert engine.nj_files([path], comment=True, replicates=R) == ns.table_text(F, R, 0.5, 42, comment=True)
    newick = ns.newick_text(F, R, 0.5, 42)
    assert newick != nr.newick_text(F) and newick.endswith(");\n")
    assert engine.nj_files([path], newick=True, replicates=R) == newick
    assert engine.nj_files([path], newick=True, comment=True, replicates=R) == ns.newick_text(F, R, 0.5, 42, comment=True)
    # another seed and another keep rate are another jackknife
    assert engine.nj_files([path], replicates=R, keep=0.25, seed=7) == ns.table_text(F, R, 0.25, 7)


def test_no_replicates_print_todays_bytes(files):
    path, F = files["small"]
    lib = engine.load()
    for comment in (False, True):
        for newick in (False, True):
            today = engine.nj_files([path], comment=comment, newick=newick)
            assert today == (nr.newick_text(F, comment) if newick else nr.table_text(F, comment))
            assert engine.nj_files([path], comment=comment, newick=newick, replicates=0) == today
            # mhx_nj_files_opts itself with replicates == 0, and without options
            arr = (ctypes.c_char_p * 1)(str(path).encode())
            opts = engine.NjOpts(ctypes.sizeof(engine.NjOpts), int(comment), int(newick), 0, 0.5, 42)
            assert engine._text_call(lambda buf, cap, need: lib.mhx_nj_files_opts(arr, 1, ctypes.byref(opts), buf, cap, need)) == today
    arr = (ctypes.c_char_p * 1)(str(path).encode())
    assert engine._text_call(lambda buf, cap, need: lib.mhx_nj_files_opts(arr, 1, None, buf, cap, need)) == nr.table_text(F)
    # refused before a file is read
    need = ctypes.c_size_t(0)
    for opts in (engine.NjOpts(8, 0, 0, 0, 0.5, 42), engine.NjOpts(ctypes.sizeof(engine.NjOpts), 0, 0, 3, 0.0, 42),
                 engine.NjOpts(ctypes.sizeof(engine.NjOpts), 0, 0, 3, float("nan"), 42), engine.NjOpts(ctypes.sizeof(engine.NjOpts), 0, 0, 10001, 0.5, 42)):
        missing = (ctypes.c_char_p * 1)(b"missing.msh")
        assert lib.mhx_nj_files_opts(missing, 1, ctypes.byref(opts), None, 0, ctypes.byref(need)) == engine.MHX_E_ARG


def test_the_command_line(files, capsys):
    path, F = files["small"]
    table, newick = ns.table_text(F, R, 0.5, 42), ns.newick_text(F, R, 0.5, 42)
    for argv, text in ((["--nj", "--support", str(R)], table), (["--nj", "--newick", "--support", str(R)], newick),
                       (["--nj", "--support", str(R), "--keep", "0.5", "--seed", "42", "-C"], ns.table_text(F, R, 0.5, 42, comment=True)),
                       (["--nj", "--support", str(R), "--keep", "0.25", "--seed", "7"], ns.table_text(F, R, 0.25, 7)),
                       (["--nj", "--support", "0"], nr.table_text(F)), (["--nj", "--support", "0", "--newick"], nr.newick_text(F)),
                       (["--nj"], nr.table_text(F))):
        assert tree.main(argv + [str(path)]) == 0, argv
        assert capsys.readouterr().out == text, argv
    for argv in (["--support", "3"], ["--support", "0"], ["--linkage", "average", "--support", "3"]):
        assert tree.main(argv + [str(path)]) == 1
        out = capsys.readouterr()
        assert out.out == "" and "--support" in out.err and "--nj" in out.err
    for argv in (["--nj", "--support", "-1"], ["--nj", "--support", "3", "--keep", "0"], ["--nj", "--support", "3", "--keep", "1.5"],
                 ["--nj", "--support", "10001"], ["--nj", "--support", "x"]):
        assert tree.main(argv + [str(path)]) == 1, argv
        out = capsys.readouterr()
        assert out.out == "" and out.err != ""

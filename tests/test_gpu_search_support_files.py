"""The reference-set search with jackknife support at file level (mhx_search_files_support) and through
`python -m auriclass_amd.search --support R [--clades FILE]`, against the rows of the restated rules (tests/search_rule.py
with the columns of tests/support_rule.py) byte for byte."""
import ctypes
import os

import numpy as np
import pytest

from auriclass_amd import engine, search
from oracle import mash_oracle as mo
from tests import search_cases as sc
from tests import search_rule
from tests import support_cases as cases
from tests import support_rule as rule

pytestmark = pytest.mark.gpu
K, S = sc.K, 1000
R8 = dict(replicates=8, keep=0.5, seed=42)


def write(path, prefix, lists):
    """one sketch file through engine.msh_write, and the same as the oracle's SketchFile; one name holds a comma"""
    names = ["%s/genome%s%d.fasta" % (prefix, "," if i == 3 else "", i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [800_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    engine.msh_write(path, K, S, names, comments, lengths, lists)
    return mo.SketchFile(K, S, [mo.Reference(n, c, l, np.asarray(h, np.uint64)) for n, c, l, h in zip(names, comments, lengths, lists)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("search_support")
    refs, _ = sc.references()
    qs = sc.queries()
    (near_q,), near_refs = cases.near_tie()
    R = write(d / "ref.msh", "r", list(refs[:70]) + list(near_refs))   # close lists, the empty reference 33, and the near-tie set
    # q1: the copies of lists 5 and 141, an empty list, 17 hashes, and the query whose best hit changes from replicate to replicate
    Q = [write(d / "q0.msh", "q0", qs[0:9]), write(d / "q1.msh", "q1", list(qs[22:30]) + [near_q])]
    clades = {ref.name: "Clade %s" % "I II III IV".split()[i % 4] for i, ref in enumerate(R.references)}
    table = d / "clade_config.csv"
    table.write_text("filename,clade\n" + "".join("%s,%s\n" % kv for kv in clades.items()) + "not/in/the/set.fna,Clade V\n")
    return d, R, Q, clades, table


def test_text_equals_the_rules_rows(files):
    d, R, Q, clades, table = files
    paths = [d / "q0.msh", d / "q1.msh"]
    for top, max_dist in ((5, 1.0), (3, 0.05), (64, 0.2)):
        want = rule.search_support_text(R, Q, top, max_dist, **R8)
        assert engine.search_files(d / "ref.msh", paths, top=top, max_dist=max_dist, **R8) == want
        assert [row.split("\t")[:5] for row in want.splitlines()] == [row.split("\t") for row in search_rule.search_text(R, Q, top, max_dist).splitlines()]
    want = rule.search_support_text(R, Q, 5, 1.0, **R8)
    counts = [int(row.split("\t")[5].split("/")[0]) for row in want.splitlines()]
    assert any(0 < c < 8 for c in counts) and sum(counts) == 8 * 18   # every query's counts sum to R; some hit is neither sure nor out
    with_clades = rule.search_support_text(R, Q, 5, 1.0, clades=clades, **R8)
    assert engine.search_files(d / "ref.msh", paths, clades=table, **R8) == with_clades
    assert all(len(row.split("\t")) == 8 for row in with_clades.splitlines()) and "r/genome,3.fasta" in with_clades
    # another seed and keep rate, more replicates than one group of lanes
    other = dict(replicates=70, keep=0.25, seed=2 ** 64 - 1)
    assert engine.search_files(d / "ref.msh", paths[:1], top=4, clades=table, **other) == rule.search_support_text(R, Q[:1], 4, clades=clades, **other)


def test_the_p_value_bound_drops_rows_afterwards(files):
    d, R, Q, clades, table = files
    paths = [d / "q0.msh", d / "q1.msh"]
    full = rule.search_support_text(R, Q, 5, 1.0, clades=clades, **R8)
    cut = rule.search_support_text(R, Q, 5, 1.0, 1e-10, clades=clades, **R8)
    assert 0 < cut.count("\n") < full.count("\n") and set(cut.splitlines()) <= set(full.splitlines())   # the counts are those of all hits
    assert engine.search_files(d / "ref.msh", paths, max_p_value=1e-10, clades=table, **R8) == cut


def test_no_replicates_is_the_plain_search(files):
    d, R, Q, clades, table = files
    paths = [d / "q0.msh", d / "q1.msh"]
    plain = engine.search_files(d / "ref.msh", paths, top=3, max_dist=0.2)
    assert plain == search_rule.search_text(R, Q, 3, 0.2)
    arr = (ctypes.c_char_p * 2)(*[os.fsencode(str(p)) for p in paths])
    opts = engine.SearchSupportOpts(ctypes.sizeof(engine.SearchSupportOpts), 3, 0.2, 1.0, 0, 0.5, 42)
    got = engine._text_call(lambda buf, cap, need: engine.load().mhx_search_files_support(os.fsencode(str(d / "ref.msh")), arr, 2, ctypes.byref(opts), None,
                                                                                         buf, cap, need))
    assert got == plain
    with pytest.raises(engine.EngineError) as exc:
        engine.search_files(d / "ref.msh", paths, clades=table)   # a clade table without replicates
    assert exc.value.code == engine.MHX_E_ARG and "replicates" in exc.value.message


def test_refusals(files, tmp_path):
    d, R, Q, clades, table = files
    short = tmp_path / "short.csv"
    short.write_text("filename,clade\n" + "".join("%s,%s\n" % kv for kv in list(clades.items())[:-1]))
    with pytest.raises(engine.EngineError) as exc:
        engine.search_files(d / "ref.msh", [d / "q0.msh"], clades=short, **R8)
    assert exc.value.code == engine.MHX_E_FORMAT and R.references[-1].name in exc.value.message
    with pytest.raises(engine.EngineError) as exc:
        engine.search_files(d / "ref.msh", [d / "q0.msh"], clades=tmp_path / "missing.csv", **R8)
    assert exc.value.code == engine.MHX_E_IO
    for bad in (dict(replicates=10001), dict(replicates=8, keep=0.0), dict(replicates=8, keep=float("nan")), dict(replicates=8, top=65)):
        with pytest.raises(engine.EngineError) as exc:
            engine.search_files(d / "ref.msh", [d / "q0.msh"], **bad)
        assert exc.value.code == engine.MHX_E_ARG


def test_command_line(files, capsys, tmp_path):
    d, R, Q, clades, table = files
    ref, q0, q1 = str(d / "ref.msh"), str(d / "q0.msh"), str(d / "q1.msh")
    assert search.main(["--support", "8", ref, q0, q1]) == 0
    assert capsys.readouterr().out == rule.search_support_text(R, Q, **R8)
    assert search.main(["-n", "3", "-d", "0.2", "--support", "8", "--keep", "0.25", "--seed", "7", "--clades", str(table), ref, q1]) == 0
    assert capsys.readouterr().out == rule.search_support_text(R, Q[1:], 3, 0.2, replicates=8, keep=0.25, seed=7, clades=clades)
    assert search.main(["--support", "0", "-n", "3", ref, q0]) == 0
    assert capsys.readouterr().out == search_rule.search_text(R, Q[:1], 3)
    for bad in (["--keep", "0.5"], ["--seed", "7"], ["--clades", str(table)], ["--support", "-1"], ["--support", "10001"], ["--support", "8", "--keep", "1.5"],
                ["--support", "0", "--clades", str(table)], ["--support", "8", "--clades", str(tmp_path / "missing.csv")]):
        assert search.main(bad + [ref, q0]) == 1, bad
        out = capsys.readouterr()
        assert out.out == "" and out.err != ""

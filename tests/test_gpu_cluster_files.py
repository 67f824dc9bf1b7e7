"""Dereplication at file level (mhx_cluster_files, python -m auriclass_amd.cluster) against the restated rule of
tests/cluster_rule.py byte for byte: the table for both kinds of representative and with comments, the sketch file of the
representatives against the oracle's writer and as the reference set of a search, refusals, and the command line."""
import numpy as np
import pytest

from auriclass_amd import cluster, engine
from oracle import mash_oracle as mo
from tests import cluster_rule as cr
from tests import triangle_cases as tc
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu
BOUND = 0.05


def sketch_file(seed, n, k=21, s=400):
    """as in tests/test_gpu_triangle_files.py: a base, near copies of it, independent lists; genome lengths all distinct and
    NOT in index order, so that the longest member of a cluster is not its first"""
    rng = np.random.default_rng(seed)
    base = tc.sketch_like(rng, s)
    lists = [base if i == 0 else (tc.mutate(rng, base, 0.02 * i) if i % 3 else tc.sketch_like(rng, s)) for i in range(n)]
    if n > 4:
        lists[4] = lists[1].copy()
        lists[2] = lists[2][:57]
    refs = [mo.Reference("set%d/ref%d.fasta" % (seed, i), "genome %d of set %d" % (i, seed), 900_000 + 12_345 * ((7 * i + 3) % 16) + seed, h)
            for i, h in enumerate(lists)]
    return mo.SketchFile(k, s, refs)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("cluster")
    A, B = sketch_file(12, 12), sketch_file(5, 5)
    # duplicates across the two files: a near copy of the first file's base, and an exact copy of one of its independent lists
    B.references[3].hashes = tc.mutate(np.random.default_rng(1), A.references[0].hashes, 0.05)
    B.references[0].hashes = A.references[6].hashes.copy()
    mo.write_msh(d / "a.msh", A)
    mo.write_msh(d / "b.msh", B)
    F = tr.combine([A, B])
    return d, F


def test_table_equals_the_rule(files):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    first = cr.cluster_text(F, BOUND)
    longest = cr.cluster_text(F, BOUND, rep="longest")
    clusters = int(first.splitlines()[-1].split("\t")[0])
    assert 1 < clusters < len(F.references) and first != longest   # the case joins some and not all, and the choice matters
    assert engine.cluster_files(paths, BOUND) == first
    assert engine.cluster_files(paths, BOUND, rep="longest") == longest
    assert engine.cluster_files(paths, BOUND, comment=True) == cr.cluster_text(F, BOUND, comment=True)
    assert engine.cluster_files(paths, BOUND, comment=True, rep="longest") == cr.cluster_text(F, BOUND, comment=True, rep="longest")
    for bound in (-1.0, 0.0, 0.01, 1.0):
        assert engine.cluster_files(paths, bound) == cr.cluster_text(F, bound)
    with pytest.raises(ValueError):
        engine.cluster_files(paths, BOUND, rep="shortest")


@pytest.mark.parametrize("rep", ["first", "longest"])
def test_the_representatives_file(files, tmp_path, rep):
    d, F = files
    out = tmp_path / "reps.msh"
    text = engine.cluster_files([d / "a.msh", d / "b.msh"], BOUND, rep=rep, out=out)
    assert text == cr.cluster_text(F, BOUND, rep=rep)
    want = cr.representatives_file(F, BOUND, rep)
    assert out.read_bytes() == mo.msh_bytes(want)   # names, comments, lengths and hash lists unchanged, in cluster order
    # the dereplicated set as the reference set of a search: every reference of the first file finds its representative's row
    hits = engine.search_files(out, [d / "a.msh"], top=1, max_dist=1.0)
    names = {r.name for r in want.references}
    rows = [row.split("\t") for row in hits.splitlines()]
    assert rows and all(row[0] in names for row in rows)
    for row in rows:
        if row[1] in names:
            assert row[0] == row[1] and row[2] == "0"   # a representative finds itself


def test_mismatch_damage_and_counts_are_refused(files, tmp_path):
    d, F = files
    mo.write_msh(tmp_path / "k19.msh", sketch_file(3, 3, k=19))
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_files([d / "a.msh", tmp_path / "k19.msh"], BOUND)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    mo.write_msh(tmp_path / "s300.msh", sketch_file(3, 3, s=300))
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_files([d / "a.msh", tmp_path / "s300.msh"], BOUND)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    bad = sketch_file(4, 4)
    bad.references[2].hashes = bad.references[2].hashes[::-1].copy()
    mo.write_msh(tmp_path / "descending.msh", bad)
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_files([d / "a.msh", tmp_path / "descending.msh"], BOUND)
    assert exc.value.code == engine.MHX_E_FORMAT and "not ascending" in exc.value.message
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_files([d / "a.msh"], float("nan"))
    assert exc.value.code == engine.MHX_E_ARG
    # multiplicity counts cannot be stored in the output file: refused, not dropped; without -o the table is printed
    counted = sketch_file(6, 4)
    counted.references[1].counts = np.full(len(counted.references[1].hashes), 3, np.uint32)
    mo.write_msh(tmp_path / "counted.msh", counted)
    out = tmp_path / "never.msh"
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_files([tmp_path / "counted.msh"], BOUND, out=out)
    assert exc.value.code == engine.MHX_E_ARG and "multiplicity counts" in exc.value.message and not out.exists()
    assert engine.cluster_files([tmp_path / "counted.msh"], BOUND) == cr.cluster_text(counted, BOUND)


def test_command_line(files, capsys, tmp_path):
    d, F = files
    a, b = str(d / "a.msh"), str(d / "b.msh")
    assert cluster.main(["-d", str(BOUND), a, b]) == 0
    assert capsys.readouterr().out == cr.cluster_text(F, BOUND)
    out = tmp_path / "cli.msh"
    assert cluster.main(["-p", "8", "-d", str(BOUND), "--rep", "longest", "-C", "-o", str(out), a, b]) == 0
    assert capsys.readouterr().out == cr.cluster_text(F, BOUND, comment=True, rep="longest")
    assert out.read_bytes() == mo.msh_bytes(cr.representatives_file(F, BOUND, "longest"))
    assert cluster.main([a, b]) != 0   # -d is required
    res = capsys.readouterr()
    assert res.out == "" and "-d" in res.err
    fa = tmp_path / "genome.fa"
    fa.write_text(">x\nACGT\n")
    assert cluster.main(["-d", "0.05", a, str(fa)]) == 1
    res = capsys.readouterr()
    assert res.out == "" and "mash sketch" in res.err and "genome.fa" in res.err
    assert cluster.main(["-d", "0.05", str(tmp_path / "missing.msh")]) == 1
    assert capsys.readouterr().out == ""

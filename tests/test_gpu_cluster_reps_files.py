"""The dereplication with medoid representatives and the distance-to-representative columns at file level
(mhx_cluster_reps_files, python -m auriclass_amd.cluster --rep medoid / --dist) against the restated rule of
tests/medoid_rule.py byte for byte: every linkage with every kind of representative, with comments, the sketch file of the
representatives and a search against it, the refusals, and the command line -- which without the two new flags still prints
what it printed before."""
import ctypes

import numpy as np
import pytest

from auriclass_amd import cluster, engine
from oracle import mash_oracle as mo
from tests import cluster_rule as cr
from tests import linkage_rule as lr
from tests import medoid_rule as mr
from tests import triangle_cases as tc
from tests import triangle_rule as tr

pytestmark = pytest.mark.gpu
BOUND = 0.05
LINKAGES = ("single", "complete", "average")
REPS = ("first", "longest", "medoid")


def sketch_files():
    """Two files, 17 references at s = 400: a base in the MIDDLE of its cluster's indices with near copies before and behind
    it (the medoid is neither the first member nor the longest genome), two far copies that single linkage joins and complete
    linkage does not, an exact duplicate (a tie on the sum), a second small cluster, a short list and independent lists."""
    rng = np.random.default_rng(1717)
    k, s = 21, 400
    base = tc.sketch_like(rng, s)
    other = tc.sketch_like(rng, s)
    lists = [tc.mutate(rng, base, 0.10), tc.mutate(rng, base, 0.12), tc.sketch_like(rng, s), base, tc.mutate(rng, base, 0.08), tc.mutate(rng, base, 0.5),
             tc.sketch_like(rng, s), tc.mutate(rng, base, 0.5), other, tc.mutate(rng, other, 0.05), tc.mutate(rng, other, 0.07), tc.sketch_like(rng, s)[:57],
             base.copy(), tc.sketch_like(rng, s), tc.mutate(rng, other, 0.06), tc.sketch_like(rng, s), tc.mutate(rng, base, 0.15)]
    refs = [mo.Reference("reps/ref%d.fasta" % i, "genome %d" % i, 900_000 + 12_345 * ((7 * i + 1) % 17), h) for i, h in enumerate(lists)]
    return mo.SketchFile(k, s, refs[:10]), mo.SketchFile(k, s, refs[10:])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("cluster_reps")
    A, B = sketch_files()
    mo.write_msh(d / "a.msh", A)
    mo.write_msh(d / "b.msh", B)
    return d, tr.combine([A, B])


@pytest.mark.parametrize("linkage", LINKAGES)
def test_table_equals_the_rule(files, linkage):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    texts = {}
    for rep in REPS:
        texts[rep] = mr.reps_text(F, BOUND, linkage, rep)
        assert engine.cluster_reps_files(paths, BOUND, linkage=linkage, rep=rep) == texts[rep], rep
        assert engine.cluster_reps_files(paths, BOUND, linkage=linkage, rep=rep, comment=True) == mr.reps_text(F, BOUND, linkage, rep, comment=True), rep
    assert len(set(texts.values())) == 3   # the choice matters: the medoid is neither the first nor the longest member
    clusters = int(texts["medoid"].splitlines()[-1].split("\t")[0])
    assert 1 < clusters < len(F.references)
    rows = [row.split("\t") for row in texts["medoid"].splitlines()]
    assert all(len(row) == 7 for row in rows) and any(row[2] == row[3] and row[4] == "0" for row in rows)   # a representative lies 0 from itself
    for bound in (-1.0, 0.0, 0.01, 1.0):
        assert engine.cluster_reps_files(paths, bound, linkage=linkage) == mr.reps_text(F, bound, linkage, "medoid"), bound


def test_the_linkages_differ_and_share_the_columns_of_the_old_calls(files):
    d, F = files
    paths = [d / "a.msh", d / "b.msh"]
    got = {linkage: engine.cluster_reps_files(paths, BOUND, linkage=linkage, rep="first") for linkage in LINKAGES}
    assert got["single"] != got["complete"]
    # the first four columns are those of the calls that were there before
    four = lambda text: "".join("\t".join(row.split("\t")[:4]) + "\n" for row in text.splitlines())
    assert four(got["single"]) == four(cr.cluster_text(F, BOUND)) == four(engine.cluster_files(paths, BOUND))
    assert four(got["complete"]) == lr.cut_text(F, lr.COMPLETE, BOUND) == engine.linkage_files(paths, "complete", mode="cut", max_dist=BOUND)
    assert four(got["average"]) == lr.cut_text(F, lr.AVERAGE, BOUND)


@pytest.mark.parametrize("linkage,rep", [("single", "medoid"), ("complete", "medoid"), ("average", "longest")])
def test_the_representatives_file(files, tmp_path, linkage, rep):
    d, F = files
    out = tmp_path / "reps.msh"
    text = engine.cluster_reps_files([d / "a.msh", d / "b.msh"], BOUND, linkage=linkage, rep=rep, out=out)
    assert text == mr.reps_text(F, BOUND, linkage, rep)
    want = mr.reps_file(F, BOUND, linkage, rep)
    assert out.read_bytes() == mo.msh_bytes(want)
    hits = engine.search_files(out, [d / "a.msh"], top=1, max_dist=1.0)
    names = {r.name for r in want.references}
    rows = [row.split("\t") for row in hits.splitlines()]
    assert rows and all(row[0] in names for row in rows)
    for row in rows:
        if row[1] in names:
            assert row[0] == row[1] and row[2] == "0"   # a representative finds itself


def test_counts_and_bad_options_are_refused(files, tmp_path):
    d, F = files
    A, _ = sketch_files()
    A.references[1].counts = np.full(len(A.references[1].hashes), 3, np.uint32)
    mo.write_msh(tmp_path / "counted.msh", A)
    out = tmp_path / "never.msh"
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_reps_files([tmp_path / "counted.msh"], BOUND, out=out)
    assert exc.value.code == engine.MHX_E_ARG and "multiplicity counts" in exc.value.message and not out.exists()
    assert engine.cluster_reps_files([tmp_path / "counted.msh"], BOUND) == mr.reps_text(A, BOUND)
    with pytest.raises(engine.EngineError) as exc:
        engine.cluster_reps_files([d / "a.msh"], float("nan"))
    assert exc.value.code == engine.MHX_E_ARG
    lib = engine.load()
    paths = (ctypes.c_char_p * 1)(str(d / "a.msh").encode())
    need = ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(1 << 16)
    size = ctypes.sizeof(engine.ClusterRepsOpts)
    for opts in (engine.ClusterRepsOpts(size - 4, 0, 0, 2, BOUND), engine.ClusterRepsOpts(size, 0, 3, 2, BOUND), engine.ClusterRepsOpts(size, 0, -1, 2, BOUND),
                 engine.ClusterRepsOpts(size, 0, 0, 3, BOUND), engine.ClusterRepsOpts(size, 0, 0, -1, BOUND), engine.ClusterRepsOpts(size, 0, 0, 2, float("nan"))):
        assert lib.mhx_cluster_reps_files(paths, 1, ctypes.byref(opts), None, buf, len(buf), ctypes.byref(need)) == engine.MHX_E_ARG
    # no options: single linkage, the medoid, every pair joined
    A0, _ = sketch_files()
    assert lib.mhx_cluster_reps_files(paths, 1, None, None, buf, len(buf), ctypes.byref(need)) == engine.MHX_OK
    assert buf.value.decode() == mr.reps_text(A0, 1.0)
    # the old calls still refuse the third kind
    old = engine.ClusterOpts(ctypes.sizeof(engine.ClusterOpts), 0, 2, BOUND)
    assert lib.mhx_cluster_files(paths, 1, ctypes.byref(old), None, buf, len(buf), ctypes.byref(need)) == engine.MHX_E_ARG


def test_command_line(files, capsys, tmp_path):
    d, F = files
    a, b = str(d / "a.msh"), str(d / "b.msh")
    assert cluster.main(["-d", str(BOUND), "--rep", "medoid", a, b]) == 0
    assert capsys.readouterr().out == mr.reps_text(F, BOUND, "single", "medoid")
    assert cluster.main(["-d", str(BOUND), "--dist", a, b]) == 0
    assert capsys.readouterr().out == mr.reps_text(F, BOUND, "single", "first")
    out = tmp_path / "cli.msh"
    assert cluster.main(["-d", str(BOUND), "--linkage", "complete", "--rep", "medoid", "-C", "-o", str(out), a, b]) == 0
    assert capsys.readouterr().out == mr.reps_text(F, BOUND, "complete", "medoid", comment=True)
    assert out.read_bytes() == mo.msh_bytes(mr.reps_file(F, BOUND, "complete", "medoid"))
    assert cluster.main(["-d", str(BOUND), "--linkage", "average", "--rep", "longest", "--dist", a, b]) == 0
    assert capsys.readouterr().out == mr.reps_text(F, BOUND, "average", "longest")
    # without the two flags: the calls and the bytes of before
    assert cluster.main(["-d", str(BOUND), a, b]) == 0
    assert capsys.readouterr().out == cr.cluster_text(F, BOUND)
    assert cluster.main(["-d", str(BOUND), "--rep", "longest", "-C", a, b]) == 0
    assert capsys.readouterr().out == cr.cluster_text(F, BOUND, comment=True, rep="longest")
    for name, code in (("complete", lr.COMPLETE), ("average", lr.AVERAGE)):
        assert cluster.main(["-d", str(BOUND), "--linkage", name, a, b]) == 0
        assert capsys.readouterr().out == lr.cut_text(F, code, BOUND)
    assert cluster.main(["-d", str(BOUND), "--rep", "shortest", a, b]) != 0
    assert capsys.readouterr().out == ""

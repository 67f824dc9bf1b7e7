"""The bounded neighbourhood call at file level (mhx_within_files), through `python -m auriclass_amd.search --all` and through
the shim's `mash dist -d / -v`, against the rows of the restated rule (tests/within_rule.py) byte for byte, formatted as the
oracle's dist_text formats them."""
import numpy as np
import pytest

from auriclass_amd import engine, mash_shim, search
from oracle import mash_oracle as mo
from tests import search_cases as sc
from tests import within_cases as wc
from tests import within_rule as rule

pytestmark = pytest.mark.gpu


def write(path, prefix, lists, k, s):
    """one sketch file through engine.msh_write, and the same as the oracle's SketchFile"""
    names = ["%s/genome%d.fasta" % (prefix, i) for i in range(len(lists))]
    comments = ["%s record %d" % (prefix, i) for i in range(len(lists))]
    lengths = [800_000 + 4321 * i + len(prefix) for i in range(len(lists))]
    engine.msh_write(path, k, s, names, comments, lengths, lists)
    return mo.SketchFile(k, s, [mo.Reference(n, c, l, np.asarray(h, np.uint64)) for n, c, l, h in zip(names, comments, lengths, lists)])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    engine.init()
    d = tmp_path_factory.mktemp("within")
    refs, qrys = wc.case_set()
    R = write(d / "ref.msh", "r", refs, wc.K, wc.S)
    Q = [write(d / "q0.msh", "q0", qrys[0:3], wc.K, wc.S), write(d / "q1.msh", "q1", qrys[3:9], wc.K, wc.S), write(d / "q2.msh", "q2", qrys[66:70], wc.K, wc.S)]
    return d, R, Q


def test_text_equals_the_rules_rows_in_both_orders(files):
    d, R, Q = files
    paths = [d / "q0.msh", d / "q1.msh", d / "q2.msh"]
    for max_dist in (0.0, 0.02, wc.exact_bound(), float(np.nextafter(wc.exact_bound(), 0.0)), 0.05):
        for order in (0, 1):
            want = rule.within_text(R, Q, max_dist, order=order)
            assert engine.within_files(d / "ref.msh", paths, max_dist, order=order) == want
        if max_dist == 0.02:
            rows = want.splitlines()
            assert sum(r.split("\t")[1] == "q0/genome0.fasta" for r in rows) > 64 and sum(r.split("\t")[1] == "q0/genome1.fasta" for r in rows) > 64
            assert rule.within_text(R, Q, max_dist, order=0) != want and sorted(rule.within_text(R, Q, max_dist, order=0).splitlines()) == sorted(rows)
    # the p-value bound drops rows on the host
    full = rule.within_text(R, Q, 0.05)
    ps = sorted(float(r.split("\t")[3]) for r in full.splitlines())
    bound = ps[len(ps) // 2]
    for order in (0, 1):
        cut = rule.within_text(R, Q, 0.05, bound, order=order)
        assert 0 < cut.count("\n") < full.count("\n") and set(cut.splitlines()) < set(full.splitlines())
        assert engine.within_files(d / "ref.msh", paths, 0.05, bound, order=order) == cut
    assert engine.within_files(d / "ref.msh", paths[2:], 0.05) == ""                       # queries without hits print nothing
    everything = rule.within_text(R, Q, 1.0, order=1)   # more hits than the first buffers of a batch hold (4096): the batch runs twice
    assert everything.count("\n") == 13 * wc.NR > 4096 and engine.within_files(d / "ref.msh", paths, 1.0, order=1) == everything


def test_query_files_across_the_batch_of_4096_sketches(tmp_path):
    """query files of 3000, 1200 and 50 sketches at s = 16 (tests/search_cases.py: batch_boundary): the first batch goes to the
    device behind file 1 with 4200 sketches, the last holds file 2 alone, and the bound leaves hits in every file.  The text is
    that of the three files one by one, in both orders."""
    engine.init()
    refs, lists = sc.batch_boundary()
    write(tmp_path / "ref.msh", "r", refs, sc.K, 16)
    paths = [tmp_path / ("q%d.msh" % i) for i in range(3)]
    for i, q in enumerate(lists):
        write(paths[i], "q%d" % i, q, sc.K, 16)
    assert len(lists[0]) < 4096 <= len(lists[0]) + len(lists[1])
    for order in (0, 1):
        one_by_one = [engine.within_files(tmp_path / "ref.msh", [p], 0.05, order=order) for p in paths]
        assert all(t.count("\n") > 0 for t in one_by_one)
        assert engine.within_files(tmp_path / "ref.msh", paths, 0.05, order=order) == "".join(one_by_one)


def test_mismatches_damaged_files_and_bad_options(files, tmp_path):
    d, R, Q = files
    _, qrys = wc.case_set()
    write(tmp_path / "k19.msh", "k19", qrys[:3], 19, wc.S)
    with pytest.raises(engine.EngineError) as exc:
        engine.within_files(d / "ref.msh", [d / "q0.msh", tmp_path / "k19.msh"], 0.05)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different k-mer sizes" in exc.value.message
    write(tmp_path / "s64.msh", "s64", [q[:64] for q in qrys[:3]], wc.K, 64)
    with pytest.raises(engine.EngineError) as exc:
        engine.within_files(d / "ref.msh", [d / "q0.msh", tmp_path / "s64.msh"], 0.05)
    assert exc.value.code == engine.MHX_E_MISMATCH and "different sketch sizes" in exc.value.message
    for bad in (dict(max_dist=float("nan")), dict(max_dist=0.05, max_p_value=float("nan")), dict(max_dist=0.05, order=2)):
        with pytest.raises(engine.EngineError) as exc:
            engine.within_files(d / "ref.msh", [d / "q0.msh"], **bad)
        assert exc.value.code == engine.MHX_E_ARG
    mo.write_msh(tmp_path / "descending.msh", mo.SketchFile(wc.K, wc.S, [mo.Reference("x", "", 1000, np.asarray(qrys[0][::-1].copy()))]))
    (tmp_path / "garbage.msh").write_bytes(b"not a sketch file at all" * 10)
    for ref in (tmp_path / "missing.msh", tmp_path / "descending.msh", tmp_path / "garbage.msh"):
        with pytest.raises(engine.EngineError) as want:
            engine.search_files(ref, [d / "q0.msh"])
        with pytest.raises(engine.EngineError) as got:
            engine.within_files(ref, [d / "q0.msh"], 0.05)
        assert got.value.code == want.value.code, ref


@pytest.fixture(scope="module")
def search_files(tmp_path_factory):
    """the files of tests/test_gpu_search_files.py: no query of the search case set has more than 11 hits below 1"""
    engine.init()
    d = tmp_path_factory.mktemp("within_search")
    refs, _ = sc.references()
    qs = sc.queries()
    write(d / "ref_a.msh", "a", refs[:70], sc.K, 1000)
    write(d / "ref_b.msh", "b", refs[100:200], sc.K, 1000)
    write(d / "q0.msh", "q0", qs[0:9], sc.K, 1000)
    write(d / "q1.msh", "q1", qs[22:30], sc.K, 1000)
    write(d / "q2.msh", "q2", qs[9:12] + qs[40:43], sc.K, 1000)
    return d


def test_search_all_equals_search_n_64_where_no_list_is_truncated(search_files, capsys):
    d = search_files
    qs = [str(d / "q0.msh"), str(d / "q1.msh"), str(d / "q2.msh")]
    assert sc.hits_per_query(0.2).max() <= 64
    for ref in (str(d / "ref_a.msh"), str(d / "ref_b.msh")):
        for extra in (["-d", "0.05"], ["-d", "0"], ["-d", "0.2", "-v", "1e-10"]):
            assert search.main(["-n", "64"] + extra + [ref] + qs) == 0
            capped = capsys.readouterr().out
            assert search.main(["--all"] + extra + ["-p", "4", ref] + qs) == 0
            assert capsys.readouterr().out == capped
            assert extra[1] == "0" or capped.count("\n") > 3


def test_search_all_refusals(search_files, capsys):
    d = search_files
    ref, q = str(d / "ref_a.msh"), str(d / "q0.msh")
    assert search.main(["--all", ref, q]) == 1
    out = capsys.readouterr()
    assert out.out == "" and "--all needs an explicit -d" in out.err
    for flag, more in (("-n", ["-n", "5"]), ("--support", ["--support", "8"]), ("--keep", ["--keep", "0.5"]), ("--seed", ["--seed", "1"]),
                       ("--clades", ["--clades", "clades.csv"])):
        assert search.main(["--all", "-d", "0.05"] + more + [ref, q]) == 1
        out = capsys.readouterr()
        assert out.out == "" and f"--all cannot be combined with {flag}" in out.err


def test_mash_dist_through_the_shim(files, capsys):
    d, R, Q = files
    ref, q0, q1 = str(d / "ref.msh"), str(d / "q0.msh"), str(d / "q1.msh")
    assert mash_shim.main(["dist", "-d", "0.02", ref, q0, q1]) == 0
    assert capsys.readouterr().out == rule.within_text(R, Q[:2], 0.02)
    full = rule.within_text(R, Q[:2], 0.05)
    ps = sorted(float(r.split("\t")[3]) for r in full.splitlines())
    bound = ps[len(ps) // 3]
    assert mash_shim.main(["dist", "-v", repr(bound), "-p", "8", "-d", "0.05", ref, q0, q1]) == 0
    assert capsys.readouterr().out == rule.within_text(R, Q[:2], 0.05, bound)
    assert mash_shim.main(["dist", "-v", repr(bound), ref, q0]) == 0            # -v alone: every distance, the p-value filter
    assert capsys.readouterr().out == rule.within_text(R, Q[:1], 1.0, bound)
    assert mash_shim.main(["dist", ref, q1]) == 0                              # no filter: today's call, today's bytes
    plain = capsys.readouterr().out
    assert plain == engine.dist_files(ref, q1) and plain.count("\n") == 6 * wc.NR
    assert mash_shim.main(["dist", ref, q0, q1]) == 0                          # several queries, no filter
    assert capsys.readouterr().out == engine.dist_files_multi(ref, [q0, q1]) == engine.dist_files(ref, q0) + plain
    for flag in ("-t", "-l", "-C", "-k", "-s", "-i", "-r"):
        assert mash_shim.main(["dist", flag, ref, q0]) == 1
        out = capsys.readouterr()
        assert out.out == "" and f"mash dist {flag} is not supported" in out.err
    assert mash_shim.main(["dist", "-d", "0.02", ref]) == 1
    assert "mash dist" in capsys.readouterr().err

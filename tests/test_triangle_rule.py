"""The restated rule of `mash triangle` (tests/triangle_rule.py) against the mash-pinned `mash dist` text of the oracle: the
edge list is the dist rows of the pairs j < i, and the matrix holds the same distances."""
import numpy as np

from oracle import mash_oracle as mo
from tests import triangle_cases as tc
from tests import triangle_rule as tr


def nine_references():
    rng = np.random.default_rng(909)
    k, s = 21, 400
    base = tc.sketch_like(rng, s)
    lists = [base, tc.mutate(rng, base, 0.01), tc.mutate(rng, base, 0.1), tc.mutate(rng, base, 0.5), tc.sketch_like(rng, s),
             tc.sketch_like(rng, s)[:40], base.copy(), np.zeros(0, np.uint64), tc.mutate(rng, base, 0.9)]
    refs = [mo.Reference("ref%d.fa" % i, "comment of %d" % i, 1_000_000 + 77_777 * i, h) for i, h in enumerate(lists)]
    return mo.SketchFile(k, s, refs)


def test_edge_rows_are_the_dist_rows_of_the_lower_triangle():
    F = nine_references()
    n = len(F.references)
    rows = mo.dist_text(F, F).splitlines(keepends=True)   # query-major: row q * n + r is reference r against query q
    assert len(rows) == n * n
    want = "".join(rows[j * n + i] for i in range(n) for j in range(i))   # reference i, query j < i
    assert tr.edge_text(F) == want
    assert tr.edge_text(F, 1.0, 1.0).count("\n") == n * (n - 1) // 2


def test_filters_and_matrix_follow_the_same_pairs():
    F = nine_references()
    pairs = tr.pairs(F)
    kept = [p for p in pairs if p[4] <= 0.05 and p[5] <= 1e-10]
    assert 0 < len(kept) < len(pairs)
    assert tr.edge_text(F, 0.05, 1e-10).count("\n") == len(kept)
    lines = tr.matrix_text(F).split("\n")
    assert lines[0] == "\t9" and lines[-1] == "" and len(lines) == 11
    assert lines[1] == "ref0.fa"
    at = 0
    for i in range(9):
        cells = lines[1 + i].split("\t")
        assert cells[0] == "ref%d.fa" % i and len(cells) == 1 + i
        for j in range(i):
            assert cells[1 + j] == mo.fmt_g(pairs[at][4])
            at += 1
    assert tr.matrix_text(F, comment=True).split("\n")[3].startswith("comment of 2\t")
    assert lines[7].split("\t")[1] == "0"   # the exact duplicate of reference 0

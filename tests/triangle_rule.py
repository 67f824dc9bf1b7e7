"""The rule of `mash triangle` (Mash 2.x CommandTriangle) as a plain statement over a set of sketches, built from the
pieces of the CPU oracle that are pinned by mash's own output for `mash dist`: compare (compareSketches), p_value and
fmt_g.  Shared by the triangle tests; not a test module itself.

    set        = the references of all sketch files, in argument order and then file order
    pair(i, j) = compare(reference i, reference j) for j < i: common, denom, distance
    matrix     = "\\t<n>\\n", then per reference i: its name (its comment under -C), "\\t<distance>" for j = 0 .. i - 1, "\\n"
    edge list  = for i ascending, j < i ascending, every pair with distance <= max_dist and p <= max_p_value:
                 "name_i\\tname_j\\tdistance\\tp\\tcommon/denom\\n" -- the `mash dist` row of reference i and query j,
                 p = p_value(common, length_i, length_j, 4^k, denom)
"""
from oracle import mash_oracle as mo


def combine(files):
    """one SketchFile holding the references of all `files` in order (they share k and sketch size)"""
    first = files[0]
    assert all(f.kmer_size == first.kmer_size and f.sketch_size == first.sketch_size for f in files)
    return mo.SketchFile(first.kmer_size, first.sketch_size, [r for f in files for r in f.references])


def pairs(F):
    """[(i, j, common, denom, distance, p)] for i ascending, j < i ascending"""
    k, s = F.kmer_size, F.sketch_size
    out = []
    for i, a in enumerate(F.references):
        for j in range(i):
            b = F.references[j]
            common, denom, d = mo.compare(a.hashes, b.hashes, s, k)
            out.append((i, j, common, denom, d, mo.p_value(common, a.length, b.length, 4.0 ** k, denom)))
    return out


def matrix_text(F, comment=False):
    rows = pairs(F)
    text = ["\t%d\n" % len(F.references)]
    at = 0
    for i, a in enumerate(F.references):
        text.append(a.comment if comment else a.name)
        for _ in range(i):
            text.append("\t" + mo.fmt_g(rows[at][4]))
            at += 1
        text.append("\n")
    return "".join(text)


def edge_text(F, max_dist=1.0, max_p_value=1.0):
    refs = F.references
    return "".join("%s\t%s\t%s\t%s\t%d/%d\n" % (refs[i].name, refs[j].name, mo.fmt_g(d), mo.fmt_g(p), common, denom)
                   for i, j, common, denom, d, p in pairs(F) if d <= max_dist and p <= max_p_value)

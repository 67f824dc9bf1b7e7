"""Sketches of more than 65 536 hashes on the all-vs-refs distance path: the number of value ranges of a call grows with its
longest list (1024 x W, mhx_dist.h: dist_windows), so that sketch sizes up to the CLI's largest (-s 1 000 000) keep short
slices and stay on the fast kernels instead of raising the overflow flag in every block.  Everything against the oracle's
compareSketches (`common`, `denom`, and `dist` where the host computes it)."""
import functools

import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests.test_dist_emulation import WORST_HI, clade_queries, clade_refs, pad_rows, sketch_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _engine():
    engine.init(0)


def _lib():
    return engine.load()


@functools.lru_cache(maxsize=1)
def _clade_refs(s, hi):
    return clade_refs(np.random.default_rng(71), s, hi)


def _run(qrys, refs, k, s):
    stride = (max(max(map(len, refs)), max(map(len, qrys)), 1) + 15) // 16 * 16
    Q, ql = pad_rows(qrys, stride)
    R, rl = pad_rows(refs, stride)
    return engine.dist_batch(Q, ql, R, rl, k, s)


def _check(got, qrys, refs, k, s):
    common, denom, dist = got
    for qi in range(len(qrys)):
        for ri, r in enumerate(refs):
            c, d, dd = mo.compare(r, qrys[qi], s, k)
            assert (int(common[qi, ri]), int(denom[qi, ri])) == (c, d), (qi, ri, len(qrys[qi]), len(r))
            assert dist[qi, ri] == dd, (qi, ri)


CLADE_CASES = [(s, hi, nq, None) for s in (250_000, 500_000, 1_000_000) for hi in (2 ** 64, WORST_HI) for nq in (1, 9)]
CLADE_CASES += [(250_000, hi, 130, walk) for hi in (2 ** 64, WORST_HI) for walk in (None, "128")]


@pytest.mark.parametrize("s,hi,nq,walk_min", CLADE_CASES)
def test_clade_shaped_references_stay_on_the_fast_path(monkeypatch, s, hi, nq, walk_min):
    """24 references of one clade (11 close to a base list, 13 half fresh, one shorter than s), values uniform below 2^64 and
    below 2^63.01 (the worst rounding of the scale: half of the ranges in use).  1 query is AuriClass's own call, 9 take
    the slice-per-wave form of the range pass, 130 the one-query-per-lane form -- also with MHX_DIST_WALK_MIN forced below
    the batch size, which a windowed call must not follow into the walk form.  No block may fall back: with at most 64
    entries per slice on average the longest slice is ~100 entries (~170 at the worst rounding) against 255, the most
    distinct keys of a range ~550 (~1040) against 1536."""
    if walk_min:
        monkeypatch.setenv("MHX_DIST_WALK_MIN", walk_min)
    refs = _clade_refs(s, hi)
    qrys = clade_queries(np.random.default_rng(171), refs, max(nq, 9), hi)
    if nq == 1:
        qrys = qrys[4:5]
    else:
        qrys[2] = qrys[2][:len(qrys[2]) // 3]   # ends a third of the way through the value space
        qrys[3] = np.zeros(0, np.uint64)
    got = _run(qrys, refs, 27, s)
    assert _lib().mhx_last_dist_fallback_blocks() == 0
    assert _lib().mhx_last_dist_ranges() > 1024
    assert _lib().mhx_last_dist_ranges() == {250_000: 4096, 500_000: 8192, 1_000_000: 16384}[s]
    _check(got, qrys, refs, 27, s)


def test_dist_files_at_the_largest_sketch_size(tmp_path):
    """`mash dist REF QUERY` at file level, s = 1 000 000: a 192 MB reference sketch file of 24 clade-like references (pinned
    image, parsed in place, row-by-row copies) and a one-sketch query file; the text is the oracle's, no block falls back."""
    s = 1_000_000
    rng = np.random.default_rng(5 + s)
    base = sketch_like(rng, s)
    refs = []
    for j in range(24):
        keep = rng.random(len(base)) >= 0.001 * (j + 1)
        h = np.unique(np.concatenate([base[keep], sketch_like(rng, int((~keep).sum()))]))
        refs.append(mo.Reference("ref%d.fa" % j, "clade %d" % (j % 5), 12_000_000 + j, h))
    q = np.unique(np.concatenate([refs[7].hashes[::2], sketch_like(rng, s // 2)]))[:s]
    R = mo.SketchFile(kmer_size=27, sketch_size=s, references=refs)
    Q = mo.SketchFile(kmer_size=27, sketch_size=s, references=[mo.Reference("sample.fa", "query", 12_300_000, q)])
    (tmp_path / "r.msh").write_bytes(mo.msh_bytes(R))
    (tmp_path / "q.msh").write_bytes(mo.msh_bytes(Q))
    assert (tmp_path / "r.msh").stat().st_size < 256 << 20
    want = mo.dist_text(R, Q)
    for _ in range(2):   # the second call reuses the pinned image
        assert engine.dist_files(tmp_path / "r.msh", tmp_path / "q.msh") == want
        assert _lib().mhx_last_dist_fallback_blocks() == 0
        assert _lib().mhx_last_dist_ranges() == 16384


def test_independent_references_at_the_largest_sketch_size():
    """24 unrelated lists of 1 000 000 hashes: 24 x 61 distinct keys per range are at the range table's limit, so blocks may
    fall back (the count is printed, not asserted); the results are exact either way."""
    rng = np.random.default_rng(72)
    s = 1_000_000
    refs = [sketch_like(rng, s) for _ in range(24)]
    qrys = clade_queries(rng, refs, 9)
    got = _run(qrys, refs, 27, s)
    print("independent references, s = 1 000 000: fallback blocks", _lib().mhx_last_dist_fallback_blocks(),
          "ranges", _lib().mhx_last_dist_ranges(), "kernel ms", round(_lib().mhx_last_dist_kernel_ms(), 3))
    _check(got, qrys, refs, 27, s)


@pytest.mark.parametrize("s", [50_000, 65_536])
def test_nothing_moves_up_to_65536_hashes(s):
    """Lists of up to 65 536 hashes keep the 1024 ranges (and the kernels, grids and workspace) they always had."""
    rng = np.random.default_rng(73)
    refs = clade_refs(rng, s)
    refs[0] = np.unique(np.concatenate([refs[0], sketch_like(rng, s // 8)]))[:s]
    assert len(refs[0]) == s   # a list of exactly s entries: 65 536 is the last length with 1024 ranges
    qrys = clade_queries(rng, refs, 3)
    got = _run(qrys, refs, 27, s)
    assert _lib().mhx_last_dist_ranges() == 1024
    assert _lib().mhx_last_dist_fallback_blocks() == 0
    _check(got, qrys, refs, 27, s)


def test_crowded_values_at_a_large_sketch_size_fall_back():
    """The construction of test_dist_non_uniform_values_fall_back_to_the_generic_kernel at s = 300 000: all hashes in one
    narrow stretch of the value space, one far outlier that sets the scale.  The windowed range pass must notice (more
    distinct keys than its table may hold) and the generic kernel deliver exact results."""
    rng = np.random.default_rng(22)
    lo, s = 1 << 62, 300_000
    refs = [lo + sketch_like(rng, s, hi=2 ** 27) for _ in range(8)]
    refs.append(np.concatenate([refs[0][:1000], np.array([2 ** 64 - 5], np.uint64)]))   # one far outlier sets the scale
    qrys = [np.unique(np.concatenate([refs[i % 8][::2], lo + sketch_like(rng, s // 2, hi=2 ** 27)])) for i in range(10)]
    got = _run(qrys, refs, 21, s)
    assert _lib().mhx_last_dist_fallback_blocks() >= 1
    _check(got, qrys, refs, 21, s)


def test_more_than_32_references_and_query_batches(monkeypatch):
    """40 references (two slices of 32 and 8) x 9 queries in batches of 4 (MHX_DIST_QBATCH) at s = 250 000: six blocks of the
    windowed form, each filling its part of the output."""
    monkeypatch.setenv("MHX_DIST_QBATCH", "4")
    rng = np.random.default_rng(74)
    s = 250_000
    refs = clade_refs(rng, s, nr=40)
    qrys = clade_queries(rng, refs, 9)
    qrys[4] = np.zeros(0, np.uint64)
    qrys[6] = qrys[6][:len(qrys[6]) // 3]
    got = _run(qrys, refs, 27, s)
    assert _lib().mhx_last_dist_fallback_blocks() == 0
    assert _lib().mhx_last_dist_ranges() == 4096
    _check(got, qrys, refs, 27, s)

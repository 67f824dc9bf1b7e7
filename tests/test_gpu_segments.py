"""mhx_sketch_segments (one bottom-s list per segment of a dense stream, `mash sketch -i` at buffer level) against the
oracle's definition-level sketch of every segment on its own: hashes and lengths exactly equal.  Shapes: tests/segment_cases.py
(lengths around k, a wave and the cut between the one-launch route and the sketcher route; touching segments; 5 000 short
segments; repeats and palindromes; N runs, lower case, line breaks)."""
import numpy as np
import pytest

from auriclass_amd import engine
from oracle import mash_oracle as mo
from tests import segment_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cut():
    engine.init()
    return engine.sketch_segments_cut()


def _device_call(data: bytes, off: np.ndarray, k: int, s: int, stride: int):
    import torch

    dev = f"cuda:{torch.cuda.current_device()}"
    d_bytes = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)   # readable to the next 16-byte boundary past the end
    d_bytes[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    n_seg = off.size - 1
    d_rows = torch.zeros((n_seg, stride), dtype=torch.int64, device=dev)
    d_len = torch.zeros(n_seg, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.sketch_segments_device(d_bytes.data_ptr(), len(data), d_off.data_ptr(), n_seg, k, s, d_rows.data_ptr(), d_len.data_ptr(), stride)
    return d_rows, d_len


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("name", sc.CASES)
def test_cases_against_the_oracle(cut, name, k):
    data, off = sc.case(name, k, cut)
    windows = np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0)
    if name == "edge_lengths":                                          # both routes and the seam between them
        assert {0, 1, 2, cut - 1, cut, cut + 1} <= set(int(w) for w in windows)
    for s in sc.SS:
        rows, lens = engine.sketch_segments(data, off, k, s)
        assert rows.shape == (off.size - 1, min(s, int(windows.max())))
        sc.check_rows(rows, lens, name, k, s, cut)
        for i in range(lens.size):
            assert not rows[i, lens[i]:].any()                          # host pointers: zero behind the list


@pytest.mark.parametrize("name,k,s", [("edge_lengths", 21, 1000), ("touching", 16, 16), ("dirty", 27, 1000), ("many", 17, 16)])
def test_device_pointers_give_the_same_rows(cut, name, k, s):
    data, off = sc.case(name, k, cut)
    rows, lens = engine.sketch_segments(data, off, k, s)
    d_rows, d_len = _device_call(data, off, k, s, rows.shape[1])
    g_rows, g_len = d_rows.cpu().numpy().view(np.uint64), d_len.cpu().numpy().view(np.uint32)
    assert np.array_equal(g_len, lens)
    for i in range(lens.size):
        assert g_rows[i, :lens[i]].tobytes() == rows[i, :lens[i]].tobytes()
    sc.check_rows(g_rows, g_len, name, k, s, cut)


def test_a_wider_stride_and_a_sketcher_oracle(cut):
    """rows wider than they need be; the expectation from the oracle's Sketcher (the heap mash keeps) this time"""
    k, s = 21, 50
    data, off = sc.case("edge_lengths", k, cut)
    rows, lens = engine.sketch_segments(data, off, k, s, stride=77)
    assert rows.shape[1] == 77
    for i in range(lens.size):
        sk = mo.Sketcher(k, s, 1)
        sk.add_seq(data[int(off[i]):int(off[i + 1])])
        want, _ = sk.finish()
        assert lens[i] == want.size and np.array_equal(rows[i, :want.size], want)


def test_stride_too_small_and_other_bad_arguments(cut):
    k, s = 21, 100
    data, off = sc.case("touching", k, cut)
    need = min(s, int(np.diff(off.astype(np.int64)).max()) - k + 1)
    rows, lens = engine.sketch_segments(data, off, k, s, stride=need)   # exactly enough
    sc.check_rows(rows, lens, "touching", k, s, cut)
    with pytest.raises(engine.EngineError) as e:
        engine.sketch_segments(data, off, k, s, stride=need - 1)
    assert e.value.code == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as e:                        # offsets that descend
        engine.sketch_segments(data, np.array([0, 50, 40, 90], np.uint64), k, s)
    assert e.value.code == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as e:                        # offsets past the stream
        engine.sketch_segments(data[:100], np.array([0, 50, 101], np.uint64), k, s)
    assert e.value.code == engine.MHX_E_ARG
    with pytest.raises(engine.EngineError) as e:
        engine.sketch_segments(data, off, 33, s)
    assert e.value.code == engine.MHX_E_ARG


def test_no_segments_and_only_empty_ones(cut):
    rows, lens = engine.sketch_segments(b"ACGT" * 10, np.array([0], np.uint64), 21, 10)
    assert rows.shape == (0, 0) and lens.size == 0
    rows, lens = engine.sketch_segments(b"", np.zeros(0, np.uint64), 21, 10)
    assert lens.size == 0
    rows, lens = engine.sketch_segments(b"ACGT" * 10, np.array([0, 0, 20, 20, 40], np.uint64), 21, 10)   # all shorter than k
    assert rows.shape == (4, 0) and not lens.any()
    L = engine.load()
    assert L.mhx_sketch_segments(None, 0, None, 0, 21, 10, None, None, 0, 0) == engine.MHX_OK


def test_result_feeds_dist_batch_without_leaving_the_device(cut):
    import torch

    k, s = 21, 200
    data, off = sc.case("edge_lengths", k, cut)
    keep = [i for i in range(off.size - 1) if int(off[i + 1] - off[i]) >= 63]   # the segments that hold hashes, both routes among them
    stride = 208                                                                # rows of whole 128-byte lines
    d_rows, d_len = _device_call(data, off, k, s, stride)
    dev = d_rows.device
    pick = torch.tensor(keep, device=dev)
    d_rows, d_len = d_rows[pick].contiguous(), d_len[pick].contiguous()         # a gather on the device
    n = len(keep)
    common = torch.zeros((n, n), dtype=torch.int32, device=dev)
    denom = torch.zeros((n, n), dtype=torch.int32, device=dev)
    dist = torch.zeros((n, n), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    engine.dist_batch_device(d_rows.data_ptr(), d_len.data_ptr(), n, d_rows.data_ptr(), d_len.data_ptr(), n, stride, k, s,
                             common.data_ptr(), denom.data_ptr(), dist.data_ptr())
    common, denom, dist = common.cpu().numpy(), denom.cpu().numpy(), dist.cpu().numpy()
    full = [sc.expected_full("edge_lengths", k, cut)[i] for i in keep]
    for qi in range(n):
        for ri in range(n):
            c, d, x = mo.compare(full[ri][:s], full[qi][:s], s, k)
            assert (int(common[qi, ri]), int(denom[qi, ri])) == (c, d), (qi, ri)
            assert abs(dist[qi, ri] - x) <= 2e-16 * max(1.0, abs(x)) + 1e-300   # device log(): <= 1 ulp (as tests/test_gpu_full_size.py)
        assert common[qi, qi] == denom[qi, qi] and dist[qi, qi] == 0.0

"""bench.py --dump-outputs without a GPU: the float64 arrays give back every 64-bit hash exactly, and a sketch beyond the
size budget is written as the same seeded sample of its entries every time, within the budget."""
import importlib.util
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d):
    return {p.stem: np.load(p) for p in Path(d).glob("*.npy")}


def _hashes(got):
    return (got["hashes_hi32"].astype(np.uint64) << np.uint64(32)) | got["hashes_lo32"].astype(np.uint64)


def test_dump_is_exact_and_float64(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(5)
    h = np.sort(rng.integers(0, np.iinfo(np.uint64).max, size=5000, dtype=np.uint64, endpoint=True))
    c = rng.integers(1, 1000, size=5000).astype(np.uint32)
    bench.dump_outputs(str(tmp_path), h, c)
    got = _load(tmp_path)
    assert sorted(got) == ["counts", "hashes_hi32", "hashes_lo32", "index"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(_hashes(got), h) and np.array_equal(got["counts"], c) and np.array_equal(got["index"], np.arange(5000))


def test_dump_beyond_the_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    n = 100_000
    h = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 17)
    c = np.arange(n, dtype=np.uint32) % 7 + 1
    bench.dump_outputs(str(tmp_path / "a"), h, c)
    bench.dump_outputs(str(tmp_path / "b"), h, c)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 1 << 20
    idx = a["index"].astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(_hashes(a), h[idx]) and np.array_equal(a["counts"], c[idx])
    assert all(np.array_equal(a[k], b[k]) for k in a)

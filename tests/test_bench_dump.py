"""bench.py --dump-outputs: what it writes for a set of hit records (host only)."""
import numpy as np

import bench

FIELDS = ("pattern", "pos", "score")


def _records(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=np.dtype([("pos", "<u8"), ("pattern", "<u4"), ("score", "<i4")]))
    r["pos"] = rng.integers(0, 1 << 40, n)
    r["pattern"] = rng.integers(0, 1024, n)
    r["score"] = rng.integers(-3, 1, n)
    return r


def _load(d):
    return {f: np.load(d / f"{f}.npy") for f in FIELDS + ("hit_count",)}


def test_dump_is_float64_in_one_order_whatever_order_the_records_came_in(tmp_path):
    r = _records(5000, 1)
    bench.dump_outputs(str(tmp_path / "a"), r, FIELDS)
    bench.dump_outputs(str(tmp_path / "b"), r[::-1].copy(), FIELDS)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    want = np.sort(r, order=list(FIELDS))
    for f in FIELDS:
        assert a[f].dtype == np.float64
        assert np.array_equal(a[f], b[f])
        assert np.array_equal(a[f], want[f].astype(np.float64))
    assert a["hit_count"].tolist() == [5000.0]


def test_dump_of_a_large_set_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    assert bench.DUMP_MAX_BYTES <= 64_000_000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    r = _records(200_000, 2)
    bench.dump_outputs(str(tmp_path / "a"), r, FIELDS)
    bench.dump_outputs(str(tmp_path / "b"), r[::-1].copy(), FIELDS)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 1 << 20
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert 0 < len(a["pos"]) < len(r)
    assert a["hit_count"].tolist() == [200_000.0]
    for f in FIELDS:
        assert np.array_equal(a[f], b[f])
    order = np.lexsort([a[f] for f in reversed(FIELDS)])     # still in the canonical order
    assert np.array_equal(order, np.arange(len(order)))

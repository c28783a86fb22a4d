"""bench.py --dump-outputs without a GPU: the writer runs on the CPU oracle, which answers `rows` / `get` for the same field
names as the device context."""
import numpy as np

import bench
import workloads as W


class OracleAsDevice:
    def __init__(self, orc, Nh):
        self.orc, self.Nh = orc, Nh

    def rows(self, name):
        return np.asarray(self.orc.get(name)).reshape(-1, self.Nh).shape[0]

    def get(self, name):
        return self.orc.get(name)


def _dump(w, directory, steps=2):
    orc = W.setup_oracle(w)
    orc.run(w["dt"], steps)
    bench.dump_outputs(W, OracleAsDevice(orc, w["Nh"]), w, str(directory))
    return orc


def test_dump_of_a_small_workload_is_every_field_whole(tmp_path):
    lat, lon = W.columns_from_mask("N72")
    sel = np.arange(0, lat.size, 7)
    w = W.make_workload("land", lat[sel], lon[sel], 16, hydraulics="vg")
    orc = _dump(w, tmp_path)
    names = W.compared_fields(w)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in names)
    for n in names:
        a = np.load(tmp_path / f"{n}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, orc.get(n), equal_nan=True), n


def test_dump_of_the_headline_workload_is_a_fixed_column_sample_under_64_MB(tmp_path):
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("richards", lat, lon, 32)
    a, b = tmp_path / "a", tmp_path / "b"
    orc = _dump(w, a)
    _dump(w, b)
    names = W.compared_fields(w)
    assert sum(p.stat().st_size for p in a.iterdir()) < 64 * 10 ** 6
    cols = bench.dump_columns(w["Nh"], sum(np.asarray(orc.get(n)).reshape(-1, w["Nh"]).shape[0] for n in names) * 8)
    assert cols is not None and np.all(np.diff(cols) > 0) and cols.size > w["Nh"] // 2
    for n in names:
        x, y = np.load(a / f"{n}.npy"), np.load(b / f"{n}.npy")
        assert x.dtype == np.float64 and x.shape[-1] == cols.size, n
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, orc.get(n)[..., cols], equal_nan=True), n


def test_fp32_workload_dumps_float32(tmp_path):
    lat, lon = W.synthetic_columns(512)
    w = W.make_workload("land", lat, lon, 64, dtype=np.float32)
    _dump(w, tmp_path)
    for n in W.compared_fields(w):
        a = np.load(tmp_path / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape[-1] == 512, n

"""The one-line JSON contract of bench.py, checked on the line the last GPU run committed under profiles/
(bench.py itself needs a GPU; the schema does not)."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def latest_line():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r01_*_bench.json")))
    assert files, "no committed bench line under profiles/"
    return json.load(open(files[-1])), files[-1]


def test_bench_line_has_the_contract_fields():
    d, path = latest_line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, (k, path)
    assert d["unit"] == "graphs/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    # achieved = algorithmic bytes per launch / mean launch time
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["mean_launch_ms"] * 1e-3) / 1e9) <= 1e-6 * r["achieved"]
    # 4nF + 4nF + 4E + 4(n+1) per graph-layer
    n, E, B = d["config"]["nodes_per_graph"], d["config"]["edges_per_graph"], d["config"]["graphs_per_gpu"]
    assert r["algorithmic_bytes_per_launch"] == (8 * n * 64 + 4 * E + 4 * (n + 1)) * B
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1


def _bench_module():
    """bench.py imported in-process for its host helpers (the environment it sets at import is put back)"""
    import importlib.util
    env = dict(os.environ)
    spec = importlib.util.spec_from_file_location("gnm_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    finally:
        os.environ.clear()
        os.environ.update(env)
    return mod


def test_dump_outputs_writes_every_array_whole_under_the_budget(tmp_path):
    import numpy as np
    bench = _bench_module()
    arrays = {"loss": np.asarray(0.75, dtype=np.float32), "grad.w": np.arange(12, dtype=np.float32).reshape(3, 4)}
    bench.write_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["grad.w.npy", "loss.npy"]
    for name, a in arrays.items():
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == np.float32 and b.shape == a.shape and np.array_equal(a, b)


def test_dump_outputs_samples_a_fixed_subset_over_the_budget(tmp_path):
    import numpy as np
    bench = _bench_module()
    arrays = {"loss": np.asarray(0.75, dtype=np.float32), "grad.big": np.arange(20000, dtype=np.float32),
              "grad.small": np.arange(500, dtype=np.float32).reshape(20, 25)}
    budget = 16384
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), arrays, budget=budget)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["grad.big.npy", "grad.small.npy", "loss.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= budget
    for f in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b)          # the same positions every run
    big = np.load(tmp_path / "a" / "grad.big.npy")
    assert 0 < big.size < 20000 and np.all(np.diff(big) > 0)            # a sorted sample of the real entries
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(0.75)
